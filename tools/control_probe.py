"""What closed-loop PI dosing with a scan per outer step costs, three ways, at 10 000 x 8 over 120 steps of 10 s:
  (a) the host loop closed-loop control needs without the feature: step(dt, 1, fused=False), sensor_readings(),
      input_image(), the PI update in numpy (tests/control_ref.py), write_holding(), every step;
  (b) one fused call with both PI loops on the device (ReactorEnsemble.enable_control), a scan per step;
  (c) the same call with plant I/O but no control, as the reference point;
  (d) the call of (b) with kp = ki = bias = 0: the controller runs but commands nothing, so the plant is (c)'s --
      (d) over (c) is the controller's own cost, (b) over (d) what the dosing does to the solver.
Checks that (a) and (b), and (c) and (d), give bitwise the same states, readings, images and boundaries ((a) and (b)
also the same controller state), and prints one JSON line.
   python tools/control_probe.py [N] [n] [steps]"""
import importlib, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
from control_ref import ControlRef
from program_helpers import HostScan
wt = importlib.import_module("ics-wt-physicsengine_amd")

N = int(sys.argv[1]) if len(sys.argv) > 1 else 10000
n = int(sys.argv[2]) if len(sys.argv) > 2 else 8
K = int(sys.argv[3]) if len(sys.argv) > 3 else 120
DT = 10.0
cols, bc = wt.make_ensemble(N)
u = np.random.default_rng(3).random((4, N))
chlorine = wt.PILoop("chlorine_outlet", setpoint=cols["initial_chlorine"] + 0.5, kp=0.5 + 1.5 * u[0], ki=1e-3 * u[1], bias=0.2)
acid = wt.PILoop("pH_outlet", setpoint=7.0 + 0.4 * u[2], kp=0.5, ki=1e-4 + 1e-3 * u[3], direction=-1, bias=0.1)
block = wt.control_block(N, chlorine, acid)
idle = dict(chlorine=wt.PILoop("chlorine_outlet", setpoint=chlorine.setpoint), acid=wt.PILoop("pH_outlet", setpoint=7.0, direction=-1))


def plant():
    ens = wt.ReactorEnsemble(cols, n_zones=n)
    ens.set_boundary(bc)
    ens.enable_sensors(seed=1)
    ens.enable_plant_io()
    ens.set_schedule(0, 1)
    return ens


def outputs(ens):
    es = ens.state
    return (es.pH, es.chlorine, es.temperature, es.time, es.flow_rate, es.status) + ens.sensor_readings() + \
        ens.input_image() + (ens.boundary(),)


warm = plant()                                   # module load, first launches
warm.enable_control(chlorine, acid); warm.step(DT, n_steps=2, download=False); warm.control_state(); warm.close()


def host_loop():
    ens = plant()
    ref = ControlRef(block, np.zeros(N))
    ens.synchronize()
    t0 = time.perf_counter()
    HostScan(N, ctl=ref, emulated=True, dt=DT).run(ens, K, 1, fused=False, image=True)
    dt = time.perf_counter() - t0
    out = outputs(ens)
    ens.close()
    return dt, out, ref.st


def fused(control):
    ens = plant()
    if control:
        ens.enable_control(**control)
    ens.synchronize()
    t0 = time.perf_counter()
    ens.step(DT, n_steps=K, download=False)
    ens.synchronize()
    dt = time.perf_counter() - t0
    out = outputs(ens)
    st = ens.control_state().block() if control else None
    ens.close()
    return dt, out, st


ta, out_a, st_a = host_loop()
tb, out_b, st_b = fused(dict(chlorine=chlorine, acid=acid))
tc, out_c, _ = fused(None)
td, out_d, _ = fused(idle)
same = all(np.array_equal(a, b, equal_nan=True) for a, b in zip(out_a, out_b)) and np.array_equal(st_a, st_b)
same_idle = all(np.array_equal(a, b, equal_nan=True) for a, b in zip(out_c, out_d))
print(json.dumps({"N": N, "n": n, "steps": K, "host_loop_s": round(ta, 4), "fused_control_s": round(tb, 4),
                  "plant_io_only_s": round(tc, 4), "idle_control_s": round(td, 4), "loop_over_fused": round(ta / tb, 2),
                  "control_over_plant_io": round(tb / tc, 3), "idle_control_over_plant_io": round(td / tc, 3),
                  "bitwise_equal": bool(same), "idle_bitwise_equal_plant_io": bool(same_idle)}))
if not (same and same_idle):
    sys.exit(1)
