"""What scripted sensor spoofing under closed-loop PI dosing costs, three ways, at 10 000 x 8 over 120 scans of 10 s:
  (a) the host loop the study needs without the feature: step(dt, 1, fused=False), sensor_readings(), input_image(),
      the injection and the PI update in numpy (tests/inject_ref.py, tests/control_ref.py), write_holding(), every step;
  (b) one fused call with both PI loops and a 4-slot injection program on the device, a scan per step;
  (c) the same call with control only, as the reference point.
(b) and (c) alternate over five repeats, in both orders; the medians are reported (fused times: median of the five).
Checks that (a) and (b) give bitwise the same states, readings, boundaries, controller and injection states, and
prints one JSON line.
   python tools/inject_probe.py [N] [n] [steps]"""
import importlib, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
from control_ref import ControlRef
from inject_ref import InjectRef
from program_helpers import HostScan
wt = importlib.import_module("ics-wt-physicsengine_amd")

N = int(sys.argv[1]) if len(sys.argv) > 1 else 10000
n = int(sys.argv[2]) if len(sys.argv) > 2 else 8
K = int(sys.argv[3]) if len(sys.argv) > 3 else 120
DT = 10.0
cols, bc = wt.make_ensemble(N)
u = np.random.default_rng(3).random((8, N))
chlorine = wt.PILoop("chlorine_outlet", setpoint=cols["initial_chlorine"] + 0.5, kp=0.5 + 1.5 * u[0], ki=1e-3 * u[1], bias=0.2)
acid = wt.PILoop("pH_outlet", setpoint=7.0 + 0.4 * u[2], kp=0.5, ki=1e-4 + 1e-3 * u[3], direction=-1, bias=0.1)
span = K * DT
program = [wt.Injection("chlorine_outlet", "constant", start=0.25 * span, end=0.5 * span, a=0.0),      # spoofed low
           wt.Injection("pH_outlet", "freeze", start=span * u[4], end=span * u[4] + 0.3 * span),         # frozen probe
           wt.Injection("chlorine_outlet", "bias", start=0.6 * span, a=-0.5 * u[5]),
           wt.Injection("pH_inlet", "fault", start=0.8 * span, a=3)]
cblock, iblock = wt.control_block(N, chlorine, acid), wt.injection_block(N, *program)


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
        (ens.boundary(), ens.control_state().block())


warm = plant()                                   # module load, first launches
warm.enable_control(chlorine, acid); warm.set_injections(*program); warm.step(DT, n_steps=2, download=False)
warm.injection_state(); warm.close()


def host_loop():
    ens = plant()
    ctl, inj = ControlRef(cblock, np.zeros(N)), InjectRef(iblock)
    ens.enable_control()                         # both loops off: control_state() is kept for the comparison
    ens.synchronize()
    t0 = time.perf_counter()
    HostScan(N, ctl=ctl, inj=inj, emulated=True, dt=DT).run(ens, K, 1, fused=False, image=True)
    dt = time.perf_counter() - t0
    out = outputs(ens)[:-1]
    ens.close()
    return dt, out + (ctl.st,), inj.st


def fused(inject):
    ens = plant()
    ens.enable_control(chlorine, acid)
    if inject:
        ens.set_injections(*program)
    ens.synchronize()
    t0 = time.perf_counter()
    ens.step(DT, n_steps=K, download=False)
    ens.synchronize()
    dt = time.perf_counter() - t0
    out = outputs(ens)
    st = ens.injection_state().block() if inject else None
    ens.close()
    return dt, out, st


REPEATS = 5
ta, out_a, st_a = host_loop()
tb_all, tc_all = [], []
for rep in range(REPEATS):                       # the two fused variants alternate, in both orders
    for inject in ((True, False) if rep % 2 == 0 else (False, True)):
        t, out, st = fused(inject)
        (tb_all if inject else tc_all).append(t)
        if inject:
            out_b, st_b = out, st
tb, tc = float(np.median(tb_all)), float(np.median(tc_all))
same = all(np.array_equal(a, b, equal_nan=True) for a, b in zip(out_a, out_b)) and np.array_equal(st_a, st_b, equal_nan=True)
print(json.dumps({"N": N, "n": n, "steps": K, "host_loop_s": round(ta, 4), "fused_inject_s": round(tb, 4),
                  "control_only_s": round(tc, 4), "loop_over_fused": round(ta / tb, 2),
                  "inject_over_control": round(tb / tc, 3), "repeats": REPEATS,
                  "fused_inject_all_s": [round(t, 4) for t in tb_all], "control_only_all_s": [round(t, 4) for t in tc_all],
                  "bitwise_equal": bool(same)}))
if not same:
    sys.exit(1)
