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
import json, sys, time
import numpy as np
from probe_common import arguments, outputs, pi_loops, plant, same, timed_step, wt
from control_ref import ControlRef
from program_helpers import HostScan

N, n, K, cols, bc = arguments(120)
DT = 10.0
chlorine, acid, _ = pi_loops(cols, N)
block = wt.control_block(N, chlorine, acid)
idle = dict(chlorine=wt.PILoop("chlorine_outlet", setpoint=chlorine.setpoint), acid=wt.PILoop("pH_outlet", setpoint=7.0, direction=-1))

OUT = ("sensor_readings", "input_image", "boundary")

warm = plant(cols, bc, n)                                   # module load, first launches
warm.enable_control(chlorine, acid); warm.step(DT, n_steps=2, download=False); warm.control_state(); warm.close()


def host_loop():
    ens = plant(cols, bc, n)
    ref = ControlRef(block, np.zeros(N))
    ens.synchronize()
    t0 = time.perf_counter()
    HostScan(N, ctl=ref, emulated=True, dt=DT).run(ens, K, 1, fused=False, image=True)
    dt = time.perf_counter() - t0
    out = outputs(ens, *OUT)
    ens.close()
    return dt, out, ref.st


def fused(control):
    ens = plant(cols, bc, n)
    if control:
        ens.enable_control(**control)
    _, dt = timed_step(ens, DT, K)
    out = outputs(ens, *OUT)
    st = ens.control_state().block() if control else None
    ens.close()
    return dt, out, st


ta, out_a, st_a = host_loop()
tb, out_b, st_b = fused(dict(chlorine=chlorine, acid=acid))
tc, out_c, _ = fused(None)
td, out_d, _ = fused(idle)
equal, equal_idle = same(out_a, out_b) and np.array_equal(st_a, st_b), same(out_c, out_d)
print(json.dumps({"N": N, "n": n, "steps": K, "host_loop_s": round(ta, 4), "fused_control_s": round(tb, 4),
                  "plant_io_only_s": round(tc, 4), "idle_control_s": round(td, 4), "loop_over_fused": round(ta / tb, 2),
                  "control_over_plant_io": round(tb / tc, 3), "idle_control_over_plant_io": round(td / tc, 3),
                  "bitwise_equal": bool(equal), "idle_bitwise_equal_plant_io": bool(equal_idle)}))
if not (equal and equal_idle):
    sys.exit(1)
