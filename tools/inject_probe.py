"""What scripted sensor spoofing under closed-loop PI dosing costs, three ways, at 10 000 x 8 over 120 scans of 10 s:
  (a) the host loop the study needs without the feature: step(dt, 1, fused=False), sensor_readings(), input_image(),
      the injection and the PI update in numpy (tests/inject_ref.py, tests/control_ref.py), write_holding(), every step;
  (b) one fused call with both PI loops and a 4-slot injection program on the device, a scan per step;
  (c) the same call with control only, as the reference point.
(b) and (c) alternate over five repeats, in both orders; the medians are reported (fused times: median of the five).
Checks that (a) and (b) give bitwise the same states, readings, boundaries, controller and injection states, and
prints one JSON line.
   python tools/inject_probe.py [N] [n] [steps]"""
import json, sys, time
import numpy as np
from probe_common import arguments, injections, outputs, pi_loops, plant, rotate, same, timed_step, wt
from control_ref import ControlRef
from inject_ref import InjectRef
from program_helpers import HostScan

N, n, K, cols, bc = arguments(120)
DT = 10.0
chlorine, acid, u = pi_loops(cols, N, 8)
program = injections(u, K * DT)
cblock, iblock = wt.control_block(N, chlorine, acid), wt.injection_block(N, *program)

OUT = ("sensor_readings", "boundary", "control_state")

warm = plant(cols, bc, n)                                   # module load, first launches
warm.enable_control(chlorine, acid); warm.set_injections(*program); warm.step(DT, n_steps=2, download=False)
warm.injection_state(); warm.close()


def host_loop():
    ens = plant(cols, bc, n)
    ctl, inj = ControlRef(cblock, np.zeros(N)), InjectRef(iblock)
    ens.enable_control()                         # both loops off: control_state() is kept for the comparison
    ens.synchronize()
    t0 = time.perf_counter()
    HostScan(N, ctl=ctl, inj=inj, emulated=True, dt=DT).run(ens, K, 1, fused=False, image=True)
    dt = time.perf_counter() - t0
    out = outputs(ens, *OUT)[:-1]
    ens.close()
    return dt, out + (ctl.st,), inj.st


def fused(inject, rep):
    ens = plant(cols, bc, n)
    ens.enable_control(chlorine, acid)
    if inject:
        ens.set_injections(*program)
    _, dt = timed_step(ens, DT, K)
    out = outputs(ens, *OUT)
    st = ens.injection_state().block() if inject else None
    ens.close()
    return dt, out, st


REPEATS = 5
ta, out_a, st_a = host_loop()
times, med, last = rotate((True, False), REPEATS, fused)     # the two fused variants alternate, in both orders
tb_all, tc_all, tb, tc = times[True], times[False], med[True], med[False]
_, out_b, st_b = last[True]
equal = same(out_a, out_b) and np.array_equal(st_a, st_b, equal_nan=True)
print(json.dumps({"N": N, "n": n, "steps": K, "host_loop_s": round(ta, 4), "fused_inject_s": round(tb, 4),
                  "control_only_s": round(tc, 4), "loop_over_fused": round(ta / tb, 2),
                  "inject_over_control": round(tb / tc, 3), "repeats": REPEATS,
                  "fused_inject_all_s": [round(t, 4) for t in tb_all], "control_only_all_s": [round(t, 4) for t in tc_all],
                  "bitwise_equal": bool(equal)}))
if not equal:
    sys.exit(1)
