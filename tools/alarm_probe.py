"""What an alarm and interlock program costs under spoofing and closed-loop PI dosing, three ways, at 10 000 x 8 over
120 scans of 10 s:
  (a) the host loop the study needs without the feature: step(dt, 1, fused=False), sensor_readings(), input_image(),
      the injection, PI and alarm updates in numpy (tests/inject_ref.py, control_ref.py, alarm_ref.py) and a
      write_holding() of the PI words with the tripped channels replaced by float32(trip value), every step;
  (b) one fused call with both PI loops, the 4-slot injection program of inject_probe.py and a 4-slot alarm program
      (one FIELD trip that fires) on the device, a scan per step;
  (c) the same call without the alarm program, as the reference point.
(b) and (c) alternate over five repeats, in both orders; the medians are reported.  Checks that (a) and (b) give
bitwise the same states, readings, boundaries, controller, injection and alarm states and alarm words, and prints one
JSON line.
   python tools/alarm_probe.py [N] [n] [steps]"""
import json, sys, time
import numpy as np
from probe_common import arguments, injections, outputs, pi_loops, plant, rotate, same, timed_step, wt
from alarm_ref import AlarmRef
from control_ref import ControlRef
from inject_ref import InjectRef
from program_helpers import HostScan

N, n, K, cols, bc = arguments(120)
DT = 10.0
chlorine, acid, u = pi_loops(cols, N, 8)
program = injections(u, K * DT)
cl0 = np.asarray(cols["initial_chlorine"])
alarms = [wt.Alarm("chlorine_outlet", "high", cl0 + 0.8, deadband=0.1, on_delay=30.0, latch=True, source="field",
                   action="trip_chlorine", trip_value=0.05),                                         # the trip that fires
          wt.Alarm("chlorine_outlet", "low", cl0 - 0.5, deadband=0.1, on_delay=60.0),
          wt.Alarm("pH_outlet", "low", 6.0, deadband=0.2, source="field", action="trip_acid", trip_value=0.0),
          wt.Alarm("pH_inlet", "high", 9.5, on_bad="alarm")]
cblock, iblock, ablock = wt.control_block(N, chlorine, acid), wt.injection_block(N, *program), wt.alarm_block(N, *alarms)

OUT = ("sensor_readings", "boundary", "control_state")

warm = plant(cols, bc, n)                                   # module load, first launches
warm.enable_control(chlorine, acid); warm.set_injections(*program); warm.set_alarms(*alarms)
warm.step(DT, n_steps=2, download=False); warm.alarm_state(); warm.close()


def host_loop():
    ens = plant(cols, bc, n)
    ctl, inj, alm = ControlRef(cblock, np.zeros(N)), InjectRef(iblock), AlarmRef(ablock, np.zeros(N))
    ens.enable_control()                         # both loops off: control_state() is kept for the comparison
    ens.synchronize()
    t0 = time.perf_counter()
    HostScan(N, ctl=ctl, inj=inj, alm=alm, emulated=True, dt=DT).run(ens, K, 1, fused=False, image=True)
    dt = time.perf_counter() - t0
    out = outputs(ens, *OUT)[:-1]
    ens.close()
    return dt, out + (ctl.st,), (inj.st, alm.st, alm.rst, alm.words)


def fused(alarm, rep):
    ens = plant(cols, bc, n)
    ens.enable_control(chlorine, acid)
    ens.set_injections(*program)
    if alarm:
        ens.set_alarms(*alarms)
    _, dt = timed_step(ens, DT, K)
    out = outputs(ens, *OUT)
    st = (ens.injection_state().block(),) + ens.alarm_state().block() + (ens.alarm_words(),) if alarm else None
    ens.close()
    return dt, out, st


REPEATS = 5
ta, out_a, st_a = host_loop()
times, med, last = rotate((True, False), REPEATS, fused)     # the two fused variants alternate, in both orders
tb_all, tc_all, tb, tc = times[True], times[False], med[True], med[False]
_, out_b, st_b = last[True]
equal = same(out_a, out_b) and same(st_a, st_b)
trips = int(np.sum(st_a[2][4:]))
print(json.dumps({"N": N, "n": n, "steps": K, "host_loop_s": round(ta, 4), "fused_alarm_s": round(tb, 4),
                  "without_alarm_s": round(tc, 4), "loop_over_fused": round(ta / tb, 2),
                  "alarm_over_without": round(tb / tc, 3), "repeats": REPEATS,
                  "reactors_tripped": int(np.sum(st_a[1][0, 3] > 0)), "overridden_scans": trips,
                  "fused_alarm_all_s": [round(t, 4) for t in tb_all], "without_alarm_all_s": [round(t, 4) for t in tc_all],
                  "bitwise_equal": bool(equal)}))
if not equal:
    sys.exit(1)
