"""What an actuator program costs under closed-loop PI dosing, at 10 000 x 8 over 120 steps of 10 s with a scan per
step, one fused call each:
  (a) both PI loops, no actuator program (the reference point);
  (b) the same with pass-through elements (the defaults) on all three channels: its bits must equal (a)'s;
  (c) the same with realistic elements: lags of 30-120 s, rate limits, dead times of 1-3 scans, backlash, and a
      chlorine pump stuck from t = 600 s in 5 % of the reactors.
The three alternate over five repeats, the order rotating; the medians are reported.  (c) also integrates the plant
under different doses, so its time is not the evaluation's alone.  Prints one JSON line.
   python tools/actuator_probe.py [N] [n] [steps]"""
import json, sys
import numpy as np
from probe_common import arguments, outputs, pi_loops, plant, rotate, same, timed_step, wt

N, n, K, cols, bc = arguments(120)
DT = 10.0
chlorine, acid, u = pi_loops(cols, N, 12)
passthrough = [wt.Actuator("acid"), wt.Actuator("chlorine"), wt.Actuator("inlet")]
realistic = [wt.Actuator("acid", tau=30.0 + 90.0 * u[4], rate=0.002 + 0.01 * u[5], backlash=0.02,
                         delay=1 + (u[6] * 3).astype(int) % 3),
             wt.Actuator("chlorine", tau=30.0 + 90.0 * u[7], rate=0.001 + 0.005 * u[8], delay=1 + (u[9] * 3).astype(int) % 3,
                         fault=np.where(u[10] < 0.05, "stuck", "none"), t_fault=600.0),
             wt.Actuator("inlet", tau=60.0, rate=0.05, delay=1)]
VARIANTS = {"a": None, "b": passthrough, "c": realistic}


def run(name, rep=0):
    ens = plant(cols, bc, n)
    ens.write_commands(0.5, 0.25, 6.0)
    ens.enable_control(chlorine, acid)
    if VARIANTS[name] is not None:
        ens.set_actuators(*VARIANTS[name])
    _, dt = timed_step(ens, DT, K)
    out = outputs(ens, "sensor_readings", "boundary", "control_state", "input_image")
    st = ens.actuator_state() if VARIANTS[name] is not None else None
    ens.close()
    return dt, out, st


run("c")                                         # module load, first launches
REPEATS = 5
times, med, last = rotate("abc", REPEATS, run)
st_c = last["c"][2]
equal = same(last["a"][1], last["b"][1])
print(json.dumps({"N": N, "n": n, "steps": K, "control_only_s": round(med["a"], 4), "passthrough_s": round(med["b"], 4),
                  "realistic_s": round(med["c"], 4), "passthrough_over_control": round(med["b"] / med["a"], 3),
                  "realistic_over_control": round(med["c"] / med["a"], 3), "repeats": REPEATS,
                  "stuck_reactors": int(np.sum(st_c.n_fault[1] > 0)),
                  "rate_limited_scans": int(st_c.n_rate.sum()),
                  "all_s": {k: [round(t, 4) for t in v] for k, v in times.items()},
                  "passthrough_bitwise_equal": bool(equal)}))
if not equal:
    sys.exit(1)
