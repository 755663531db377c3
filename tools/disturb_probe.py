"""What a disturbance program costs in an open-loop run, at 10 000 x 8 over 500 steps of 10 s, one fused call each:
  (a) no program (the reference point);
  (b) an all-OFF program: its bits must equal (a)'s;
  (c) OU on inlet pH and inlet chlorine, SINE on inlet temperature, STEP on ambient temperature, with history;
  (d) the boundary series of (c), composed on the host from its history, through step_scheduled (timed with the
      upload the call makes): its bits must equal (c)'s.
The four alternate over five repeats, the order rotating; the medians are reported.  (c) and (d) also integrate the
plant under moving boundaries, so their time is not the evaluation's alone.  Prints one JSON line.
   python tools/disturb_probe.py [N] [n] [steps]"""
import json, sys
import numpy as np
from probe_common import arguments, ensemble, outputs, rotate, same, timed_step, wt
from disturb_ref import compose_rows

N, n, K, cols, bc = arguments(500)
DT = 10.0
u = np.random.default_rng(3).random((4, N))
MIXED = (wt.Disturbance.ou("inlet_pH", 0.1, 600.0 + 600.0 * u[0]), wt.Disturbance.ou("inlet_chlorine", 0.1, 900.0),
         wt.Disturbance.sine("inlet_temperature", 3.0, 86400.0, phase=6.28 * u[1]),
         wt.Disturbance.step("ambient_temperature", -5.0, 1000.0 + 2000.0 * u[2]))
VARIANTS = {"a": None, "b": (wt.Disturbance("inlet_pH"), wt.Disturbance("ambient_temperature")), "c": MIXED}


def run(name, rep=0):
    ens = ensemble(cols, bc, n)
    if VARIANTS.get(name) is not None:
        ens.set_disturbances(*VARIANTS[name], seed=7, history=K if name == "c" else 0)
    _, dt = timed_step(ens, DT, K, **(dict(boundary_schedule=sched) if name == "d" else {}))
    out = outputs(ens)
    extra = None
    if name == "c":
        off, _ = ens.disturbance_history()
        base = ens.disturbance_state().base
        params = wt.disturbance_block(N, *MIXED)
        extra = np.stack([compose_rows(params, base, off[k]) for k in range(K)])
    ens.close()
    return dt, out, extra


_, _, sched = run("c")                           # module load, first launches, the schedule of (d)
REPEATS = 5
times, med, last = rotate("abcd", REPEATS, run)
off_same, replay_same = same(last["a"][1], last["b"][1]), same(last["c"][1], last["d"][1])
print(json.dumps({"N": N, "n": n, "steps": K, "none_s": round(med["a"], 4), "all_off_s": round(med["b"], 4),
                  "mixed_s": round(med["c"], 4), "scheduled_s": round(med["d"], 4),
                  "all_off_over_none": round(med["b"] / med["a"], 3), "mixed_over_none": round(med["c"] / med["a"], 3),
                  "scheduled_over_none": round(med["d"] / med["a"], 3), "repeats": REPEATS,
                  "schedule_bytes": int(sched.nbytes),
                  "all_s": {k: [round(t, 4) for t in v] for k, v in times.items()},
                  "all_off_bitwise_equal": bool(off_same), "mixed_equals_scheduled_bitwise": bool(replay_same)}))
if not (off_same and replay_same):
    sys.exit(1)
