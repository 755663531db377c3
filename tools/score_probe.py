"""What a score program costs in an open-loop run, at 10 000 x 8 over 500 steps of 10 s, one fused call each:
  (a) no program (the reference point);
  (b) four all-OFF slots;
  (c) four ZONE slots (outlet chlorine, outlet pH, outlet and inlet-zone temperature);
  (d) four slots with MIN and MEAN among them;
  (e) the slots of (d) with the ensemble curve;
  (f) (e) with a 32-bin fan;
  (g) the route this replaces: record(every=1, capacity=steps), the download and score_ref on the host (timed from
      the step call to the restatement's end).
The seven alternate over five repeats, the order rotating; the medians are reported.  The state of every run must
equal (a)'s bit for bit, the curves of (e) and (f) must agree, and (f)'s rows must equal the restatement's of (g).
Prints one JSON line.
   python tools/score_probe.py [N] [n] [steps]"""
import json, sys, time
import numpy as np
from probe_common import arguments, ensemble, outputs, rotate, same, timed_step, wt
from score_ref import ScoreRef

N, n, K, cols, bc = arguments(500)
DT = 10.0
S = wt.Score
OFF = tuple(S(q, kind="off") for q in ("pH", "chlorine", "temperature", "chlorine"))
ZONE = (S("chlorine", 0.2, 4.0), S("pH", 6.5, 8.5), S("temperature", hi=25.0), S("temperature", hi=25.0, zone=0))
MIXED = (S("chlorine", 0.2, 4.0), S("pH", 6.5, 8.5, reduce="mean"), S("temperature", hi=25.0, reduce="max"),
         S("chlorine", lo=0.5, reduce="min", t_start=1000.0, t_end=4000.0))
FAN = ([0.0, 2.0, 5.0, 0.0], [5.0, 9.0, 35.0, 5.0])
VARIANTS = {"a": None, "b": (OFF, {}), "c": (ZONE, {}), "d": (MIXED, {}), "e": (MIXED, dict(curve=K)),
            "f": (MIXED, dict(curve=K, bins=32, fan_range=FAN)), "g": None}


def run(name, rep=0):
    ens = ensemble(cols, bc, n)
    if VARIANTS[name] is not None:
        ens.set_scores(*VARIANTS[name][0], **VARIANTS[name][1])
    if name == "g":
        ens.record(every=1, capacity=K)
    t0, _ = timed_step(ens, DT, K)
    extra = None
    if name == "g":
        tr = ens.trajectory()
        ref = ScoreRef(wt.score_block(N, *MIXED), np.zeros(N), curve=K, bins=32, fan_lo=FAN[0], fan_hi=FAN[1])
        ref.run(tr.pH, tr.chlorine, tr.temperature, tr.time, tr.status)
        extra = (ref.st, ref.counts, ref.fan)
    dt = time.perf_counter() - t0
    if name in "ef":
        c = ens.score_curve()
        st = ens.score_state()
        extra = (np.stack([getattr(st, k) for k in wt.core.score.STATE_ROWS], axis=1),
                 np.stack([c.n_scored, c.n_low, c.n_high], axis=2), c.fan)
    out = outputs(ens)
    ens.close()
    return dt, out, extra


run("f")                                         # module load, first launches
REPEATS = 5
names = "abcdefg"
times, med, last = rotate(names, REPEATS, run)
extras = {k: last[k][2] for k in names}
equal = all(same(last["a"][1], last[k][1]) for k in names[1:])
curves = np.array_equal(extras["e"][1], extras["f"][1])
exact = same(extras["f"], extras["g"])
labels = {"a": "none", "b": "all_off", "c": "zone", "d": "mixed", "e": "curve", "f": "fan", "g": "record_and_host"}
res = {"N": N, "n": n, "steps": K, "repeats": REPEATS}
res.update({labels[k] + "_s": round(med[k], 4) for k in names})
res.update({labels[k] + "_over_none": round(med[k] / med["a"], 3) for k in names[1:]})
res.update({"record_bytes": int(K * N * (3 * n + 2) * 8 + K * N * 4),
            "all_s": {k: [round(t, 4) for t in v] for k, v in times.items()},
            "state_bitwise_equal": bool(equal), "curve_equals_fan_run": bool(curves), "fan_run_equals_restatement": bool(exact)})
print(json.dumps(res))
if not (equal and curves and exact):
    sys.exit(1)
