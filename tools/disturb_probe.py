"""What a disturbance program costs in an open-loop run, at 10 000 x 8 over 500 steps of 10 s, one fused call each:
  (a) no program (the reference point);
  (b) an all-OFF program: its bits must equal (a)'s;
  (c) OU on inlet pH and inlet chlorine, SINE on inlet temperature, STEP on ambient temperature, with history;
  (d) the boundary series of (c), composed on the host from its history, through step_scheduled (timed with the
      upload the call makes): its bits must equal (c)'s.
The four alternate over five repeats, the order rotating; the medians are reported.  (c) and (d) also integrate the
plant under moving boundaries, so their time is not the evaluation's alone.  Prints one JSON line.
   python tools/disturb_probe.py [N] [n] [steps]"""
import importlib, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import numpy as np
from disturb_ref import compose_rows
wt = importlib.import_module("ics-wt-physicsengine_amd")

N = int(sys.argv[1]) if len(sys.argv) > 1 else 10000
n = int(sys.argv[2]) if len(sys.argv) > 2 else 8
K = int(sys.argv[3]) if len(sys.argv) > 3 else 500
DT = 10.0
cols, bc = wt.make_ensemble(N)
u = np.random.default_rng(3).random((4, N))
MIXED = (wt.Disturbance.ou("inlet_pH", 0.1, 600.0 + 600.0 * u[0]), wt.Disturbance.ou("inlet_chlorine", 0.1, 900.0),
         wt.Disturbance.sine("inlet_temperature", 3.0, 86400.0, phase=6.28 * u[1]),
         wt.Disturbance.step("ambient_temperature", -5.0, 1000.0 + 2000.0 * u[2]))
VARIANTS = {"a": None, "b": (wt.Disturbance("inlet_pH"), wt.Disturbance("ambient_temperature")), "c": MIXED}


def outputs(ens):
    es = ens.state
    return (es.pH, es.chlorine, es.temperature, es.time, es.flow_rate, es.status)


def run(name, sched=None):
    ens = wt.ReactorEnsemble(cols, n_zones=n)
    ens.set_boundary(bc)
    if VARIANTS.get(name) is not None:
        ens.set_disturbances(*VARIANTS[name], seed=7, history=K if name == "c" else 0)
    ens.synchronize()
    t0 = time.perf_counter()
    if name == "d":
        ens.step(DT, n_steps=K, boundary_schedule=sched, download=False)
    else:
        ens.step(DT, n_steps=K, download=False)
    ens.synchronize()
    dt = time.perf_counter() - t0
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
times = {k: [] for k in "abcd"}
orders = ("abcd", "bcda", "cdab", "dabc")
outs = {}
for rep in range(REPEATS):
    for name in orders[rep % 4]:
        t, out, _ = run(name, sched)
        times[name].append(t)
        outs[name] = out
med = {k: float(np.median(v)) for k, v in times.items()}
off_same = all(np.array_equal(x, y, equal_nan=True) for x, y in zip(outs["a"], outs["b"]))
replay_same = all(np.array_equal(x, y, equal_nan=True) for x, y in zip(outs["c"], outs["d"]))
print(json.dumps({"N": N, "n": n, "steps": K, "none_s": round(med["a"], 4), "all_off_s": round(med["b"], 4),
                  "mixed_s": round(med["c"], 4), "scheduled_s": round(med["d"], 4),
                  "all_off_over_none": round(med["b"] / med["a"], 3), "mixed_over_none": round(med["c"] / med["a"], 3),
                  "scheduled_over_none": round(med["d"] / med["a"], 3), "repeats": REPEATS,
                  "schedule_bytes": int(sched.nbytes),
                  "all_s": {k: [round(t, 4) for t in v] for k, v in times.items()},
                  "all_off_bitwise_equal": bool(off_same), "mixed_equals_scheduled_bitwise": bool(replay_same)}))
if not (off_same and replay_same):
    sys.exit(1)
