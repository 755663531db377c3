"""What a per-step boundary schedule with a recorded trajectory costs, three ways, at 10 000 x 8 over 120 steps:
  (a) the host loop a scenario study needs without the feature: set_boundary(row k), step(dt, 1), state, every step;
  (b) one scheduled call recording every step (ReactorEnsemble.step(boundary_schedule=S) + record(1)), then trajectory();
  (c) a constant-boundary fused call of the same length, as the reference point.
Checks that (a) and (b) give bitwise the same states and prints one JSON line.
   python tools/forcing_probe.py [N] [n] [steps]"""
import importlib, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
wt = importlib.import_module("ics-wt-physicsengine_amd")

N = int(sys.argv[1]) if len(sys.argv) > 1 else 10000
n = int(sys.argv[2]) if len(sys.argv) > 2 else 8
K = int(sys.argv[3]) if len(sys.argv) > 3 else 120
cols, bc = wt.make_ensemble(N)
S = wt.make_boundary_schedule(bc, K, seed=1)

warm = wt.ReactorEnsemble(cols, n_zones=n)          # module load, first launches
warm.record(every=1, capacity=2)
warm.step(1.0, n_steps=2, boundary_schedule=S[:2]); warm.trajectory(); warm.close()


def host_loop():
    ens = wt.ReactorEnsemble(cols, n_zones=n)
    ens.synchronize()
    t0 = time.perf_counter()
    out = []
    for k in range(K):
        ens.set_boundary(S[k])
        es = ens.step(1.0, n_steps=1)
        out.append((es.pH, es.chlorine, es.temperature, es.time, es.flow_rate, es.status))
    dt = time.perf_counter() - t0
    ens.close()
    return dt, out


def scheduled():
    ens = wt.ReactorEnsemble(cols, n_zones=n)
    ens.record(every=1, capacity=K)
    ens.synchronize()
    t0 = time.perf_counter()
    ens.step(1.0, n_steps=K, boundary_schedule=S, download=False)
    tr = ens.trajectory()
    dt = time.perf_counter() - t0
    ens.close()
    return dt, tr


def constant():
    ens = wt.ReactorEnsemble(cols, n_zones=n)
    ens.set_boundary(S[0])
    ens.synchronize()
    t0 = time.perf_counter()
    ens.step(1.0, n_steps=K, download=False)
    ens.synchronize()
    dt = time.perf_counter() - t0
    ens.close()
    return dt


ta, loop = host_loop()
tb, tr = scheduled()
tc = constant()
same = len(tr) == K and all(
    np.array_equal(a, b, equal_nan=True)
    for k in range(K) for a, b in zip(loop[k], (tr.pH[k], tr.chlorine[k], tr.temperature[k], tr.time[k], tr.flow_rate[k], tr.status[k])))
print(json.dumps({"N": N, "n": n, "steps": K, "host_loop_s": round(ta, 4), "scheduled_recorded_s": round(tb, 4),
                  "constant_fused_s": round(tc, 4), "loop_over_scheduled": round(ta / tb, 2),
                  "scheduled_over_constant": round(tb / tc, 3), "bitwise_equal": bool(same)}))
if not same:
    sys.exit(1)
