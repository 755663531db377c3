"""What an actuator program costs under closed-loop PI dosing, at 10 000 x 8 over 120 steps of 10 s with a scan per
step, one fused call each:
  (a) both PI loops, no actuator program (the reference point);
  (b) the same with pass-through elements (the defaults) on all three channels: its bits must equal (a)'s;
  (c) the same with realistic elements: lags of 30-120 s, rate limits, dead times of 1-3 scans, backlash, and a
      chlorine pump stuck from t = 600 s in 5 % of the reactors.
The three alternate over five repeats, the order rotating; the medians are reported.  (c) also integrates the plant
under different doses, so its time is not the evaluation's alone.  Prints one JSON line.
   python tools/actuator_probe.py [N] [n] [steps]"""
import importlib, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
wt = importlib.import_module("ics-wt-physicsengine_amd")

N = int(sys.argv[1]) if len(sys.argv) > 1 else 10000
n = int(sys.argv[2]) if len(sys.argv) > 2 else 8
K = int(sys.argv[3]) if len(sys.argv) > 3 else 120
DT = 10.0
cols, bc = wt.make_ensemble(N)
u = np.random.default_rng(3).random((12, N))
chlorine = wt.PILoop("chlorine_outlet", setpoint=cols["initial_chlorine"] + 0.5, kp=0.5 + 1.5 * u[0], ki=1e-3 * u[1], bias=0.2)
acid = wt.PILoop("pH_outlet", setpoint=7.0 + 0.4 * u[2], kp=0.5, ki=1e-4 + 1e-3 * u[3], direction=-1, bias=0.1)
passthrough = [wt.Actuator("acid"), wt.Actuator("chlorine"), wt.Actuator("inlet")]
realistic = [wt.Actuator("acid", tau=30.0 + 90.0 * u[4], rate=0.002 + 0.01 * u[5], backlash=0.02,
                         delay=1 + (u[6] * 3).astype(int) % 3),
             wt.Actuator("chlorine", tau=30.0 + 90.0 * u[7], rate=0.001 + 0.005 * u[8], delay=1 + (u[9] * 3).astype(int) % 3,
                         fault=np.where(u[10] < 0.05, "stuck", "none"), t_fault=600.0),
             wt.Actuator("inlet", tau=60.0, rate=0.05, delay=1)]
VARIANTS = {"a": None, "b": passthrough, "c": realistic}


def plant():
    ens = wt.ReactorEnsemble(cols, n_zones=n)
    ens.set_boundary(bc)
    ens.enable_sensors(seed=1)
    ens.enable_plant_io()
    ens.set_schedule(0, 1)
    ens.write_commands(0.5, 0.25, 6.0)
    ens.enable_control(chlorine, acid)
    return ens


def outputs(ens):
    es = ens.state
    return (es.pH, es.chlorine, es.temperature, es.time, es.flow_rate, es.status) + ens.sensor_readings() + \
        (ens.boundary(), ens.control_state().block()) + ens.input_image()


def run(name):
    ens = plant()
    if VARIANTS[name] is not None:
        ens.set_actuators(*VARIANTS[name])
    ens.synchronize()
    t0 = time.perf_counter()
    ens.step(DT, n_steps=K, download=False)
    ens.synchronize()
    dt = time.perf_counter() - t0
    out = outputs(ens)
    st = ens.actuator_state() if VARIANTS[name] is not None else None
    ens.close()
    return dt, out, st


run("c")                                         # module load, first launches
REPEATS = 5
times = {k: [] for k in VARIANTS}
orders = ("abc", "bca", "cab")
for rep in range(REPEATS):
    for name in orders[rep % 3]:
        t, out, st = run(name)
        times[name].append(t)
        if name == "a":
            out_a = out
        elif name == "b":
            out_b = out
        else:
            st_c = st
med = {k: float(np.median(v)) for k, v in times.items()}
same = all(np.array_equal(x, y, equal_nan=True) for x, y in zip(out_a, out_b))
print(json.dumps({"N": N, "n": n, "steps": K, "control_only_s": round(med["a"], 4), "passthrough_s": round(med["b"], 4),
                  "realistic_s": round(med["c"], 4), "passthrough_over_control": round(med["b"] / med["a"], 3),
                  "realistic_over_control": round(med["c"] / med["a"], 3), "repeats": REPEATS,
                  "stuck_reactors": int(np.sum(st_c.n_fault[1] > 0)),
                  "rate_limited_scans": int(st_c.n_rate.sum()),
                  "all_s": {k: [round(t, 4) for t in v] for k, v in times.items()},
                  "passthrough_bitwise_equal": bool(same)}))
if not same:
    sys.exit(1)
