"""What a trend recorder program costs under closed-loop PI dosing with a scan per step, at 10 000 x 8 over 500 steps of
1 s after 100 warm-up steps (the shape of `bench.py --plant-io --chunk 1`), one fused call each:
  (a) no trend program, the reference point;
  (b) eight OFF slots (the section's fixed cost: the flag and eight tag loads);
  (c) one slot, every = 1, capacity 512: the chlorine loop's output;
  (d) eight slots, every = 1, capacity 512: a reading, its field twin, a command, both PI outputs, an ISE, the alarm
      word (no alarm program: NaN) and a fault code.
A recorded sample is one 16-byte store, so (c) writes 16 and (d) 128 bytes per reactor-scan, next to 32 bytes of slot
state read and written per slot.  The warm-up call is the ensemble's first (a first call after a set call carries a
20 ... 25 ms outlier now and then, with or without slots that record); reset_trends() then empties the store.  The four
alternate over nine repeats in rotating order; the medians and the minima of the step call alone are reported, with the
time of one download of the whole store (all eight slots' capacity, used or not).  Checks that every plant state of
(b), (c) and (d) is bitwise (a)'s and that (c)'s series is (d)'s, and prints one JSON line.
   python tools/trend_probe.py [N] [n] [steps]"""
import importlib, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
wt = importlib.import_module("ics-wt-physicsengine_amd")

N = int(sys.argv[1]) if len(sys.argv) > 1 else 10000
n = int(sys.argv[2]) if len(sys.argv) > 2 else 8
K = int(sys.argv[3]) if len(sys.argv) > 3 else 500
DT, CAPACITY, WARMUP = 1.0, 512, 100
cols, bc = wt.make_ensemble(N)
u = np.random.default_rng(3).random((4, N))
chlorine = wt.PILoop("chlorine_outlet", setpoint=cols["initial_chlorine"] + 0.5, kp=0.5 + 1.5 * u[0], ki=1e-3 * u[1], bias=0.2)
acid = wt.PILoop("pH_outlet", setpoint=7.0 + 0.4 * u[2], kp=0.5, ki=1e-4 + 1e-3 * u[3], direction=-1, bias=0.1)
one = [wt.Trend("control", ("chlorine", "output"))]
eight = one + [wt.Trend("image_value", "chlorine_outlet"), wt.Trend("field_value", "chlorine_outlet"), wt.Trend("command", "chlorine"),
               wt.Trend("control", ("acid", "output")), wt.Trend("control", ("chlorine", "ise")), wt.Trend("alarm_word"),
               wt.Trend("image_fault", "pH_outlet")]
off = [wt.Trend("off")] * 8


def outputs(ens):
    es = ens.state
    return (es.pH, es.chlorine, es.temperature, es.time, es.flow_rate, es.status) + ens.sensor_readings() + ens.input_image() + \
        (ens.boundary(), ens.control_state().block())


def run(variant, download=False):
    ens = wt.ReactorEnsemble(cols, n_zones=n)
    ens.set_boundary(bc)
    ens.enable_sensors(seed=1)
    ens.enable_plant_io()
    ens.set_schedule(0, 1)
    ens.enable_control(chlorine, acid)
    if variant != "none":
        ens.set_trends(*{"off": off, "one": one, "eight": eight}[variant], capacity=CAPACITY)
    ens.step(DT, n_steps=WARMUP, download=False)
    if variant != "none":
        ens.reset_trends()
    ens.synchronize()
    t0 = time.perf_counter()
    ens.step(DT, n_steps=K, download=False)
    ens.synchronize()
    t_step = time.perf_counter() - t0
    data, t_data = None, 0.0
    if download:
        t0 = time.perf_counter()
        data = ens.trend_data()
        t_data = time.perf_counter() - t0
    out = outputs(ens)
    ens.close()
    return t_step, t_data, out, data


run("none")                                      # module load, first launches
VARIANTS, REPEATS = ("none", "off", "one", "eight"), 9
times, downloads, outs, data = {v: [] for v in VARIANTS}, {}, {}, {}
for rep in range(REPEATS):
    for i in range(len(VARIANTS)):
        v = VARIANTS[(i + rep) % len(VARIANTS)]
        t, t_data, outs[v], d = run(v, download=rep == REPEATS - 1 and v in ("one", "eight"))      # the series once, at the end
        times[v].append(t)
        if d is not None:
            data[v], downloads[v] = d, t_data
med = {v: float(np.median(times[v])) for v in VARIANTS}
same = lambda a, b: all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a, b))
plant_equal = all(same(outs["none"], outs[v]) for v in VARIANTS[1:])
series_equal = same((data["one"].time[0], data["one"].value[0]), (data["eight"].time[0], data["eight"].value[0]))
held = data["eight"].count
print(json.dumps({"N": N, "n": n, "steps": K, "warmup": WARMUP, "capacity": CAPACITY, "repeats": REPEATS, "none_s": round(med["none"], 4),
                  "off_s": round(med["off"], 4), "one_s": round(med["one"], 4), "eight_s": round(med["eight"], 4),
                  "off_over_none": round(med["off"] / med["none"], 3), "one_over_none": round(med["one"] / med["none"], 3),
                  "eight_over_none": round(med["eight"] / med["none"], 3),
                  "min_s": {v: round(min(times[v]), 4) for v in VARIANTS},
                  "step_all_s": {v: [round(t, 4) for t in times[v]] for v in VARIANTS},
                  "data_download_s": {v: round(downloads[v], 3) for v in ("one", "eight")},
                  "bytes_per_reactor_scan": {"one": 16, "eight": 128}, "samples_held_min_max": [int(held.min()), int(held.max())],
                  "plant_bitwise_equal": bool(plant_equal), "series_bitwise_equal": bool(series_equal)}))
if not (plant_equal and series_equal):
    sys.exit(1)
