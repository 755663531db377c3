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
import json, sys, time
import numpy as np
from probe_common import arguments, outputs, pi_loops, plant, rotate, same, timed_step, wt

N, n, K, cols, bc = arguments(500)
DT, CAPACITY, WARMUP = 1.0, 512, 100
chlorine, acid, _ = pi_loops(cols, N)
one = [wt.Trend("control", ("chlorine", "output"))]
eight = one + [wt.Trend("image_value", "chlorine_outlet"), wt.Trend("field_value", "chlorine_outlet"), wt.Trend("command", "chlorine"),
               wt.Trend("control", ("acid", "output")), wt.Trend("control", ("chlorine", "ise")), wt.Trend("alarm_word"),
               wt.Trend("image_fault", "pH_outlet")]
off = [wt.Trend("off")] * 8


def run(variant, rep=0):
    download = rep == REPEATS - 1 and variant in ("one", "eight")          # the series once, at the end
    ens = plant(cols, bc, n)
    ens.enable_control(chlorine, acid)
    if variant != "none":
        ens.set_trends(*{"off": off, "one": one, "eight": eight}[variant], capacity=CAPACITY)
    ens.step(DT, n_steps=WARMUP, download=False)
    if variant != "none":
        ens.reset_trends()
    _, t_step = timed_step(ens, DT, K)
    data, t_data = None, 0.0
    if download:
        t0 = time.perf_counter()
        data = ens.trend_data()
        t_data = time.perf_counter() - t0
    out = outputs(ens, "sensor_readings", "input_image", "boundary", "control_state")
    ens.close()
    return t_step, t_data, out, data


VARIANTS, REPEATS = ("none", "off", "one", "eight"), 9
run("none")                                      # module load, first launches
times, med, last = rotate(VARIANTS, REPEATS, run)
downloads, data = {v: last[v][1] for v in ("one", "eight")}, {v: last[v][3] for v in ("one", "eight")}
plant_equal = all(same(last["none"][2], last[v][2]) for v in VARIANTS[1:])
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
