#!/usr/bin/env python3
"""What an installation of the sensor suite costs: `python tools/install_probe.py [N] [n] [steps]` (12 500 x 8 over 500
steps of 1 s after 100 warm-up steps by default, the shape of `bench.py --sensors`), one fused call each:
  (a) the sensor suite without an installation,
  (b) an installation of the suite's own defaults on every reactor (the flag on, no branch taken),
  (c) every reactor with its own delays and ambient temperature (no extra draw),
  (d) all four installation effects on every reactor: stagnant flow, bubbles at 1/128 per read, poor grounding, vibration
      (up to four more Philox calls per sensor and read; the sensors die off as the bubbles hit),
  (e) (d) without the bubbles: three more draws per sensor and read for the whole run.
Five repeats in rotating order, medians and ranges, with the bitwise check of (a) against (b); one JSON line."""
import json

import numpy as np

from probe_common import arguments, ensemble, outputs, rotate, same, timed_step, wt

N, n, K, cols, bc = arguments(500)
if len(__import__("sys").argv) < 2:
    N = 12500
    cols, bc = wt.make_ensemble(N)
WARMUP = 100
r = np.arange(N)
volume = np.array([750.0, 250.0, 100.0, 250.0, 83.0])
flow = np.array([500.0, 0.0, 500.0, 300.0, 500.0])
delays = dict(inlet_line_volume_mL=volume[r % 5], inlet_line_flow_mL_min=flow[r % 5], outlet_line_volume_mL=volume[(r + 1) % 5],
              outlet_line_flow_mL_min=flow[(r + 1) % 5], ambient_temperature=10.0 + (r % 30))
effects = dict(flow_velocity=0.05, grounding_quality=0.4, pipe_vibration_g=0.5)
VARIANTS = {"a_none": None, "b_defaults": wt.Installation(), "c_delays": wt.Installation(**delays),
            "d_all_four": wt.Installation(air_bubble_frequency=0.46875, **delays, **effects),
            "e_three_noises": wt.Installation(**delays, **effects)}


def run(variant, rep):
    ens = ensemble(cols, bc, n)
    ens.enable_sensors(seed=1)
    if VARIANTS[variant] is not None:
        ens.set_installation(VARIANTS[variant])
    ens.step(1.0, n_steps=WARMUP, download=False)
    _, sec = timed_step(ens, 1.0, K)
    out = outputs(ens, "sensor_readings")
    alive = float(np.isfinite(out[-3]).mean())
    ens.close()
    return sec, out, alive


times, median, last = rotate(list(VARIANTS), 5, run)
print(json.dumps({"probe": "install", "reactors": N, "zones": n, "steps": K, "warmup": WARMUP,
                  "seconds_median": median, "seconds_all": times,
                  "reactor_zone_steps_per_s": {v: N * n * K / s for v, s in median.items()},
                  "relative_to_none": {v: s / median["a_none"] for v, s in median.items()},
                  "finite_readings_at_end": {v: last[v][2] for v in VARIANTS},
                  "defaults_equal_none_bitwise": same(last["a_none"][1], last["b_defaults"][1])}))
