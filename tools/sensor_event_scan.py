#!/usr/bin/env python3
"""Where the sensor suite's random stream draws its rare events (CPU only, the oracle alone).

For a suite seed and a range of global reactor indices: the first read at which each (sensor, fault) pair fires --
the 4-sigma supply draw that leaves a sensor in its sticky POWER_FAULT (power_low / power_high) and the 1e-4 per
read open / short circuit that kills it.  The taps are constants (every sensor sits at its calibration reference,
so no value-driven fault fires): which draw a read takes depends on the path the read takes (warming up: the
supply draw alone), not on the values, so a run on the device with the same seed, reactor index, step size and
clock meets the same events at the same reads -- unless its values drive a sensor through OUT_OF_RANGE or
RATE_FAULT, whose reads skip the circuit draw.

    python tools/sensor_event_scan.py --seed 0xC0FFEE --first 0 --count 400 --dt 30 --reads 150 [--t0 1800]

``--t0``: the clock at the first step's start, the suite calibrated at 0 (1800: every sensor warm at the first
read, what tests/test_gpu_sensor_edges.py does with ``set_state(..., time + 1800.0)``).  One line per event:
reactor, sensor, fault, read index (0-based).  ``events()`` is what the tests import.
"""
from __future__ import annotations

import argparse
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
import sensor_oracle as SO  # noqa: E402

FAULT_NAMES = {SO.FL_OPEN_CIRCUIT: "open_circuit", SO.FL_SHORT_CIRCUIT: "short_circuit", SO.FL_POWER_LOW: "power_low",
               SO.FL_POWER_HIGH: "power_high"}
FLOW, CHLORINE, TEMPERATURE = 5.0, 2.0, 20.0


def events(seed: int, reactors, dt: float, reads: int, t0: float = 0.0):
    """[(reactor, sensor index, fault name, read index)], the first read of every (sensor, fault) pair that fires within
    ``reads`` reads at t0 + dt, t0 + 2 dt, ...; sorted by reactor, then read, then sensor."""
    out = []
    for r in reactors:
        suite = SO.SensorSuite(FLOW, CHLORINE, TEMPERATURE, 0.0, seed, int(r))
        pH, Cl, T = {0: 7.0, -1: 7.0}, {0: CHLORINE, -1: CHLORINE}, {0: TEMPERATURE, -1: TEMPERATURE}
        seen = set()
        for k in range(reads):
            _, _, fault = suite.read_all(pH, Cl, T, FLOW, t0 + (k + 1) * dt)
            for i, f in enumerate(fault):
                if f in FAULT_NAMES and (i, f) not in seen:
                    seen.add((i, f))
                    out.append((int(r), i, FAULT_NAMES[f], k))
    return sorted(out, key=lambda e: (e[0], e[3], e[1]))


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--seed", type=lambda s: int(s, 0), default=0xC0FFEE)
    ap.add_argument("--first", type=int, default=0)
    ap.add_argument("--count", type=int, default=400)
    ap.add_argument("--dt", type=float, default=30.0)
    ap.add_argument("--reads", type=int, default=150)
    ap.add_argument("--t0", type=float, default=0.0)
    a = ap.parse_args()
    found = events(a.seed, range(a.first, a.first + a.count), a.dt, a.reads, a.t0)
    for r, i, name, k in found:
        print(f"{r:8d}  {SO.SENSOR_NAMES[i]:16s} {name:14s} read {k}")
    print(f"{len(found)} events in {a.count} reactors x {a.reads} reads")
