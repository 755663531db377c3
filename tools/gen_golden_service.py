#!/usr/bin/env python3
"""Golden vectors for the sensor service program from the Python reference: tests/golden/g14_service_*.npz.

Build container only, like oracle/gen_golden_sensors.py: imports the reference's sensors and physics from
/root/reference/src, replaces each sensor's private numpy Generator by the counter-based stream of
oracle/sensor_oracle.py, runs the orchestrator's per-step sequence (``reactor.step`` -> ``read`` of every sensor) and,
between two iterations, calls the reference's own maintenance methods (``calibrate``, ``calibrate_two_point``,
``clean_electrode``, ``replace_membrane``, ``replace_reagent``) at the times a slot list dictates, with
``current_time`` the time of the read just taken.  The few lines of trigger logic below are the generator's own
(include/wtphys.h states them); SAMPLE and TRIM reference values come from the taps and ``sensor.calibration_offset``.

    python tools/gen_golden_service.py

Recorded: taps, values / status / fault per step, the slot list ([slots][WT_NSV], a case may hold more slots than one
reactor's program: sensors do not interact, a test deals them to several reactors), every service performed (step,
sensor, action, reference value) and each sensor's final calibration_offset, last_calibration_time, power_on_time and
slow fields.  Suite time starts at 0 (t0 = 0).
"""
from __future__ import annotations

import copy
import logging
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, "/root/reference/src"); sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "oracle"))
logging.disable(logging.CRITICAL)

from wt_simulator.core import BoundaryConditions, IntegratedCSTR, ReactorConfiguration  # noqa: E402
from wt_simulator.sensors import create_realistic_sensor_suite  # noqa: E402
from wt_simulator.sensors.base_sensor import SensorFault, SensorStatus  # noqa: E402
import sensor_oracle as SO  # noqa: E402

STATUS = {s: i for i, s in enumerate(SensorStatus)}
FAULT = {f: i for i, f in enumerate(SensorFault)}
SENSOR = {name: i for i, name in enumerate(SO.SENSOR_NAMES)}
CALIBRATE, TWO_POINT, RINSE, ACID_CLEAN, PEPSIN_CLEAN, REPLACE_MEMBRANE, REPLACE_REAGENT = range(7)
AT_TIME, ON_STATUS = 0, 1
CONSTANT, SAMPLE, TRIM = range(3)
CLEANING = {RINSE: "water_rinse", ACID_CLEAN: "acid_clean", PEPSIN_CLEAN: "pepsin_clean"}
TAP_SELF = (0, 1, 2, 3, 6, 4, 5)          # each sensor's own tap in (pH0, pHN, Cl0, ClN, T0, TN, flow)
SLOW = {"pH": ("membrane_fouling", "days_since_cleaning", "reference_contamination"),
        "chlorine_inlet": ("membrane_fouling", "membrane_age_days", None),
        "chlorine_outlet": ("reagent_potency", "light_exposure_hours", "reagent_age_days"),
        "flow_main": ("electrode_fouling", None, None), "temp": (None, None, None)}


def slot(sensor, action, at=None, every=0.0, count=0, on_status=None, delay=0.0, ref=0.0, ref2=0.0, ref_mode=CONSTANT):
    """One row in WT_SV_* order: enable, sensor, action, trigger, t_first, period, count, status, delay, ref_mode, ref, ref2."""
    timed = on_status is None
    return [1.0, SENSOR[sensor], action, AT_TIME if timed else ON_STATUS, at if timed else 0.0, every, count,
            0.0 if timed else STATUS[on_status], delay, ref_mode, ref, ref2]


def run(case, cfg_kw, bc_kw, steps, dt, reactor_id, seed, slots, expect):
    cfg = ReactorConfiguration(**cfg_kw)
    r = IntegratedCSTR(cfg)
    b = BoundaryConditions(**bc_kw)
    sensors = create_realistic_sensor_suite(cfg)
    assert tuple(sensors) == SO.SENSOR_NAMES
    objs = list(sensors.values())
    for i, (name, s) in enumerate(sensors.items()):
        s._rng = SO.SuiteRng(seed, reactor_id, i)
        ref = 7.0 if "pH" in name else cfg.initial_chlorine if "chlorine" in name else cfg.temperature if "temp" in name else cfg.flow_rate
        s.calibrate(ref, 0.0, "system_init")                                   # initialize_sensors (__main__.py:96-105)
    P = np.array(slots, dtype=np.float64)
    n_done = np.zeros(len(P)); t_due = P[:, 4].copy(); t_seen = np.full(len(P), np.nan)
    taps = np.empty((steps, 7)); vals = np.empty((steps, 7)); stat = np.empty((steps, 7), dtype=np.int8); flt = np.empty((steps, 7), dtype=np.int8)
    services = []
    for k in range(steps):
        st = copy.copy(r.step(dt, b))
        # the sensors look at the state rounded to float32, as the device's taps are: the recorded taps are exactly
        # what they saw, and a float32 in a float64 compresses to half (the files stay below the g7 ones)
        st.pH, st.chlorine, st.temperature = (np.asarray(a, dtype=np.float32).astype(np.float64) for a in (st.pH, st.chlorine, st.temperature))
        st.flow_rate = float(np.float32(st.flow_rate))
        t = (k + 1) * dt
        taps[k] = [st.pH[0], st.pH[-1], st.chlorine[0], st.chlorine[-1], st.temperature[0], st.temperature[-1], st.flow_rate]
        for i, s in enumerate(objs):
            rd = s.read(st, current_time=t)
            vals[k, i] = rd.value; stat[k, i] = STATUS[rd.status]; flt[k, i] = FAULT[rd.fault]
        # between two iterations: the slots, in order
        for j, p in enumerate(P):
            i, action = int(p[1]), int(p[2])
            if p[6] > 0 and n_done[j] >= p[6]:
                continue
            if int(p[3]) == AT_TIME:
                due = t >= t_due[j]
            else:
                if math.isnan(t_seen[j]) and stat[k, i] == int(p[7]):
                    t_seen[j] = t
                due = t - t_seen[j] >= p[8]
            if not due:
                continue
            s = objs[i]
            assert stat[k, i] not in (STATUS[SensorStatus.FAILED], STATUS[SensorStatus.POWER_FAULT]), \
                f"{case}: sensor {i} is dead at its service at step {k}: choose another seed"
            x = p[10]
            if int(p[9]) == SAMPLE:
                x = taps[k, TAP_SELF[i]] + p[10]
            elif int(p[9]) == TRIM:
                x = (taps[k, TAP_SELF[i]] + s.calibration_offset) + p[10]
            if action == CALIBRATE:
                s.calibrate(x, t, "service")
            elif action == TWO_POINT:
                x = (p[10] + p[11]) / 2.0
                s.calibrate_two_point(p[10], p[11], p[10], p[11], t, "service")
            elif action in CLEANING:
                s.clean_electrode(CLEANING[action], t)
            elif action == REPLACE_MEMBRANE:
                x = 0.0
                s.replace_membrane(t)
            else:
                x = 0.0
                s.replace_reagent(t)
            services.append((k, i, action, x))
            n_done[j] += 1
            if int(p[3]) == AT_TIME:
                if p[5] > 0:
                    t_due[j] = t_due[j] + (math.floor((t - t_due[j]) / p[5]) + 1.0) * p[5]
                    if not t_due[j] > t:
                        t_due[j] += p[5]
                else:
                    t_due[j] = math.inf
            else:
                t_seen[j] = math.nan
    final = np.zeros((7, 6))
    for i, (name, s) in enumerate(sensors.items()):
        final[i, :3] = s.calibration_offset, s.last_calibration_time, s.power_on_time
        key = "pH" if "pH" in name else "temp" if "temp" in name else name
        for q, attr in enumerate(SLOW[key]):
            final[i, 3 + q] = getattr(s, attr) if attr else 0.0
    assert n_done.astype(int).tolist() == expect, (case, n_done.tolist(), expect)
    path = os.path.join(ROOT, "tests", "golden", f"g14_service_{case}.npz")
    np.savez_compressed(path, taps=taps, values=vals, status=stat, fault=flt, dt=dt, seed=seed, reactor=reactor_id,
                        cfg_flow_rate=cfg.flow_rate, cfg_initial_chlorine=cfg.initial_chlorine, cfg_temperature=cfg.temperature,
                        n_zones=cfg.n_zones, slots=P, services=np.array(services, dtype=np.float64), final=final)
    dead = sorted({int(i) for i in np.argwhere((flt == FAULT[SensorFault.OPEN_CIRCUIT]) | (flt == FAULT[SensorFault.SHORT_CIRCUIT]))[:, 1]})
    print(f"{case}: {len(services)} services (per slot {n_done.astype(int).tolist()}), every serviced sensor alive at each of its "
          f"services; sensors with a random open/short-circuit fault in the run: {dead or 'none'}; "
          f"{os.path.getsize(path)} bytes", flush=True)


# Seeds for which no random open/short-circuit or power fault kills a serviced sensor before its services: run()
# asserts it at every service.  Found by trying 0x5E41CE0002, 3, ... in order (each rejected seed fails that assertion).
SEED_LONG5 = int(os.environ.get("WT_G14_SEED", "0x5E41CE0003"), 0)

if __name__ == "__main__":
    run("short8", dict(n_zones=8, flow_rate=8.0, initial_chlorine=2.0),
        dict(inlet_flow_rate=6.0, chlorine_flow_rate=0.2, inlet_temperature=22.0), 700, 1.0, reactor_id=3, seed=0x5E41CE0001,
        slots=[slot("flow_main", CALIBRATE, on_status=SensorStatus.DRIFT_WARNING, delay=20.0, ref_mode=TRIM),
               slot("chlorine_outlet", CALIBRATE, at=100.0, every=200.0, ref=1.5),
               slot("chlorine_inlet", REPLACE_MEMBRANE, at=150.0),
               slot("chlorine_inlet", CALIBRATE, at=460.0, ref_mode=TRIM),
               slot("temp_outlet", CALIBRATE, at=50.5, ref_mode=SAMPLE, ref=0.25)],
        expect=[1, 4, 1, 1, 1])
    run("long5", dict(n_zones=5, initial_pH=7.2), dict(inlet_flow_rate=5.0, inlet_pH=7.5, chlorine_flow_rate=0.3), 3120, 30.0,
        reactor_id=11, seed=SEED_LONG5,
        slots=[slot("pH_outlet", RINSE, at=6 * 3600.0, every=6 * 3600.0),
               slot("pH_outlet", ACID_CLEAN, at=12 * 3600.0),
               slot("pH_outlet", TWO_POINT, on_status=SensorStatus.CALIBRATION_EXPIRED, delay=600.0, ref=7.0, ref2=4.0),
               slot("pH_inlet", PEPSIN_CLEAN, at=8 * 3600.0),
               slot("chlorine_outlet", REPLACE_REAGENT, at=20 * 3600.0),
               slot("chlorine_outlet", CALIBRATE, at=20 * 3600.0, ref_mode=TRIM)],
        expect=[4, 1, 1, 1, 1, 1])
