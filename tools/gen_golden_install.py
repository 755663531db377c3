#!/usr/bin/env python3
"""Golden vectors for the installation of the sensor suite from the Python reference: tests/golden/g16_install_*.npz.

Build container only, like tools/gen_golden_service.py: imports the reference's sensors and physics from
/root/reference/src, replaces each sensor's private numpy Generator by the counter-based stream of
oracle/sensor_oracle.py, then gives the suite another installation than the one ``create_realistic_sensor_suite``
builds: it mutates the ``InstallationQuality`` object all seven sensors share and replaces the two ``SampleLine``
objects (each shared by a pH electrode and the RTD next to it) by new ones of another volume and flow.  A case with a
mid-run change assigns ``transport_delay_s`` of the lines between two reads and keeps their buffers.  Then the
orchestrator's per-step sequence: ``reactor.step`` -> ``read`` of every sensor.

    python tools/gen_golden_install.py

The suite is calibrated at t = 0 and the first read is taken at 1800 s + dt, so that every sensor is warm (the pH
electrodes warm up for 1800 s) and both sensors of a line push from the first read on.  Recorded per case: the taps
(rounded to float32, what the device's sensors see), the time, values, status and fault of every read, the nine
installation parameters in WT_INS_* order, the two lines' delay at every read, and each sensor's final slow fields.
Bubble frequencies are 3.75 and 0.46875 per minute: frequency / 60 is 1/16 and 1/128, so a 24-bit uniform compares
with it alike in fp32 and in fp64.
"""
from __future__ import annotations

import copy
import logging
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, "/root/reference/src"); sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "oracle"))
logging.disable(logging.CRITICAL)

from wt_simulator.core import BoundaryConditions, IntegratedCSTR, ReactorConfiguration  # noqa: E402
from wt_simulator.sensors import create_realistic_sensor_suite  # noqa: E402
from wt_simulator.sensors.base_sensor import SampleLine, SensorFault, SensorStatus  # noqa: E402
import sensor_oracle as SO  # noqa: E402

STATUS = {s: i for i, s in enumerate(SensorStatus)}
FAULT = {f: i for i, f in enumerate(SensorFault)}
WARM = 1800.0
SEED = 0x1257A11
SLOW = {"pH": ("membrane_fouling", "days_since_cleaning", "reference_contamination"),
        "chlorine_inlet": ("membrane_fouling", "membrane_age_days", None),
        "chlorine_outlet": ("reagent_potency", "light_exposure_hours", "reagent_age_days"),
        "flow_main": ("electrode_fouling", None, None), "temp": (None, None, None)}
# WT_INS_* order; the suite's own build
DEFAULTS = dict(inlet_line_volume_mL=250.0, inlet_line_flow_mL_min=500.0, outlet_line_volume_mL=250.0, outlet_line_flow_mL_min=500.0,
                flow_velocity=0.5, air_bubble_frequency=0.0, grounding_quality=0.9, pipe_vibration_g=0.1, ambient_temperature=30.0)
# a plant whose line signals move: acid and chlorine dosing, a warm inlet
CFG = dict(n_zones=5, flow_rate=8.0, initial_chlorine=1.0, initial_pH=7.6)
BC = dict(inlet_flow_rate=6.0, inlet_pH=7.8, acid_flow_rate=0.4, acid_concentration=0.1, chlorine_flow_rate=0.3, inlet_temperature=27.0)


def run(case, steps, dt, reactor_id, changes=(), **inst):
    """``inst``: fields of DEFAULTS to replace.  ``changes``: (read index, inlet delay, outlet delay) -- before that
    read the lines' ``transport_delay_s`` are set to these values (the buffers stay)."""
    par = dict(DEFAULTS, **inst)
    assert set(par) == set(DEFAULTS)
    cfg = ReactorConfiguration(**CFG)
    r = IntegratedCSTR(cfg)
    b = BoundaryConditions(**BC)
    sensors = create_realistic_sensor_suite(cfg)
    assert tuple(sensors) == SO.SENSOR_NAMES
    objs = list(sensors.values())
    quality = objs[0].installation
    assert all(s.installation is quality for s in objs)
    for k in ("flow_velocity", "air_bubble_frequency", "grounding_quality", "pipe_vibration_g", "ambient_temperature"):
        setattr(quality, k, par[k])
    quality.validate()
    lines = (SampleLine(volume_mL=par["inlet_line_volume_mL"], flow_rate_mL_min=par["inlet_line_flow_mL_min"], ambient_temp=25.0),
             SampleLine(volume_mL=par["outlet_line_volume_mL"], flow_rate_mL_min=par["outlet_line_flow_mL_min"], ambient_temp=25.0))
    assert all(l.delay_buffer.maxlen == 100 for l in lines), "a delay of 91 s or more: the reference's buffer grows"
    for name, s in sensors.items():
        if s.sample_line is not None:
            s.sample_line = lines[0 if name.endswith("inlet") else 1]
    for i, (name, s) in enumerate(sensors.items()):
        s._rng = SO.SuiteRng(SEED, reactor_id, i)
        ref = 7.0 if "pH" in name else cfg.initial_chlorine if "chlorine" in name else cfg.temperature if "temp" in name else cfg.flow_rate
        s.calibrate(ref, 0.0, "system_init")                                   # initialize_sensors (__main__.py:96-105)
    taps = np.empty((steps, 7)); vals = np.empty((steps, 7)); stat = np.empty((steps, 7), dtype=np.int8); flt = np.empty((steps, 7), dtype=np.int8)
    time = np.empty(steps); delays = np.empty((steps, 2))
    changes = {k: (a, c) for k, a, c in changes}
    for k in range(steps):
        st = copy.copy(r.step(dt, b))
        st.pH, st.chlorine, st.temperature = (np.asarray(a, dtype=np.float32).astype(np.float64) for a in (st.pH, st.chlorine, st.temperature))
        st.flow_rate = float(np.float32(st.flow_rate))
        if k in changes:
            lines[0].transport_delay_s, lines[1].transport_delay_s = changes[k]
        t = WARM + (k + 1) * dt
        time[k] = t
        delays[k] = lines[0].transport_delay_s, lines[1].transport_delay_s
        taps[k] = [st.pH[0], st.pH[-1], st.chlorine[0], st.chlorine[-1], st.temperature[0], st.temperature[-1], st.flow_rate]
        for i, s in enumerate(objs):
            rd = s.read(st, current_time=t)
            vals[k, i] = rd.value; stat[k, i] = STATUS[rd.status]; flt[k, i] = FAULT[rd.fault]
    final = np.zeros((7, 3))
    for i, (name, s) in enumerate(sensors.items()):
        key = "pH" if "pH" in name else "temp" if "temp" in name else name
        for q, attr in enumerate(SLOW[key]):
            final[i, q] = getattr(s, attr) if attr else 0.0
    path = os.path.join(ROOT, "tests", "golden", f"g16_install_{case}.npz")
    np.savez_compressed(path, taps=taps, time=time, values=vals, status=stat, fault=flt, dt=dt, seed=SEED, reactor=reactor_id,
                        cfg_flow_rate=cfg.flow_rate, cfg_initial_chlorine=cfg.initial_chlorine, cfg_temperature=cfg.temperature,
                        n_zones=cfg.n_zones, params=np.array([par[k] for k in DEFAULTS]), delays=delays, final=final,
                        draws=np.array([s._rng.draws for s in objs]))
    nan_from = [int(np.argmax(np.isnan(vals[:, i]))) if np.isnan(vals[:, i]).any() else -1 for i in range(7)]
    print(f"{case}: {steps} reads of {dt} s, delays {delays[0].tolist()} -> {delays[-1].tolist()}, first NaN per sensor {nan_from}, "
          f"flow dropouts {int((vals[:, 4] == 0.0).sum())}, statuses {sorted(set(stat.ravel().tolist()))}, {os.path.getsize(path)} bytes", flush=True)


if __name__ == "__main__":
    # each installation branch alone, at its threshold value (the branch is not taken) and just beyond it
    run("stagnant_at", 40, 1.0, 2, flow_velocity=0.1)
    run("stagnant_beyond", 40, 1.0, 2, flow_velocity=0.09)
    run("ground_at", 40, 1.0, 3, grounding_quality=0.8)
    run("ground_beyond", 40, 1.0, 3, grounding_quality=0.79)
    run("vibration_at", 40, 1.0, 4, pipe_vibration_g=0.2)
    run("vibration_beyond", 40, 1.0, 4, pipe_vibration_g=0.21)
    # bubbles: 1/16 and 1/128 per read
    run("bubbles_fast", 60, 1.0, 5, air_bubble_frequency=3.75)
    run("bubbles_slow", 300, 1.0, 6, air_bubble_frequency=0.46875)
    run("all_four", 60, 1.0, 7, flow_velocity=0.05, air_bubble_frequency=0.46875, grounding_quality=0.3, pipe_vibration_g=0.6,
        ambient_temperature=45.0)
    # the stagnant ageing rates over a day of hourly reads, and another ambient temperature
    run("stagnant_day", 24, 3600.0, 8, flow_velocity=0.0, ambient_temperature=12.5)
    # line delays: 0 (flow 0) and 9.96 s (83 mL); 12 s and 50 s; 90 s and 12 s
    run("delay_0_10", 60, 1.0, 9, inlet_line_flow_mL_min=0.0, outlet_line_volume_mL=83.0)
    run("delay_12_50", 80, 0.8, 10, inlet_line_volume_mL=100.0, outlet_line_flow_mL_min=300.0)
    run("delay_90_12", 120, 1.0, 11, inlet_line_volume_mL=750.0, outlet_line_volume_mL=100.0)
    # 90 s at dt = 0.5 s: the 100 entries (two pushes per read) span 25 s, the winner is the oldest entry held
    run("delay_90_short_ring", 120, 0.5, 12, inlet_line_volume_mL=750.0, outlet_line_volume_mL=750.0)
    # a mid-run change, up and down: 12 s -> 50 s -> 0 s on the inlet line, 12 s -> 0 s -> 50 s on the outlet line
    run("delay_change", 150, 1.0, 13, inlet_line_volume_mL=100.0, outlet_line_volume_mL=100.0,
        changes=((60, 50.0, 0.0), (110, 0.0, 50.0)))
