"""The sensor oracle with an installation (TEST INFRASTRUCTURE ONLY): oracle/sensor_oracle.py's ``SensorSuite`` with the
attributes and sample lines of a ``tests/golden/g16_install_*.npz`` case or of an ``Installation`` block, and the one
correction the g16 fixtures call for.

The disagreement.  ``BaseSensor._apply_installation_effects`` (sensors/base_sensor.py:464-507) returns early only when
the bubble draw *hits*; a value that is NaN already -- the lag keeps the NaN of an earlier bubble or open circuit --
goes on to the grounding and the vibration draw.  ``SensorSuite._base_read`` skips those two draws whenever the value
is NaN, so from the read after a sensor's first bubble on its draw counter falls behind the reference's by one or two
per read, and its later random-fault draws (and with them status and fault) are others.  No fixture before g16 took
these branches.  ``InstalledSuite`` restates ``_base_read`` with the reference's condition; g16_install_all_four is
the case that tells the two apart (tests/test_install_cpu.py).
"""
import math

import numpy as np

import sensor_oracle as SO

PARAM_ROWS = ("inlet_line_volume_mL", "inlet_line_flow_mL_min", "outlet_line_volume_mL", "outlet_line_flow_mL_min",
              "flow_velocity", "air_bubble_frequency", "grounding_quality", "pipe_vibration_g", "ambient_temperature")
DEFAULTS = (250.0, 500.0, 250.0, 500.0, 0.5, 0.0, 0.9, 0.1, 30.0)


class InstalledSuite(SO.SensorSuite):
    """``params``: the nine values of one reactor in WT_INS_* order."""

    def __init__(self, cfg_flow_rate, cfg_initial_chlorine, cfg_temperature, t0, seed, reactor, params=DEFAULTS):
        super().__init__(cfg_flow_rate, cfg_initial_chlorine, cfg_temperature, t0, seed, reactor)
        p = [float(x) for x in params]
        self.lines = (SO.SampleLine(p[0], p[1]), SO.SampleLine(p[2], p[3]))
        self.flow_velocity, self.air_bubble_frequency, self.grounding_quality, self.pipe_vibration_g, self.ambient_temperature = p[4:]

    def set_delays(self, inlet, outlet):
        """A mid-run change: the lines keep their buffers."""
        self.lines[0].transport_delay_s, self.lines[1].transport_delay_s = float(inlet), float(outlet)

    def _base_read(self, i, st, t):
        """sensor_oracle.SensorSuite._base_read with the installation effects as base_sensor.py:464-507 has them."""
        s, rng = self.sensors[i], self.rng[i]
        if not (20.0 < s["supply"] < 28.0):
            status = SO.ST_POWER_FAULT
            fault = SO.FL_POWER_LOW if s["supply"] < 20.0 else SO.FL_POWER_HIGH
            self._append(s, t, float("nan"))
            return float("nan"), status, fault
        s["supply"] = 24.0 + rng.normal(0.0, 1.0)
        if not (t - s["power_on"] >= s["warmup"]):
            self._append(s, t, float("nan"))
            return float("nan"), SO.ST_WARMING_UP, SO.FL_NONE
        cal_expired = not (s["have_cal"] and not ((t - s["cal_time"]) / 3600.0 > s["cal_valid_h"]))
        if cal_expired:
            s["status"] = SO.ST_CAL_EXPIRED
        true_value = self._true_value(s, st)
        if s["line"] is not None:
            temp = st[2][s["zone"]]
            true_value, _ = self.lines[s["line"]].transport_sample(true_value, temp, t)
        drift = s["drift_rate"] * ((t - s["cal_time"]) / 3600.0) + s["cal_offset"]
        noise = rng.normal(0.0, s["precision"])
        cur = 0.5 * (true_value + noise + drift) + 0.5 * s["current"]
        cur = self._installation_effects(cur, s, rng)
        s["current"] = cur
        rate = 0.0
        if s["hist_n"] > 0:
            dt = t - s["last_t"]
            if dt > 0 and math.isfinite(s["last_value"]):
                rate = (cur - s["last_value"]) / dt
        fault = None
        if not (20.0 < s["supply"] < 28.0):
            fault = SO.FL_POWER_LOW if s["supply"] < 20.0 else SO.FL_POWER_HIGH
        else:
            span = s["hi"] - s["lo"]
            if cur < s["lo"] - 0.1 * span or cur > s["hi"] + 0.1 * span:
                fault = SO.FL_OUT_OF_RANGE
            elif s["max_rate"] is not None and abs(rate) > s["max_rate"]:
                fault = SO.FL_RATE_FAULT
            elif rng.random() < 0.0001:
                fault = rng.choice([SO.FL_OPEN_CIRCUIT, SO.FL_SHORT_CIRCUIT])
        if fault is not None:
            s["fault"] = fault
            if fault in (SO.FL_OPEN_CIRCUIT, SO.FL_SHORT_CIRCUIT):
                s["status"] = SO.ST_FAILED
                s["current"] = cur = float("nan")
            elif fault == SO.FL_OUT_OF_RANGE:
                s["status"] = SO.ST_OUT_OF_RANGE
            elif fault in (SO.FL_POWER_LOW, SO.FL_POWER_HIGH):
                s["status"] = SO.ST_POWER_FAULT
            else:
                s["status"] = SO.ST_RATE_FAULT
        else:
            s["fault"] = SO.FL_NONE
            if not math.isnan(cur):
                bounded = min(max(cur, s["lo"]), s["hi"])
                if bounded != cur:
                    s["status"] = SO.ST_SATURATED
                elif not cal_expired:
                    s["status"] = SO.ST_NORMAL
                s["current"] = cur = bounded
            if abs(drift) > 0.1 * (s["hi"] - s["lo"]):
                if s["status"] != SO.ST_CAL_EXPIRED:
                    s["status"] = SO.ST_DRIFT_WARNING
        self._append(s, t, cur)
        return cur, s["status"], s["fault"]

    def _installation_effects(self, value, s, rng):
        if self.flow_velocity < 0.1:
            value += rng.normal(0.0, s["precision"] * 2.0)
        if self.air_bubble_frequency > 0:
            if rng.random() < self.air_bubble_frequency / 60.0:
                return float("nan")
        if self.grounding_quality < 0.8:
            value += rng.normal(0.0, s["precision"] * (2.0 - self.grounding_quality))
        if self.pipe_vibration_g > 0.2:
            value += rng.normal(0.0, self.pipe_vibration_g * s["precision"])
        return value


def run_case(g, suite_class=InstalledSuite):
    """A g16 case through ``suite_class``: (values, status, fault) (reads, 7), the suite."""
    suite = suite_class(float(g["cfg_flow_rate"]), float(g["cfg_initial_chlorine"]), float(g["cfg_temperature"]), 0.0,
                        int(g["seed"]), int(g["reactor"]), g["params"])
    taps, time, delays = g["taps"], g["time"], g["delays"]
    K = taps.shape[0]
    vals = np.empty((K, 7)); stat = np.empty((K, 7), dtype=np.int8); flt = np.empty((K, 7), dtype=np.int8)
    for k in range(K):
        if k > 0 and not np.array_equal(delays[k], delays[k - 1]):
            suite.set_delays(*delays[k])
        pH0, pHN, Cl0, ClN, T0, TN, flow = taps[k]
        vals[k], stat[k], flt[k] = suite.read_all({0: pH0, -1: pHN}, {0: Cl0, -1: ClN}, {0: T0, -1: TN}, flow, float(time[k]))
    return (vals, stat, flt), suite


def slow_fields(suite):
    """(7, 3): the slow fields of every sensor in the order of the fixtures' ``final`` (and of sensor_health()'s slow0..2)."""
    S = suite.sensors
    out = np.zeros((7, 3))
    for i in (SO.S_PH_IN, SO.S_PH_OUT):
        out[i] = S[i]["fouling"], S[i]["days_clean"], S[i]["ref_contam"]
    out[SO.S_CL_IN, :2] = S[SO.S_CL_IN]["fouling"], S[SO.S_CL_IN]["membrane_age"]
    out[SO.S_CL_OUT] = S[SO.S_CL_OUT]["potency"], S[SO.S_CL_OUT]["light_h"], S[SO.S_CL_OUT]["reagent_age"]
    out[SO.S_FLOW, 0] = S[SO.S_FLOW]["electrode_fouling"]
    return out
