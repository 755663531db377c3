"""Host restatement of the sensor service program (include/wtphys.h, ``wt_ensemble_service_*``), test infrastructure.

Two halves.  The maintenance methods of the reference's sensors -- ``BaseSensor.calibrate`` (base_sensor.py:701-755),
``pHSensor.calibrate_two_point`` / ``clean_electrode`` (ph_sensor.py:338-434), ``ChlorineSensor.replace_membrane`` /
``replace_reagent`` (chlorine_sensor.py:486-537) -- restated on the sensor dictionaries of ``oracle/sensor_oracle.py``'s
``SensorSuite``, in fp64 as the reference computes them.  And the slot logic of the program: which slots fall due after
a read, and the new slot state (``ServiceProgram``), in the header's fp64 arithmetic.
"""
from __future__ import annotations

import math

import numpy as np

import sensor_oracle as SO

SLOTS, NSV, NSVS = 4, 12, 4
(V_ENABLE, V_SENSOR, V_ACTION, V_TRIGGER, V_T_FIRST, V_PERIOD, V_COUNT, V_STATUS, V_DELAY, V_REF_MODE, V_REF, V_REF2) = range(NSV)
VS_N_DONE, VS_T_LAST, VS_T_DUE, VS_T_SEEN = range(NSVS)
CALIBRATE, TWO_POINT, RINSE, ACID_CLEAN, PEPSIN_CLEAN, REPLACE_MEMBRANE, REPLACE_REAGENT = range(7)
AT_TIME, ON_STATUS = 0, 1
REF_CONSTANT, REF_SAMPLE, REF_TRIM = range(3)
CLEANING = {RINSE: ("water_rinse", 0.5), ACID_CLEAN: ("acid_clean", 0.1), PEPSIN_CLEAN: ("pepsin_clean", 0.2)}
# index of each sensor's own tap in (pH0, pHN, Cl0, ClN, T0, TN, flow)
TAP_SELF = (0, 1, 2, 3, 6, 4, 5)
# the oracle's names of the device's slow0 / slow1 / slow2 rows, by sensor kind
SLOW = {SO.K_PH: ("fouling", "days_clean", "ref_contam"), SO.K_CL_AMP: ("fouling", "membrane_age", None),
        SO.K_CL_DPD: ("potency", "light_h", "reagent_age"), SO.K_FLOW_MAG: ("electrode_fouling", None, None),
        SO.K_T_RTD: (None, None, None)}


# ---------------------------------------------------------------- the reference's maintenance methods
def calibrate(s: dict, reference_value: float, t: float) -> None:
    s["cal_offset"] = reference_value - s["current"]
    s["cal_time"] = t
    s["status"], s["fault"] = SO.ST_NORMAL, SO.FL_NONE
    s["power_on"] = t
    s["have_cal"] = True


def calibrate_two_point(s: dict, buffer_1: float, buffer_2: float, t: float) -> None:
    if s["kind"] != SO.K_PH:
        raise ValueError("only pH sensors have a two-point calibration")
    s["cal_p1"], s["cal_p2"] = buffer_1, buffer_2          # ph_sensor.py:386-387 (read by ServicedSuite alone)
    s["ref_contam"] = 0.0
    calibrate(s, (buffer_1 + buffer_2) / 2.0, t)


def clean_electrode(s: dict, action: int, t: float) -> None:
    if s["kind"] != SO.K_PH:
        raise ValueError("only pH electrodes are cleaned")
    s["fouling"] *= CLEANING[action][1]
    s["days_clean"] = 0.0
    s["power_on"] = t


def replace_membrane(s: dict, t: float) -> None:
    if s["kind"] != SO.K_CL_AMP:
        raise ValueError("Only amperometric sensors have membranes")
    s["fouling"] = 0.0
    s["membrane_age"] = 0.0
    s["power_on"] = t
    calibrate(s, 0.0, t)


def replace_reagent(s: dict, t: float) -> None:
    if s["kind"] != SO.K_CL_DPD:
        raise ValueError("Only DPD sensors have reagent")
    s["potency"] = 1.0
    s["reagent_age"] = 0.0
    s["light_h"] = 0.0
    calibrate(s, 0.0, t)


def reference_value(s: dict, action: int, ref_mode: int, ref: float, ref2: float, tap: float) -> float:
    """The calibration's reference value (fp64; the device rounds it once to float32)."""
    if action == TWO_POINT:
        return (ref + ref2) / 2.0
    if action in (REPLACE_MEMBRANE, REPLACE_REAGENT):
        return 0.0
    if ref_mode == REF_SAMPLE:
        return tap + ref
    if ref_mode == REF_TRIM:
        return (tap + s["cal_offset"]) + ref
    return ref


def apply(suite: "SO.SensorSuite", sensor: int, action: int, t: float, ref_mode: int = REF_CONSTANT, ref: float = 0.0,
          ref2: float = 0.0, taps=None) -> float:
    """One action on one sensor of ``suite`` at suite time ``t``; ``taps``: the seven true values the sensors see (only
    SAMPLE and TRIM read the sensor's own).  Returns the reference value used."""
    s = suite.sensors[sensor]
    tap = float("nan") if taps is None else float(taps[TAP_SELF[sensor]])
    x = reference_value(s, action, ref_mode, ref, ref2, tap)
    if action == CALIBRATE:
        calibrate(s, x, t)
    elif action == TWO_POINT:
        calibrate_two_point(s, ref, ref2, t)
    elif action in CLEANING:
        clean_electrode(s, action, t)
    elif action == REPLACE_MEMBRANE:
        replace_membrane(s, t)
    elif action == REPLACE_REAGENT:
        replace_reagent(s, t)
    else:
        raise ValueError(f"unknown action {action}")
    return x


def health(suite: "SO.SensorSuite") -> np.ndarray:
    """(7, 8): cal_offset, cal_time, power_on, slow0, slow1, slow2, status, fault of every sensor, as
    ``sensor_health()`` orders them (a slow row the sensor's kind does not have: 0, the DPD potency row aside)."""
    out = np.zeros((7, 8))
    for i, s in enumerate(suite.sensors):
        out[i, :3] = s["cal_offset"], s["cal_time"], s["power_on"]
        for k, name in enumerate(SLOW[s["kind"]]):
            out[i, 3 + k] = s[name] if name else 0.0
        out[i, 6:] = s["status"], s["fault"]
    return out


class ServicedSuite(SO.SensorSuite):
    """The oracle suite with the one reference field a two-point calibration changes that the oracle holds constant:
    ``calibration_point_1 / _2`` (ph_sensor.py:135-136, :282-290, :386-387).  The slope error of a pH reading is zero
    strictly between the two points and the distance to the nearer point times the slope loss elsewhere; the oracle
    (and the device) keep the suite's points 4 and 7.  Buffers given as (7, 4) leave no value between
    them, so the reference then adds ``min(|v - 7|, |v - 4|) * 1e-5 * days since calibration`` everywhere.  This class
    puts that term where the oracle's pH read has the fixed-point one; everything else is the oracle's."""

    def _read(self, i, st, t):
        s = self.sensors[i]
        if s["kind"] != SO.K_PH or (s.get("cal_p1", 4.0), s.get("cal_p2", 7.0)) == (4.0, 7.0):
            return super()._read(i, st, t)
        p1, p2 = s["cal_p1"], s["cal_p2"]
        fixed = {}
        base = self._base_read

        def spy(j, st_, t_):            # the lagged value the slope error is computed from
            out = base(j, st_, t_)
            fixed["v"] = out[0]
            return out

        self._base_read = spy
        try:
            final, status, fault = super()._read(i, st, t)
        finally:
            del self._base_read
        v = fixed["v"]
        if not math.isfinite(v):
            return final, status, fault
        theirs = 0.0 if 4.0 < v < 7.0 else min(abs(v - 4.0), abs(v - 7.0)) * (100.0 - s["slope_pct"]) / 100.0
        ours = 0.0 if p1 < v < p2 else min(abs(v - p1), abs(v - p2)) * (100.0 - s["slope_pct"]) / 100.0
        final = min(max(final - theirs + ours, s["lo"]), s["hi"])
        s["current"] = final
        s["last_value"] = final
        return final, status, fault


# ---------------------------------------------------------------- the slot logic
class ServiceProgram:
    """The slots of N reactors: ``params`` [slots][NSV][N] as ``service_block`` builds it (the device has SLOTS slots;
    the restatement takes any number); ``state`` [slots][NSVS][N] starts at the set-time values."""

    def __init__(self, params: np.ndarray):
        self.params = np.array(params, dtype=np.float64)
        assert self.params.ndim == 3 and self.params.shape[1] == NSV
        self.slots, self.n = self.params.shape[0], self.params.shape[-1]
        self.reset()

    def reset(self) -> None:
        self.state = np.empty((self.slots, NSVS, self.n))
        self.state[:, VS_N_DONE] = 0.0
        self.state[:, VS_T_LAST] = np.nan
        self.state[:, VS_T_DUE] = self.params[:, V_T_FIRST]
        self.state[:, VS_T_SEEN] = np.nan

    def after_read(self, r: int, t: float, status) -> list:
        """The read of reactor ``r`` at suite time ``t`` returned ``status`` (seven codes): the slots that fall due, in
        slot order, as (slot, sensor, action, ref_mode, ref, ref2); the slot state is updated."""
        due = []
        for k in range(self.slots):
            p, q = self.params[k, :, r], self.state[k, :, r]
            if p[V_ENABLE] != 1.0:
                continue
            if p[V_COUNT] > 0.0 and q[VS_N_DONE] >= p[V_COUNT]:
                continue
            i = int(p[V_SENSOR])
            if int(p[V_TRIGGER]) == AT_TIME:
                is_due = t >= q[VS_T_DUE]
            else:
                if math.isnan(q[VS_T_SEEN]) and int(status[i]) == int(p[V_STATUS]):
                    q[VS_T_SEEN] = t
                is_due = t - q[VS_T_SEEN] >= p[V_DELAY]          # NaN: False
            if not is_due:
                continue
            due.append((k, i, int(p[V_ACTION]), int(p[V_REF_MODE]), float(p[V_REF]), float(p[V_REF2])))
            q[VS_N_DONE] += 1.0
            q[VS_T_LAST] = t
            if int(p[V_TRIGGER]) == AT_TIME:
                if p[V_PERIOD] > 0.0:
                    nd = q[VS_T_DUE] + (math.floor((t - q[VS_T_DUE]) / p[V_PERIOD]) + 1.0) * p[V_PERIOD]
                    if not nd > t:
                        nd = nd + p[V_PERIOD]
                    q[VS_T_DUE] = nd
                else:
                    q[VS_T_DUE] = math.inf
            else:
                q[VS_T_SEEN] = math.nan
        return due
