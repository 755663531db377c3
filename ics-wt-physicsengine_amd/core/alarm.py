"""Per-reactor alarm and interlock programs that run on the device at every PLC scan (include/wtphys.h,
``wt_ensemble_alarm_*``): the safety side of the control layer.

A program has up to four slots.  A slot watches one sensor reading -- the scan's image copy, after any injection
program, or the instrument's own field reading -- against a HIGH or LOW limit with deadband, on-delay and latch.  An
active slot may trip the acid or chlorine dosing command to a fixed value from the next scan on.  This module builds
and checks the parameter block and unpacks the state; the evaluation itself runs in ``csrc/wt_alm.hpp``.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional, Union

import numpy as np

from . import _native
from ._program import SENSOR_NAMES, codes, field_rows, slot_block

SLOTS, NA, NAS, NAR = 4, 10, 8, 6        # WT_ALM_SLOTS, WT_NA, WT_NAS, WT_NAR
PARAM_ROWS = ("kind", "sensor", "source", "setpoint", "deadband", "on_delay", "latch", "on_bad", "action", "trip_value")
STATE_ROWS = ("active", "cond", "pending", "n_act", "t_first", "t_last", "time_active", "n_bad")
REACTOR_ROWS = ("t_prev", "first_out", "ovr_acid", "ovr_chlorine", "n_ovr_acid", "n_ovr_chlorine")
KINDS = ("off", "high", "low")
SOURCES = ("image", "field")
ON_BAD = ("hold", "alarm")
ACTIONS = ("none", "trip_acid", "trip_chlorine")
# alarm word bits (wt_ensemble_alarm_words)
WORD_ACID, WORD_CHLORINE, WORD_FIRST_OUT_SHIFT = 1 << 8, 1 << 9, 12

Value = Union[float, int, str, np.ndarray]


@dataclass
class Alarm:
    """One slot.  ``sensor``: a name of :data:`SENSOR_NAMES` or its index; ``kind``: "high" or "low" (or "off");
    ``source``: "image" (the scan's copy after any injection program) or "field" (the instrument's own reading);
    ``on_bad``: "hold" (a NaN or faulted reading changes nothing but the count) or "alarm" (it counts as the
    condition); ``action``: None, "trip_acid" or "trip_chlorine", with ``trip_value`` the command the trip forces.
    A HIGH slot's condition is v > setpoint and clears at v < setpoint - deadband (LOW mirrored); it activates after
    the condition held for ``on_delay`` seconds; a latched slot stays active until :meth:`reset_alarms`.  Every field
    takes a scalar or an (N,) array."""

    sensor: Value
    kind: Value
    setpoint: Value
    deadband: Value = 0.0
    on_delay: Value = 0.0
    latch: Value = False
    source: Value = "image"
    on_bad: Value = "hold"
    action: Optional[Value] = None
    trip_value: Value = 0.0


@dataclass
class AlarmState:
    """``ReactorEnsemble.alarm_state()``: slot fields (SLOTS, N), reactor fields (N,), float64."""

    active: np.ndarray
    cond: np.ndarray
    pending: np.ndarray        # loop time the condition started to stand while inactive (NaN: none)
    n_act: np.ndarray          # activations
    t_first: np.ndarray        # loop time of the first activation (NaN: never)
    t_last: np.ndarray         # last scan at which the slot was active
    time_active: np.ndarray    # seconds active
    n_bad: np.ndarray          # scans with a NaN or faulted reading
    t_prev: np.ndarray
    first_out: np.ndarray      # slot that activated first since the last clean state (-1: none)
    ovr_acid: np.ndarray       # trip value in force for the next scan (NaN: none)
    ovr_chlorine: np.ndarray
    n_ovr_acid: np.ndarray     # scans whose command was overridden
    n_ovr_chlorine: np.ndarray

    @classmethod
    def from_block(cls, slot_block: np.ndarray, reactor_block: np.ndarray) -> "AlarmState":
        """From a [WT_ALM_SLOTS][WT_NAS][N] and a [WT_NAR][N] block."""
        return cls(*(np.array(slot_block[:, k]) for k in range(NAS)), *(np.array(reactor_block[k]) for k in range(NAR)))

    def block(self):
        """The (SLOTS, NAS, N) and (NAR, N) blocks again."""
        return (np.stack([getattr(self, k) for k in STATE_ROWS], axis=1),
                np.stack([getattr(self, k) for k in REACTOR_ROWS]))


def slot_rows(alarm: Alarm, n: int, name: str = "alarm") -> np.ndarray:
    """(NA, N) rows of one slot."""
    if not isinstance(alarm, Alarm):
        raise TypeError(f"{name}: expected an Alarm, got {type(alarm).__name__}")
    return field_rows(alarm, PARAM_ROWS, n, name, kind=codes(alarm.kind, KINDS, "kind"),
                      sensor=codes(alarm.sensor, SENSOR_NAMES, "sensor"), source=codes(alarm.source, SOURCES, "source"),
                      on_bad=codes(alarm.on_bad, ON_BAD, "on_bad"),
                      action=codes("none" if alarm.action is None else alarm.action, ACTIONS, "action"))


def alarm_block(n_reactors: int, *alarms: Alarm) -> np.ndarray:
    """The [WT_ALM_SLOTS][WT_NA][N] float64 block of ``wt_ensemble_alarm_set``, checked by the library: slot k is the
    k-th alarm, the slots after the last are off."""
    n = int(n_reactors)
    return slot_block(alarms, n, SLOTS, "alarm", slot_rows, np.zeros((NA, n)), _native.WT_PROG_ALARM)
