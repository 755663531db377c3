"""Per-reactor trend recorder programs that run on the device at every PLC scan (include/wtphys.h,
``wt_ensemble_trend_*``): the plant's historian.

A program has up to eight slots.  A slot takes one value of every scan -- a reading as the controller's image or the
instrument itself has it, a fault code, a command as it reaches the plant, or one entry of another program's state --
keeps every ``every``-th one that left a deadband inside a time window, and appends (time, value) to a store of
``capacity`` samples.  The values are copies, so a series is bit for bit what a host loop of one call per scan reads from
the getters.  This module builds the parameter block and unpacks state and data; the recording itself runs in
``csrc/wt_trd.hpp``.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Tuple, Union

import numpy as np

from . import _native, actuator, alarm, control, detect, inject
from ._program import SENSOR_NAMES, codes, field_rows, slot_block

SLOTS, NT, NTS = 8, 6, 4                 # WT_TRD_SLOTS, WT_NT, WT_NTS
PARAM_ROWS = ("tag", "index", "every", "deadband", "t_start", "t_end")
STATE_ROWS = ("n_seen", "n_recorded", "n_dropped", "last")
TAGS = ("off", "image_value", "image_fault", "field_value", "field_fault", "command", "control", "inject", "alarm",
        "alarm_word", "actuator", "detect")
# tags whose index names an entry of another program's state block: (names of its loops / channels or None, state rows)
_STATE_OF = {"control": (control.LOOPS, control.STATE_ROWS), "inject": (None, inject.STATE_ROWS),
             "alarm": (None, alarm.STATE_ROWS), "actuator": (actuator.CHANNELS, actuator.STATE_ROWS),
             "detect": (None, detect.STATE_ROWS)}

Value = Union[float, int, str, np.ndarray]


@dataclass
class Trend:
    """One slot.  ``tag``: a name of :data:`TAGS` or its code; ``index``: which entry of the tag -- a sensor (name of
    :data:`SENSOR_NAMES` or index) for "image_value", "image_fault", "field_value" and "field_fault"; a channel
    ("acid", "chlorine", "inlet" or 0..2) for "command"; for "control", "inject", "alarm", "actuator" and "detect" a pair
    (loop, slot or channel; name of a state row), as in ``("chlorine", "output")`` or ``(0, "stat")``, or the flat
    number ``unit * rows + row``; 0 for "alarm_word".  ``every``: a candidate every that many scans the slot sees;
    ``deadband``: negative records every candidate, otherwise only a value more than ``deadband`` away from the last
    recorded one; the slot sees the scans with ``t_start <= t < t_end``.  Every field takes a scalar or an (N,) array."""

    tag: Value
    index: Union[Value, Tuple] = 0
    every: Value = 1
    deadband: Value = -1.0
    t_start: Value = -np.inf
    t_end: Value = np.inf


@dataclass
class TrendState:
    """``ReactorEnsemble.trend_state()``: slot fields (SLOTS, N), float64."""

    n_seen: np.ndarray         # scans inside the slot's window
    n_recorded: np.ndarray     # samples stored or overwritten
    n_dropped: np.ndarray      # samples that found the store full (wrap off)
    last: np.ndarray           # the last value taken (NaN: none yet)

    @classmethod
    def from_block(cls, slot_block: np.ndarray) -> "TrendState":
        """From a [WT_TRD_SLOTS][WT_NTS][N] block."""
        return cls(*(np.array(slot_block[:, k]) for k in range(NTS)))

    def block(self) -> np.ndarray:
        """The (SLOTS, NTS, N) block again."""
        return np.stack([getattr(self, k) for k in STATE_ROWS], axis=1)


@dataclass
class TrendData:
    """``ReactorEnsemble.trend_data()``: ``time`` and ``value`` (SLOTS, capacity, N), oldest sample first, NaN past the
    ``count`` (SLOTS, N) samples held."""

    time: np.ndarray
    value: np.ndarray
    count: np.ndarray

    def series(self, slot: int, reactor: int):
        """(t, x) of one slot of one reactor, trimmed to the samples held."""
        k = int(self.count[slot, reactor])
        return self.time[slot, :k, reactor].copy(), self.value[slot, :k, reactor].copy()


def _unit_names(tag: str):
    return SENSOR_NAMES if tag in TAGS[1:5] else actuator.CHANNELS if tag == "command" else None


def _index_row(trend: Trend, name: str):
    """``index`` (names, pairs or numbers) -> the index row, a scalar or an array."""
    index = trend.index
    tags = np.asarray(trend.tag)
    named = isinstance(index, tuple) or np.asarray(index).dtype.kind in "US"
    if not named:
        return np.asarray(index, dtype=np.float64)
    if tags.ndim != 0:
        raise ValueError(f"{name}.index: names need one tag for all reactors, use numbers with per-reactor tags")
    tag = TAGS[int(tags)] if tags.dtype.kind not in "US" and 0 <= int(tags) < len(TAGS) else str(tags)
    if isinstance(index, tuple):
        if tag not in _STATE_OF or len(index) != 2:
            raise ValueError(f"{name}.index: a (unit, state row) pair goes with the tags {tuple(_STATE_OF)}")
        units, rows = _STATE_OF[tag]
        unit, row = index
        if units is None and np.asarray(unit).dtype.kind in "US":
            raise ValueError(f"{name}.index: the slots of {tag!r} are numbered")
        return codes(unit, units or (), "loop" if tag == "control" else "channel") * len(rows) + codes(row, rows, "state row")
    units = _unit_names(tag)
    if units is None:
        raise ValueError(f"{name}.index: {tag!r} takes a number" + (" or a (unit, state row) pair" if tag in _STATE_OF else ""))
    return codes(index, units, "sensor" if units is SENSOR_NAMES else "channel")


def slot_rows(trend: Trend, n: int, name: str = "trend") -> np.ndarray:
    """(NT, N) rows of one slot."""
    if not isinstance(trend, Trend):
        raise TypeError(f"{name}: expected a Trend, got {type(trend).__name__}")
    return field_rows(trend, PARAM_ROWS, n, name, tag=codes(trend.tag, TAGS, "tag"), index=_index_row(trend, name))


def trend_block(n_reactors: int, *trends: Trend) -> np.ndarray:
    """The [WT_TRD_SLOTS][WT_NT][N] float64 block of ``wt_ensemble_trend_set``, checked by the library: slot k is the
    k-th trend, the slots after the last are off."""
    n = int(n_reactors)
    return slot_block(trends, n, SLOTS, "trend", slot_rows, np.zeros((NT, n)), _native.WT_PROG_TREND)
