"""Per-reactor injection programs that run on the device at every PLC scan (include/wtphys.h,
``wt_ensemble_inject_*``): scripted sensor spoofing and command tampering on the cyber layer between the plant and
its controller.

A program has up to four slots.  A slot spoofs one sensor reading on its way into the input image and the PI
programs, or tampers with one decoded actuator command on its way into the command path, while its window
``start <= t < end`` holds.  This module builds and checks the parameter block and unpacks the state; the
tampering itself runs in ``csrc/wt_inj.hpp``.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Union

import numpy as np

from . import _native
from ._program import SENSOR_NAMES, codes, field_rows, slot_block

SLOTS, NI, NIS = 4, 6, 4                 # WT_INJ_SLOTS, WT_NI, WT_NIS
PARAM_ROWS = ("mode", "target", "start", "end", "a", "b")
STATE_ROWS = ("n_applied", "t_first", "t_last", "held")
MODES = ("off", "bias", "gain", "constant", "ramp", "freeze", "dropout", "fault")
COMMAND_NAMES = ("acid_flow_rate", "chlorine_flow_rate", "inlet_flow_rate")
TARGETS = SENSOR_NAMES + COMMAND_NAMES   # index = target code (WT_INJ_CMD_ACID = 7 ...)

Value = Union[float, int, str, np.ndarray]


@dataclass
class Injection:
    """One slot.  ``target``: a name of :data:`TARGETS` or its index; ``mode``: a name of :data:`MODES` or its index.
    Active at the scans whose loop time t has ``start <= t < end``.  BIAS x + a, GAIN x * a, CONSTANT a,
    RAMP x + (a + b (t - start)), FREEZE the value at the first application, DROPOUT NaN, FAULT (sensors only) the
    fault code ``a`` (1..6).  Every field takes a scalar or an (N,) array."""

    target: Value
    mode: Value
    start: Value = 0.0
    end: Value = np.inf
    a: Value = 0.0
    b: Value = 0.0


@dataclass
class InjectionState:
    """``ReactorEnsemble.injection_state()``: (SLOTS, N) float64 each, indexed by slot and reactor."""

    n_applied: np.ndarray
    t_first: np.ndarray      # loop time of the first application (NaN: never applied)
    t_last: np.ndarray
    held: np.ndarray         # FREEZE: the value it replays (NaN otherwise)

    @classmethod
    def from_block(cls, block: np.ndarray) -> "InjectionState":
        """From a [WT_INJ_SLOTS][WT_NIS][N] block."""
        return cls(*(np.array(block[:, k]) for k in range(NIS)))

    def block(self) -> np.ndarray:
        """The (SLOTS, NIS, N) block again."""
        return np.stack([getattr(self, k) for k in STATE_ROWS], axis=1)


def _off_rows(n: int) -> np.ndarray:
    rows = np.zeros((NI, n))
    rows[PARAM_ROWS.index("end")] = np.inf
    return rows


def slot_rows(inj: Injection, n: int, name: str = "injection") -> np.ndarray:
    """(NI, N) rows of one slot."""
    if not isinstance(inj, Injection):
        raise TypeError(f"{name}: expected an Injection, got {type(inj).__name__}")
    return field_rows(inj, PARAM_ROWS, n, name, mode=codes(inj.mode, MODES, "mode"),
                      target=codes(inj.target, TARGETS, "target"))


def injection_block(n_reactors: int, *injections: Injection) -> np.ndarray:
    """The [WT_INJ_SLOTS][WT_NI][N] float64 block of ``wt_ensemble_inject_set``, checked by the library: slot k is the
    k-th injection, the slots after the last are off."""
    n = int(n_reactors)
    return slot_block(injections, n, SLOTS, "injection", slot_rows, _off_rows(n), _native.WT_PROG_INJECT)


def attack_window(block: np.ndarray):
    """Per reactor, the (earliest start, latest end) over the slots of a [WT_INJ_SLOTS][WT_NI][N] injection block that
    are not OFF; (+inf, +inf) where every slot is off.  The ground-truth label of a detector program:
    ``set_detectors(..., attack=attack_window(injection_block(...)))``."""
    block = np.asarray(block, dtype=np.float64)
    on = block[:, PARAM_ROWS.index("mode")] != MODES.index("off")
    start = np.where(on, block[:, PARAM_ROWS.index("start")], np.inf).min(axis=0)
    end = np.where(on, block[:, PARAM_ROWS.index("end")], -np.inf).max(axis=0)
    return start, np.where(on.any(axis=0), end, np.inf)
