"""Per-reactor actuator programs that run on the device at every PLC scan (include/wtphys.h,
``wt_ensemble_actuator_*``): the dosing pumps and the inlet valve between the command path and the plant.

A program has one optional final element per channel: acid (boundary row 4), chlorine (row 6) and inlet (row 0).  Each
has dead time in scans, a first-order lag, a rate limit, backlash and a STUCK or FAIL_TO fault window; its position
is what the plant receives, downstream of PI outputs, tampered commands and interlock trips.  This module builds and
checks the parameter block and unpacks the state; the evaluation itself runs in ``csrc/wt_act.hpp``.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Union

import numpy as np

from . import _native
from ._program import check, codes, field_rows

CHANNELS = ("acid", "chlorine", "inlet")   # WT_ACT_ACID, WT_ACT_CHLORINE, WT_ACT_INLET: the order of WT_INJ_CMD_*
ROWS = (4, 6, 0)                           # the boundary row of each channel
NV, NVS, MAX_DELAY = 9, 9, 8               # WT_NV, WT_NVS, WT_ACT_MAX_DELAY
PARAM_ROWS = ("enable", "tau", "rate", "backlash", "delay", "fault", "t_fault", "t_repair", "fail_value")
STATE_ROWS = ("position", "applied", "play", "demand", "delivered", "travel", "n_exec", "n_rate", "n_fault")
FAULTS = ("none", "stuck", "fail_to")
# the rows of a channel without an actuator: the defaults of :class:`Actuator`, enable 0
OFF_ROW = np.array([0.0, 0.0, np.inf, 0.0, 0.0, 0.0, 0.0, np.inf, 0.0])

Value = Union[float, int, str, np.ndarray]


@dataclass
class Actuator:
    """The final element of one channel ("acid", "chlorine" or "inlet").  ``tau``: first-order lag in seconds;
    ``rate``: largest change of position per second; ``backlash``: width of the play band; ``delay``: dead time in
    scans (0..8); ``fault``: "none", "stuck" (the position holds) or "fail_to" (the position is ``fail_value``) for
    loop times t_fault <= t < t_repair.  Every field takes a scalar or an (N,) array.  With the defaults the element
    passes every command through unchanged."""

    channel: str
    tau: Value = 0.0
    rate: Value = np.inf
    backlash: Value = 0.0
    delay: Value = 0
    fault: Value = "none"
    t_fault: Value = 0.0
    t_repair: Value = np.inf
    fail_value: Value = 0.0


@dataclass
class ActuatorState:
    """``ReactorEnsemble.actuator_state()``: channel fields (3, N), ``queue`` (3, 8, N), ``t_prev`` (N,), float64."""

    position: np.ndarray       # where the element stands (a double, not a float32 register)
    applied: np.ndarray        # the flow the plant receives: position clamped to the channel's limit
    play: np.ndarray           # output of the backlash band
    demand: np.ndarray         # the command of the last scan
    delivered: np.ndarray      # integral of applied over loop time (up to the last scan)
    travel: np.ndarray         # total distance moved
    n_exec: np.ndarray         # evaluations
    n_rate: np.ndarray         # evaluations the rate limit cut
    n_fault: np.ndarray        # evaluations inside the fault window
    queue: np.ndarray          # the last 8 demands, newest first
    t_prev: np.ndarray

    @classmethod
    def from_block(cls, state: np.ndarray, queue: np.ndarray, t_prev: np.ndarray) -> "ActuatorState":
        """From a [3][WT_NVS][N] state block, a [3][8][N] queue and a [N] t_prev."""
        return cls(*(np.array(state[:, k]) for k in range(NVS)), np.array(queue), np.array(t_prev))

    def block(self):
        """The (3, NVS, N) state block, the (3, 8, N) queue and the (N,) t_prev again."""
        return np.stack([getattr(self, k) for k in STATE_ROWS], axis=1), self.queue, self.t_prev


def channel_rows(act: Actuator, n: int, name: str = "actuator") -> np.ndarray:
    """(NV, N) rows of one channel, enable = 1."""
    if not isinstance(act, Actuator):
        raise TypeError(f"{name}: expected an Actuator, got {type(act).__name__}")
    return field_rows(act, PARAM_ROWS, n, name, enable=1.0, fault=codes(act.fault, FAULTS, "fault"))


def actuator_block(n_reactors: int, *actuators: Actuator) -> np.ndarray:
    """The [WT_ACT_CHANNELS][WT_NV][N] float64 block of ``wt_ensemble_actuator_set``, checked by the library: each
    actuator fills the rows of its channel, a channel without one holds :data:`OFF_ROW` (the defaults with enable 0)."""
    n = int(n_reactors)
    block = np.repeat(np.repeat(OFF_ROW[None, :, None], len(CHANNELS), axis=0), n, axis=2)
    seen = set()
    for k, act in enumerate(actuators):
        if not isinstance(act, Actuator):
            raise TypeError(f"actuator {k}: expected an Actuator, got {type(act).__name__}")
        if act.channel not in CHANNELS:
            raise ValueError(f"unknown channel {act.channel!r}: one of {CHANNELS}")
        if act.channel in seen:
            raise ValueError(f"two actuators on the {act.channel} channel: at most one per channel")
        seen.add(act.channel)
        block[CHANNELS.index(act.channel)] = channel_rows(act, n, f"actuator {act.channel}")
    check(_native.WT_PROG_ACTUATOR, block)
    return block
