"""Per-reactor response programs that run on the device at every PLC scan (include/wtphys.h,
``wt_ensemble_respond_*``): what an operator or a safety PLC does about what the alarm and detector programs noticed.

A program has up to four slots.  A slot watches a cause -- an alarm slot that is active, a detector slot whose alarm is
set, or a sensor whose image reading is not finite or faulted -- and, once the cause has stood for the slot's reaction
time, takes a dosing loop out of automatic: it holds the output, writes a fixed one or ramps to one, and the PI and
model predictive controllers skip the loop as they skip one a relay experiment has.  When the cause has been clear
long enough the slot hands the loop back, with or without a bump.  One reactor per reaction time, a score program as
the judge and ``mark()`` / ``rewind()`` for the unmitigated twin give the curve of harm against reaction time in one
launch.  This module builds the parameter block and unpacks the state; the library checks the block
(``wt_respond_check``), and the program itself runs in ``csrc/wt_rsp.hpp``.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Union

import numpy as np

from . import _native
from ._program import SENSOR_NAMES, codes, field_rows
from .control import LOOPS

SLOTS, NR, NRS, NRR = 4, 11, 14, 3       # WT_RSP_SLOTS, WT_NR, WT_NRS, WT_NRR
PARAM_ROWS = ("cause", "index", "delay", "loop", "action", "value", "rate", "latch", "clear_delay", "min_hold", "handback")
STATE_ROWS = ("phase", "pending", "clearing", "output", "t_first", "t_engaged", "t_released", "n_engaged", "time_engaged",
              "n_owned", "n_blocked", "n_cause", "n_tracked", "n_handback")
REACTOR_ROWS = ("t_prev", "owner_chlorine", "owner_acid")
CAUSES = ("off", "alarm", "detector", "bad")
ACTIONS = ("hold", "manual", "ramp")
HANDBACKS = ("bump", "bumpless")
PHASES = ("idle", "engaged")             # the codes of ``ResponseState.phase``

Value = Union[float, int, str, np.ndarray]


@dataclass
class Response:
    """One slot.  ``cause``: "alarm" (slot ``index`` of the alarm program is active), "detector" (slot ``index`` of the
    detector program has its alarm set), "bad" (the image reading of sensor ``index``, a name of :data:`SENSOR_NAMES` or
    its index, is not finite or faulted) or "off".  ``loop``: "chlorine" or "acid".  ``delay``: seconds the cause must
    have stood without interruption before the slot engages -- the reaction time; 0 engages on the scan that first sees
    the cause.  ``action``: "hold" (the output the loop had at engagement), "manual" (``value``) or "ramp" (from the
    output at engagement towards ``value`` by at most ``rate`` per second).  A latched slot stays engaged until
    ``reset_responses()``; an unlatched one releases on the first scan at which the cause has been clear for
    ``clear_delay`` seconds and the slot engaged for ``min_hold`` seconds.  ``handback``: "bump" (the controllers
    continue from their own state) or "bumpless" (they continue from the forced output).  Every field takes a scalar or
    an (N,) array."""

    cause: Value
    index: Value
    loop: Value
    action: Value = "hold"
    value: Value = 0.0
    delay: Value = 0.0
    rate: Value = 0.0
    latch: Value = False
    clear_delay: Value = 0.0
    min_hold: Value = 0.0
    handback: Value = "bump"


@dataclass
class ResponseState:
    """``ReactorEnsemble.response_state()``: slot fields (SLOTS, N), reactor fields (N,), float64."""

    phase: np.ndarray          # 0 idle, 1 engaged
    pending: np.ndarray        # loop time since which the cause has stood while idle (NaN: none)
    clearing: np.ndarray       # loop time since which the cause has been clear while engaged (NaN: none)
    output: np.ndarray         # the forced output
    t_first: np.ndarray        # loop time of the first engagement (NaN: never)
    t_engaged: np.ndarray      # of the last engagement
    t_released: np.ndarray     # of the last release
    n_engaged: np.ndarray      # engagements
    time_engaged: np.ndarray   # seconds engaged
    n_owned: np.ndarray        # scans in which the slot wrote its loop's words
    n_blocked: np.ndarray      # engaged scans in which a relay experiment had the loop
    n_cause: np.ndarray        # scans with the cause true
    n_tracked: np.ndarray      # engaged scans in which a lower slot had the loop
    n_handback: np.ndarray     # bumpless hand-backs
    t_prev: np.ndarray
    owner_chlorine: np.ndarray  # the slot that owned the loop in the last scan (-1: none)
    owner_acid: np.ndarray

    @classmethod
    def from_block(cls, slot_block: np.ndarray, reactor_block: np.ndarray) -> "ResponseState":
        """From a [WT_RSP_SLOTS][WT_NRS][N] and a [WT_NRR][N] block."""
        return cls(*(np.array(slot_block[:, k]) for k in range(NRS)), *(np.array(reactor_block[k]) for k in range(NRR)))

    def block(self):
        """The (SLOTS, NRS, N) and (NRR, N) blocks again."""
        return (np.stack([getattr(self, k) for k in STATE_ROWS], axis=1),
                np.stack([getattr(self, k) for k in REACTOR_ROWS]))


def slot_rows(response: Response, n: int, name: str = "response") -> np.ndarray:
    """(NR, N) rows of one slot."""
    if not isinstance(response, Response):
        raise TypeError(f"{name}: expected a Response, got {type(response).__name__}")
    return field_rows(response, PARAM_ROWS, n, name, cause=codes(response.cause, CAUSES, "cause"),
                      index=codes(response.index, SENSOR_NAMES, "sensor"), loop=codes(response.loop, LOOPS, "loop"),
                      action=codes(response.action, ACTIONS, "action"), handback=codes(response.handback, HANDBACKS, "handback"))


def response_block(n_reactors: int, *responses: Response) -> np.ndarray:
    """The [WT_RSP_SLOTS][WT_NR][N] float64 block of ``wt_ensemble_respond_set``, checked by the library: slot k is the
    k-th response, the slots after the last are off."""
    n = int(n_reactors)
    if len(responses) > SLOTS:
        raise ValueError(f"at most {SLOTS} responses per program, got {len(responses)}")
    rows = [slot_rows(item, n, f"response {k}") for k, item in enumerate(responses)]
    rows += [np.zeros((NR, n))] * (SLOTS - len(responses))
    block = np.ascontiguousarray(np.stack(rows))
    try:
        _native.check(_native.lib().wt_respond_check(n, _native.dptr(block)))
    except _native.WtError as e:   # WT_E_ARG is the only error it returns
        raise ValueError(e.message) from None
    return block
