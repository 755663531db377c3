"""Per-reactor link programs that run on the device at every PLC scan (include/wtphys.h, ``wt_ensemble_link_*``):
what the fieldbus between the plant and its controller does to a signal in time -- delay, loss and replay.

A program has up to four slots.  A slot sits on one channel of the plant's I/O (a reading on its way into the input
image and the controllers, or a decoded command on its way into the command path), keeps a ring of the channel's last
64 samples, and while its window ``start <= t < end`` holds delivers the sample of some scans ago (``Link.delay``), the
last value that came through with a timeout into a fail state (``Link.loss``), or a taped stretch of the channel's own
past in a loop (``Link.replay``).  It runs before the injection program on both paths, so a delayed remote analyser is
a wire plus a link, and one reactor per delay gives the curve of harm against network delay in one launch.  This module
builds the parameter block and unpacks the state; the library checks the block (``wt_link_check``), and the program
itself runs in ``csrc/wt_lnk.hpp``.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Union

import numpy as np

from . import _native
from ._program import codes, field_rows
from .inject import TARGETS

SLOTS, DEPTH, NL, NLS = 4, 64, 8, 10     # WT_LNK_SLOTS, WT_LNK_DEPTH, WT_NL, WT_NLS
PARAM_ROWS = ("mode", "target", "start", "end", "a", "b", "timeout", "fail")
STATE_ROWS = ("n_rec", "n_applied", "n_fresh", "n_lost", "n_timeout", "n_draw", "t_fresh", "held_value", "held_fault",
              "tape_end")
MODES = ("off", "delay", "loss", "replay")
N_READINGS = 7                           # targets below it are readings, the others commands

Value = Union[float, int, str, np.ndarray]


@dataclass
class Link:
    """One slot.  ``target``: a name of :data:`TARGETS` (the injection program's) or its index; ``mode``: a name of
    :data:`MODES` or its index.  Active at the scans whose loop time t has ``start <= t < end``.  DELAY: ``a`` scans
    late, plus a jitter of 0..``b`` scans drawn per scan.  LOSS: each scan's update is lost with probability ``a`` and
    the receiver holds the last value; after ``timeout`` seconds without a fresh one a reading becomes NaN with the fault
    code ``fail`` (1..6) and a command the value ``fail``.  REPLAY: the ``a`` scans before the window, in a loop.  A
    field a mode does not use stays at its default.  Every field takes a scalar or an (N,) array; the constructors
    :meth:`delay`, :meth:`loss` and :meth:`replay` name the fields by what they mean."""

    target: Value
    mode: Value
    start: Value = 0.0
    end: Value = np.inf
    a: Value = 0.0
    b: Value = 0.0
    timeout: Value = np.inf
    fail: Value = 0.0

    @classmethod
    def delay(cls, target: Value, scans: Value, jitter: Value = 0.0, start: Value = 0.0, end: Value = np.inf) -> "Link":
        """The sample of ``scans`` scans ago (the oldest recorded while there are fewer), ``scans`` + 0..``jitter``
        with jitter; whole numbers, ``scans + jitter <= 63``."""
        return cls(target, "delay", start, end, a=scans, b=jitter)

    @classmethod
    def loss(cls, target: Value, probability: Value, start: Value = 0.0, end: Value = np.inf, timeout: Value = np.inf,
             fail: Value = None) -> "Link":
        """Updates lost with ``probability`` (1: a denial of service); ``timeout`` seconds after the last fresh value the
        receiver gets the fail state.  ``fail`` defaults to fault code 1 (open circuit) for a reading and to 0.0 for a
        command, and to nothing where there is no timeout."""
        if fail is None:
            reading = codes(target, TARGETS, "target") < N_READINGS
            fail = np.where(np.isinf(np.asarray(timeout, dtype=np.float64)), 0.0, np.where(reading, 1.0, 0.0))
        return cls(target, "loss", start, end, a=probability, timeout=timeout, fail=fail)

    @classmethod
    def replay(cls, target: Value, length: Value, start: Value = 0.0, end: Value = np.inf) -> "Link":
        """The last ``length`` scans (1..63) before ``start``, played in a loop until ``end``."""
        return cls(target, "replay", start, end, a=length)


@dataclass
class LinkState:
    """``ReactorEnsemble.link_state()``: (SLOTS, N) float64 each, indexed by slot and reactor."""

    n_rec: np.ndarray        # samples recorded into the ring since set
    n_applied: np.ndarray    # scans inside the window
    n_fresh: np.ndarray      # of those, deliveries that count as fresh
    n_lost: np.ndarray       # LOSS: updates lost
    n_timeout: np.ndarray    # LOSS: scans that delivered the fail state
    n_draw: np.ndarray       # uniform draws taken
    t_fresh: np.ndarray      # loop time of the last fresh delivery (NaN: none yet)
    held_value: np.ndarray   # the last fresh delivery
    held_fault: np.ndarray
    tape_end: np.ndarray     # REPLAY: n_rec when the window opened (NaN outside one)

    @classmethod
    def from_block(cls, block: np.ndarray) -> "LinkState":
        """From a [WT_LNK_SLOTS][WT_NLS][N] block."""
        return cls(*(np.array(block[:, k]) for k in range(NLS)))

    def block(self) -> np.ndarray:
        """The (SLOTS, NLS, N) block again."""
        return np.stack([getattr(self, k) for k in STATE_ROWS], axis=1)


def _off_rows(n: int) -> np.ndarray:
    rows = np.zeros((NL, n))
    rows[PARAM_ROWS.index("end")] = np.inf
    rows[PARAM_ROWS.index("timeout")] = np.inf
    return rows


def slot_rows(link: Link, n: int, name: str = "link") -> np.ndarray:
    """(NL, N) rows of one slot."""
    if not isinstance(link, Link):
        raise TypeError(f"{name}: expected a Link, got {type(link).__name__}")
    return field_rows(link, PARAM_ROWS, n, name, mode=codes(link.mode, MODES, "mode"), target=codes(link.target, TARGETS, "target"))


def link_block(n_reactors: int, *links: Link) -> np.ndarray:
    """The [WT_LNK_SLOTS][WT_NL][N] float64 block of ``wt_ensemble_link_set``, checked by the library: slot k is the
    k-th link, the slots after the last are off."""
    n = int(n_reactors)
    if len(links) > SLOTS:
        raise ValueError(f"at most {SLOTS} links per program, got {len(links)}")
    rows = [slot_rows(item, n, f"link {k}") for k, item in enumerate(links)]
    rows += [_off_rows(n)] * (SLOTS - len(links))
    block = np.ascontiguousarray(np.stack(rows))
    try:
        _native.check(_native.lib().wt_link_check(n, _native.dptr(block)))
    except _native.WtError as e:   # WT_E_ARG is the only error it returns
        raise ValueError(e.message) from None
    return block


def attack_window(block: np.ndarray):
    """Per reactor, the (earliest start, latest end) over the slots of a [WT_LNK_SLOTS][WT_NL][N] link block that are
    not OFF; (+inf, +inf) where every slot is off: the semantics of :func:`inject.attack_window`, so a detector program
    can be labelled with a link attack, ``set_detectors(..., attack=attack_window(link_block(...)))``."""
    block = np.asarray(block, dtype=np.float64)
    on = block[:, PARAM_ROWS.index("mode")] != MODES.index("off")
    start = np.where(on, block[:, PARAM_ROWS.index("start")], np.inf).min(axis=0)
    end = np.where(on, block[:, PARAM_ROWS.index("end")], -np.inf).max(axis=0)
    return start, np.where(on.any(axis=0), end, np.inf)
