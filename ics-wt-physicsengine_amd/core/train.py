"""The train program (include/wtphys.h, ``wt_ensemble_train_*``): reactors coupled into treatment trains inside the
step call.

An ensemble of N reactors is read as N / length trains of ``length`` stages (rapid mix, contact tank, clearwell):
reactor r is stage ``r % length`` of train ``r // length``.  After every outer step its upstream took, a linked stage
gets the upstream's outlet zone (pH, chlorine, temperature) in its boundary rows inlet_pH, inlet_chlorine and
inlet_temperature -- the boundary of its next outer step.  Flows are not carried: every tank keeps its own inlet flow.
This module builds and checks the parameter block and unpacks the state; the feed itself runs in ``csrc/wt_trn.hpp``.

The pipe program (``wt_ensemble_pipe_*``) on top of it gives a link a dead time of D whole outer steps: the upstream's
outlet goes through a FIFO of D samples before it reaches the downstream's rows.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from . import _native

NTR, NTRS = 2, 2                                          # WT_NTR, WT_NTRS
PARAM_ROWS = ("link", "rows")
STATE_ROWS = ("n_fed", "t_last")
NPS, PIPE_MAX_DELAY = 2, 4095                             # WT_NPS, WT_PIPE_MAX_DELAY
PIPE_STATE_ROWS = ("n_sent", "t_sent")
PIPE_SAMPLE = ("pH", "chlorine", "temperature", "time")   # the four numbers of a sample in a line
ROW_BITS = {"pH": 1, "chlorine": 2, "temperature": 4}     # WT_TRN_PH, WT_TRN_CHLORINE, WT_TRN_TEMPERATURE
ALL_ROWS = tuple(ROW_BITS)


def rows_mask(rows) -> np.ndarray:
    """``rows`` -> float64 mask(s) 1 pH | 2 chlorine | 4 temperature: a name or a sequence of names (one mask for all
    reactors), or numbers that are masks already (a scalar or an (N,) array; the library checks their range)."""
    if isinstance(rows, str):
        rows = (rows,)
    a = np.asarray(rows)
    if a.size == 0:
        return np.float64(0.0)
    if a.dtype.kind in "US":
        bad = [str(s) for s in a.ravel() if str(s) not in ROW_BITS]
        if bad:
            raise ValueError(f"unknown train row {bad[0]!r}: one of {ALL_ROWS}")
        mask = 0
        for s in a.ravel():
            mask |= ROW_BITS[str(s)]
        return np.float64(mask)
    return a.astype(np.float64)


def check(length: int, n_zones: int, block: np.ndarray) -> None:
    """The checks ``wt_ensemble_train_set`` makes on ``length`` and a [WT_NTR][N] block for ``n_zones`` zones;
    ``ValueError`` names the first one that fails."""
    try:
        _native.check(_native.lib().wt_train_check(int(length), int(n_zones), block.shape[-1], _native.dptr(block)))
    except _native.WtError as e:   # WT_E_ARG is the only error it returns
        raise ValueError(e.message) from None


def train_block(n_reactors: int, n_zones: int, length: int, linked=True, rows=ALL_ROWS) -> np.ndarray:
    """The [WT_NTR][N] float64 block of ``wt_ensemble_train_set``, checked by the library.  ``linked``: a scalar or an
    (N,) array of truth values; the first stage of every train has no upstream and is never linked, whatever
    ``linked`` says there.  ``rows``: see :func:`rows_mask`."""
    n, length = int(n_reactors), int(length)
    block = np.empty((NTR, n))
    for i, (name, v) in enumerate((("linked", np.asarray(linked, dtype=np.float64)), ("rows", rows_mask(rows)))):
        try:
            block[i] = np.broadcast_to(v, (n,))
        except ValueError:
            raise ValueError(f"train.{name}: expected a scalar or ({n},) values, got shape {np.shape(v)}") from None
    if length >= 1:
        block[0, ::length] = 0.0
    check(length, n_zones, block)
    return block


@dataclass
class TrainState:
    """``ReactorEnsemble.train_state()``: (N,) float64 each, and the shape of the handle while the program is set."""

    n_fed: np.ndarray          # feeds the step kernel wrote into this reactor
    t_last: np.ndarray         # the upstream's ReactorState.time at the last of them, NaN before the first
    length: int = 0            # stages per train
    per_wavefront: int = 0     # reactors per wavefront (a multiple of length)

    @classmethod
    def from_block(cls, state: np.ndarray, length: int = 0, per_wavefront: int = 0) -> "TrainState":
        """From a [WT_NTRS][N] state block."""
        return cls(np.array(state[0]), np.array(state[1]), int(length), int(per_wavefront))

    def block(self) -> np.ndarray:
        """The (NTRS, N) block again."""
        return np.stack([getattr(self, k) for k in STATE_ROWS])


def pipe_delay(seconds: float, dt: float) -> int:
    """The delay in whole outer steps of length ``dt`` [s] nearest to a dead time of ``seconds`` (a half rounds up)."""
    seconds, dt = float(seconds), float(dt)
    if not (np.isfinite(dt) and dt > 0.0):
        raise ValueError(f"pipe_delay: dt must be positive and finite, got {dt}")
    if not (np.isfinite(seconds) and seconds >= 0.0):
        raise ValueError(f"pipe_delay: the dead time must be finite and not negative, got {seconds}")
    return int(np.floor(seconds / dt + 0.5))


def pipe_block(n_reactors: int, length: int, delay, linked=True) -> np.ndarray:
    """The (N,) float64 delays of ``wt_ensemble_pipe_set`` for trains of ``length`` stages whose links are ``linked``
    (as :func:`train_block` takes it), checked by the library.  ``delay``: a scalar or an (N,) array of whole outer
    steps, 0..``PIPE_MAX_DELAY``; first stages and stages that are not linked have no pipe and get 0, whatever
    ``delay`` says there."""
    n, length = int(n_reactors), int(length)
    if length < 1:
        raise ValueError(f"train.length: expected at least 1, got {length}")
    out = []
    for name, v in (("linked", linked), ("delay", delay)):
        try:
            out.append(np.array(np.broadcast_to(np.asarray(v, dtype=np.float64), (n,))))
        except ValueError:
            raise ValueError(f"train.{name}: expected a scalar or ({n},) values, got shape {np.shape(v)}") from None
    link, d = out
    link[::length] = 0.0
    d[link == 0.0] = 0.0
    blk = np.stack([link, np.full(n, 7.0)])
    try:
        _native.check(_native.lib().wt_pipe_check(n, _native.dptr(blk), _native.dptr(d)))
    except _native.WtError as e:   # WT_E_ARG is the only error it returns
        raise ValueError(e.message) from None
    return d


@dataclass
class PipeState:
    """``ReactorEnsemble.pipe_state()``: (N,) float64 each, and the ring slots of the program (largest delay + 1)."""

    n_sent: np.ndarray         # feeds that went through this reactor's line inside step calls
    t_sent: np.ndarray         # the time stamp of the sample last delivered by one, NaN: none, or one of the initial fill
    delay: np.ndarray          # the delay of the link into this reactor [outer steps]
    slots: int = 0
