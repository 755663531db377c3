"""Per-reactor score programs evaluated on the device after every outer step (include/wtphys.h,
``wt_ensemble_score_*``): what happened to the water.

A program has up to four slots.  Each judges one quantity of the true reactor state (pH, chlorine or temperature of
one zone, or the minimum, maximum or mean over the zones) against a band and accumulates per reactor the time below
and above it, the deficit and excess areas, the exposure integral and the excursion runs.  An optional ensemble curve
counts per outer step how many reactors were scored, below and above, and a coarse histogram of the value (the fan)
gives quantile bands over time.  This module builds and checks the parameter block and unpacks the results; the
evaluation itself runs in ``csrc/wt_scr.hpp``.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional, Union

import numpy as np

from . import _native, _program

SLOTS, NSP, NSS, MAX_BINS = 4, 8, 15, 32                  # WT_SCR_SLOTS, WT_NSP, WT_NSS, WT_SCR_MAX_BINS
KINDS = ("off", "band")                                   # WT_SCR_OFF, WT_SCR_BAND
QUANTITIES = ("pH", "chlorine", "temperature")            # WT_SQ_*
REDUCES = ("zone", "min", "max", "mean")                  # WT_SR_*
PARAM_ROWS = ("kind", "quantity", "reduce", "zone", "lo", "hi", "t_start", "t_end")
STATE_ROWS = ("n_eval", "time", "integral", "t_low", "t_high", "area_low", "area_high", "v_min", "v_max", "last", "out",
              "n_exc", "t_first_out", "run", "run_max")
# an unused slot: kind off
OFF_ROW = np.array([0.0, 0.0, 0.0, -1.0, -np.inf, np.inf, -np.inf, np.inf])

Value = Union[float, int, np.ndarray]


@dataclass
class Score:
    """One slot: ``quantity`` ("pH", "chlorine", "temperature" or its code) of zone ``zone`` (-1: the last zone, the
    outlet), or its ``reduce`` ("min", "max", "mean") over the zones, judged against ``lo <= v <= hi`` while
    ``t_start <= t < t_end``.  Every numeric field takes a scalar or an (N,) array."""

    quantity: Union[str, int, np.ndarray]
    lo: Value = -np.inf
    hi: Value = np.inf
    reduce: Union[str, int, np.ndarray] = "zone"
    zone: Value = -1
    t_start: Value = -np.inf
    t_end: Value = np.inf
    kind: Union[str, int] = "band"


@dataclass
class ScoreState:
    """``ReactorEnsemble.score_state()``: slot rows (4, N), ``t_prev`` (N,), float64."""

    n_eval: np.ndarray         # evaluations inside the window
    time: np.ndarray           # scored time [s]
    integral: np.ndarray       # integral of v dt (outlet chlorine: the CT exposure)
    t_low: np.ndarray          # time below lo
    t_high: np.ndarray         # time above hi
    area_low: np.ndarray       # integral of (lo - v) dt while below (the deficit)
    area_high: np.ndarray      # integral of (v - hi) dt while above
    v_min: np.ndarray          # NaN before the first evaluation, like v_max, last and t_first_out
    v_max: np.ndarray
    last: np.ndarray
    out: np.ndarray            # 1 while outside the band
    n_exc: np.ndarray          # excursions (entries into violation)
    t_first_out: np.ndarray    # time of the first violation
    run: np.ndarray            # length of the violation in progress
    run_max: np.ndarray        # longest contiguous violation
    t_prev: np.ndarray         # ReactorState.time of the last evaluation

    @classmethod
    def from_block(cls, state: np.ndarray, t_prev: np.ndarray) -> "ScoreState":
        """From a [SLOTS][WT_NSS][N] state block and a [N] t_prev."""
        return cls(*(np.array(state[:, k]) for k in range(NSS)), np.array(t_prev))


@dataclass
class ScoreCurve:
    """``ReactorEnsemble.score_curve()``: per outer step since ``set_scores`` / ``reset_scores`` and per slot, how many
    reactors were scored, below and above the band: (n_steps, 4) int32.  ``fan`` (n_steps, 4, bins + 2) counts the
    scored value per bin (bin 0 below ``edges[s, 0]``, bin bins + 1 at or above ``edges[s, -1]``), ``edges`` (4, bins +
    1) are the bin edges; both None without a fan."""

    n_scored: np.ndarray
    n_low: np.ndarray
    n_high: np.ndarray
    fan: Optional[np.ndarray] = None
    edges: Optional[np.ndarray] = None

    def quantiles(self, q) -> np.ndarray:
        """(len(q), n_steps, 4) quantiles of the scored value, interpolated linearly inside the fan's bins.  A
        quantile that falls below the fan's range gives its lower edge, one above it the upper edge; steps that
        scored nothing give NaN."""
        if self.fan is None:
            raise ValueError("the curve has no fan (set_scores(..., bins=B))")
        q = np.atleast_1d(np.asarray(q, dtype=np.float64))
        K, S, B2 = self.fan.shape
        out = np.full((len(q), K, S), np.nan)
        cum = np.cumsum(self.fan, axis=2, dtype=np.int64)
        for j in range(K):
            for s in range(S):
                total = cum[j, s, -1]
                if total == 0:
                    continue
                for i, qi in enumerate(q):
                    want = qi * total
                    b = min(int(np.searchsorted(cum[j, s], want, side="left")), B2 - 1)
                    if b == 0:
                        out[i, j, s] = self.edges[s, 0]
                    elif b == B2 - 1:
                        out[i, j, s] = self.edges[s, -1]
                    else:
                        below, inside = cum[j, s, b - 1], self.fan[j, s, b]
                        e0, e1 = self.edges[s, b - 1], self.edges[s, b]
                        out[i, j, s] = e0 + (e1 - e0) * (want - below) / inside
        return out


def fan_edges(fan_lo, fan_hi, bins: int) -> np.ndarray:
    """(4, bins + 1) bin edges of a fan between ``fan_lo`` and ``fan_hi`` (4,)."""
    return np.linspace(np.asarray(fan_lo, dtype=np.float64), np.asarray(fan_hi, dtype=np.float64), int(bins) + 1, axis=1)


def slot_rows(s: Score, n: int, name: str = "score") -> np.ndarray:
    """(NSP, N) rows of one slot."""
    if not isinstance(s, Score):
        raise TypeError(f"{name}: expected a Score, got {type(s).__name__}")
    return _program.field_rows(s, PARAM_ROWS, n, name, kind=_program.codes(s.kind, KINDS, "kind"),
                               quantity=_program.codes(s.quantity, QUANTITIES, "quantity"),
                               reduce=_program.codes(s.reduce, REDUCES, "reduce"))


def score_block(n_reactors: int, *scores: Score) -> np.ndarray:
    """The [WT_SCR_SLOTS][WT_NSP][N] float64 block of ``wt_ensemble_score_set``, checked by the library: slot k holds
    score k, the slots after the last one :data:`OFF_ROW`."""
    return _program.slot_block(scores, int(n_reactors), SLOTS, "score", slot_rows, np.repeat(OFF_ROW[:, None], int(n_reactors), axis=1),
                               _native.WT_PROG_SCORE)
