"""The junction program (include/wtphys.h, ``wt_ensemble_junction_*``): flow-weighted merges and splits in a treatment
train, inside the step call.

On top of a train program.  A real plant is not a chain: a rapid mix splits into parallel contact tanks, the tanks
merge into one clearwell, a bypass blends part-treated water back in, a recycle returns water upstream.  A linked
reactor with at least one source slot (stage, share) is a *junction*: after every outer step in which all its sources
stepped, its inlet rows get the blend of the sources' outlet zones, weighted by ``share * the source's inlet flow`` --
chlorine and temperature as flow-weighted means, pH through the flow-weighted mean of H+ -- instead of the outlet of
stage - 1.  With ``carry`` the junction's own inlet flow becomes the sum of those flows.  A split needs nothing of its
own: several junctions name the same source, each with the share of its flow they take.  This module builds the
parameter block and unpacks the state; the library checks the block, and the blend itself runs in ``csrc/wt_trn.hpp``.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional, Sequence

import numpy as np

from . import _native

JCT_SLOTS, NJ, NJS = 4, 2, 3                              # WT_JCT_SLOTS, WT_NJ, WT_NJS
PARAM_ROWS = ("stage", "share")
STATE_ROWS = ("n_blend", "n_held", "q_last")
UNUSED = -1                                               # stage code of a slot that names no source


@dataclass
class Junction:
    """One junction, the same in every selected train: stage ``to_stage`` is fed by the blend of ``from_stages`` (up to
    four other stages of the train, in slot order), each with its ``shares`` entry of that stage's inlet flow (a
    scalar serves all; a (trains,) array per source gives every selected train its own).  ``carry``: the junction's
    inlet flow becomes the summed flow.  ``trains``: a boolean mask or an index selection over the N / length trains
    (default: all)."""

    to_stage: int
    from_stages: Sequence[int]
    shares: object = 1.0
    carry: bool = False
    trains: Optional[object] = None


def check(length: int, linked: np.ndarray, block: np.ndarray, carry: np.ndarray) -> None:
    """The checks ``wt_ensemble_junction_set`` makes on a [WT_JCT_SLOTS][WT_NJ][N] block and its (N,) ``carry`` for
    trains of ``length`` stages whose links are ``linked`` (N,); ``ValueError`` names the first one that fails."""
    n = block.shape[-1]
    tr = np.stack([np.asarray(linked, dtype=np.float64), np.full(n, 7.0)])
    try:
        _native.check(_native.lib().wt_junction_check(int(length), n, _native.dptr(tr), _native.dptr(block),
                                                      _native.dptr(carry)))
    except _native.WtError as e:   # WT_E_ARG is the only error it returns
        raise ValueError(e.message) from None


def junction_block(n_reactors: int, length: int, linked, *junctions: Junction):
    """The [WT_JCT_SLOTS][WT_NJ][N] float64 block and the (N,) carry array of ``wt_ensemble_junction_set`` for
    N / ``length`` trains whose links are ``linked`` (a scalar or (N,), as ``train_block`` takes it), checked by the
    library: no slot used, then the ``junctions`` in order (a later one replaces an earlier one on the same stage)."""
    n, length = int(n_reactors), int(length)
    if length < 1 or n % length:
        raise ValueError("n_reactors must be a multiple of length (an ensemble holds whole trains)")
    link = np.array(np.broadcast_to(np.asarray(linked, dtype=np.float64), (n,)))
    link[::length] = 0.0
    block = np.zeros((JCT_SLOTS, NJ, n))
    block[:, 0] = UNUSED
    carry = np.zeros(n)
    first = np.arange(0, n, length)
    for k, j in enumerate(junctions):
        if not (isinstance(j.to_stage, (int, np.integer)) and 0 <= j.to_stage < length):
            raise ValueError(f"junction {k}: to_stage must be a stage of the train, 0..{length - 1}")
        src = list(j.from_stages)
        if not 1 <= len(src) <= JCT_SLOTS:
            raise ValueError(f"junction {k}: from_stages must name 1..{JCT_SLOTS} stages")
        try:
            at = first if j.trains is None else first[np.asarray(j.trains)]
        except IndexError:
            raise ValueError(f"junction {k}: trains must select among the {n // length} trains") from None
        at = np.atleast_1d(at) + int(j.to_stage)
        try:
            shares = np.broadcast_to(np.asarray(j.shares, dtype=np.float64).T, (at.size, len(src))).T
        except ValueError:
            raise ValueError(f"junction {k}: shares must be a scalar, one per source, or (sources, trains) values, "
                             f"got shape {np.shape(j.shares)}") from None
        block[:, 0, at] = UNUSED
        block[:, 1, at] = 0.0
        for s, g in enumerate(src):
            block[s, 0, at] = float(g)
            block[s, 1, at] = shares[s]
        carry[at] = 1.0 if j.carry else 0.0
    check(length, link, block, carry)
    return block, carry


@dataclass
class JunctionState:
    """``ReactorEnsemble.junction_state()``: (N,) float64 each."""

    n_blend: np.ndarray        # feeds a junction got inside step calls
    n_held: np.ndarray         # outer steps in which a source was live but nothing was fed
    q_last: np.ndarray         # the summed flow of the last feed, NaN before the first

    @classmethod
    def from_block(cls, state: np.ndarray) -> "JunctionState":
        """From a [WT_NJS][N] state block."""
        return cls(np.array(state[0]), np.array(state[1]), np.array(state[2]))

    def block(self) -> np.ndarray:
        """The (NJS, N) block again."""
        return np.stack([getattr(self, k) for k in STATE_ROWS])
