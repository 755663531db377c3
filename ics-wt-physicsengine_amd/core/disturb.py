"""Per-reactor disturbance programs generated on the device after every outer step (include/wtphys.h,
``wt_ensemble_disturb_*``): a raw-water side and chemical stocks that move on their own.

A program has up to four slots.  Each moves one boundary row the command path does not own (inlet pH, chlorine and
temperature, the two stock concentrations, ambient temperature, heat-loss coefficient) by a step, a ramp, a sine or an
Ornstein-Uhlenbeck process; the rows are ``clamp(base + offsets)``.  This module builds and checks the parameter block
and unpacks the state; the evaluation itself runs in ``csrc/wt_dst.hpp``.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Union

import numpy as np

from . import _native, _program, params

SLOTS, ND, NDS = 4, 7, 4                                  # WT_DST_SLOTS, WT_ND, WT_NDS
KINDS = ("off", "step", "ramp", "sine", "ou")             # WT_DST_OFF .. WT_DST_OU
PARAM_ROWS = ("kind", "row", "t_start", "t_end", "a", "b", "c")
STATE_ROWS = ("value", "x", "n_eval", "n_draw")
ROWS = (1, 2, 3, 5, 7, 8, 9)                              # the boundary rows a slot may target
# an unused slot: kind off (its row is never written)
OFF_ROW = np.array([0.0, 1.0, 0.0, np.inf, 0.0, 0.0, 0.0])

Value = Union[float, int, np.ndarray]


def row_index(row) -> np.ndarray:
    """Boundary rows given by ``BoundaryConditions`` field names or indices -> float64 codes (the library checks them)."""
    return _program.codes(row, params.BOUNDARY_FIELDS, "boundary row")


@dataclass
class Disturbance:
    """One slot: ``kind`` ("step", "ramp", "sine", "ou" or "off") moves boundary ``row`` (a field name such as
    "inlet_temperature", or its index) within t_start <= t < t_end.  ``a``, ``b``, ``c`` are the kind's parameters
    (include/wtphys.h): STEP offset a; RAMP a + b (t - t_start), held after the window; SINE a sin(2 pi (t - t_start)
    / b + c); OU stationary sigma a and time constant b [s].  Every numeric field takes a scalar or an (N,) array."""

    row: Union[str, int]
    kind: str = "off"
    t_start: Value = 0.0
    t_end: Value = np.inf
    a: Value = 0.0
    b: Value = 0.0
    c: Value = 0.0

    @classmethod
    def step(cls, row, value, start=0.0, end=np.inf) -> "Disturbance":
        """``value`` added to the row for start <= t < end (a step change in the source)."""
        return cls(row, "step", start, end, value)

    @classmethod
    def ramp(cls, row, rate, start=0.0, end=np.inf, offset=0.0) -> "Disturbance":
        """``offset + rate (t - start)`` from ``start`` on, held at its value at ``end`` (stock drift)."""
        return cls(row, "ramp", start, end, offset, rate)

    @classmethod
    def sine(cls, row, amplitude, period, phase=0.0, start=0.0, end=np.inf) -> "Disturbance":
        """``amplitude sin(2 pi (t - start) / period + phase)`` (a diurnal swing: period 86400 s)."""
        return cls(row, "sine", start, end, amplitude, period, phase)

    @classmethod
    def ou(cls, row, sigma, tau, start=0.0, end=np.inf) -> "Disturbance":
        """Ornstein-Uhlenbeck wandering with stationary standard deviation ``sigma`` and time constant ``tau`` [s]."""
        return cls(row, "ou", start, end, sigma, tau)


@dataclass
class DisturbanceState:
    """``ReactorEnsemble.disturbance_state()``: slot fields (4, N), ``base`` (10, N), ``t_prev`` (N,), float64."""

    value: np.ndarray          # the offset d of the last evaluation
    x: np.ndarray              # the OU state
    n_eval: np.ndarray         # evaluations, the one at set time included
    n_draw: np.ndarray         # normal deviates drawn
    base: np.ndarray           # the boundary the offsets are added to
    t_prev: np.ndarray         # ReactorState.time of the last evaluation

    @classmethod
    def from_block(cls, state: np.ndarray, base: np.ndarray, t_prev: np.ndarray) -> "DisturbanceState":
        """From a [SLOTS][WT_NDS][N] state block, a [WT_NB][N] base and a [N] t_prev."""
        return cls(*(np.array(state[:, k]) for k in range(NDS)), np.array(base), np.array(t_prev))


def slot_rows(d: Disturbance, n: int, name: str = "disturbance") -> np.ndarray:
    """(ND, N) rows of one slot."""
    if not isinstance(d, Disturbance):
        raise TypeError(f"{name}: expected a Disturbance, got {type(d).__name__}")
    return _program.field_rows(d, PARAM_ROWS, n, name, kind=_program.codes(d.kind, KINDS, "kind"), row=row_index(d.row))


def disturbance_block(n_reactors: int, *disturbances: Disturbance) -> np.ndarray:
    """The [WT_DST_SLOTS][WT_ND][N] float64 block of ``wt_ensemble_disturb_set``, checked by the library: slot k holds
    disturbance k, the slots after the last one :data:`OFF_ROW`."""
    return _program.slot_block(disturbances, int(n_reactors), SLOTS, "disturbance", slot_rows, np.repeat(OFF_ROW[:, None], int(n_reactors), axis=1),
                               _native.WT_PROG_DISTURB)
