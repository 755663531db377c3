"""The wire program (include/wtphys.h, ``wt_ensemble_wire_*``): a stage's PLC inputs wired to another stage's
instruments of the same treatment train, inside the step call.

On top of a train program, with plant I/O on.  A real plant doses chlorine at the rapid mix and trims on the residual
analyser at the contact tank's outlet: per reactor and input slot (the seven sensors, suite order) the program says
whether the slot reads the reactor's own instrument (the default) or sensor ``source`` of stage ``from_stage`` of the
same train.  At every PLC scan, before everything else in the scan, the wired slots of a reactor's controller-side
copy of the readings get the source instrument's reading and fault code; the injection program, the input image, the
PI loops, the IMAGE slots of alarms and detectors and the trend recorder's image tags then see the wired value.
FIELD slots, ``sensor_readings()`` and the sensor history stay the reactor's own instrument.  A source that did not
take the outer step reads NaN with fault 1 (open circuit).  This module builds the parameter block and unpacks the
state; the library checks the block, and the routing itself runs in ``csrc/wt_wir.hpp``.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional

import numpy as np

from . import _native
from ._program import SENSOR_NAMES, codes

NSENS, NW, NWS = len(SENSOR_NAMES), 2, 2                  # WT_NSENS, WT_NW, WT_NWS
PARAM_ROWS = ("stage", "sensor")
STATE_ROWS = ("n_routed", "n_lost")
OWN = -1                                                  # stage code of a slot on the reactor's own instrument


@dataclass
class Wire:
    """One cable, the same in every selected train: input slot ``sensor`` of stage ``to_stage`` reads sensor ``source``
    (default: the same sensor) of stage ``from_stage``.  ``sensor`` and ``source``: names of :data:`SENSOR_NAMES` or
    indices.  ``from_stage`` may be ``to_stage`` itself with another ``source``.  ``trains``: a boolean mask or an
    index selection over the N / length trains (default: all)."""

    sensor: object
    to_stage: int
    from_stage: int
    source: object = None
    trains: Optional[object] = None


def _slot(value, what: str) -> float:
    a = codes(value, SENSOR_NAMES, what)
    if a.ndim != 0:
        raise ValueError(f"wire.{what}: expected one sensor name or index, got shape {a.shape}")
    return float(a)


def check(length: int, block: np.ndarray) -> None:
    """The checks ``wt_ensemble_wire_set`` makes on a [WT_NSENS][WT_NW][N] block for trains of ``length`` stages;
    ``ValueError`` names the first one that fails."""
    try:
        _native.check(_native.lib().wt_wire_check(int(length), block.shape[-1], _native.dptr(block)))
    except _native.WtError as e:   # WT_E_ARG is the only error it returns
        raise ValueError(e.message) from None


def wire_block(n_reactors: int, length: int, *wires: Wire) -> np.ndarray:
    """The [WT_NSENS][WT_NW][N] float64 block of ``wt_ensemble_wire_set`` for N / ``length`` trains, checked by the
    library: every slot on the reactor's own instrument, then the ``wires`` in order (a later one wins a slot)."""
    n, length = int(n_reactors), int(length)
    if length < 1 or n % length:
        raise ValueError("n_reactors must be a multiple of length (an ensemble holds whole trains)")
    block = np.empty((NSENS, NW, n))
    block[:, 0] = OWN
    block[:, 1] = np.arange(NSENS, dtype=np.float64)[:, None]
    first = np.arange(0, n, length)
    for k, w in enumerate(wires):
        slot = _slot(w.sensor, "sensor")
        if slot not in range(NSENS):
            raise ValueError(f"wire {k}: sensor must be one of {SENSOR_NAMES} or an index in 0..{NSENS - 1}")
        if not (isinstance(w.to_stage, (int, np.integer)) and 0 <= w.to_stage < length):
            raise ValueError(f"wire {k}: to_stage must be a stage of the train, 0..{length - 1}")
        try:
            at = first if w.trains is None else first[np.asarray(w.trains)]
        except IndexError:
            raise ValueError(f"wire {k}: trains must select among the {n // length} trains") from None
        block[int(slot), 0, at + int(w.to_stage)] = float(w.from_stage)
        block[int(slot), 1, at + int(w.to_stage)] = slot if w.source is None else _slot(w.source, "source")
    check(length, block)
    return block


@dataclass
class WireState:
    """``ReactorEnsemble.wire_state()``: (7, N) float64 each, slot by slot in sensor order."""

    n_routed: np.ndarray       # scans that delivered the source's reading into this slot
    n_lost: np.ndarray         # scans that found the source stopped: the slot read NaN with fault 1

    @classmethod
    def from_block(cls, state: np.ndarray) -> "WireState":
        """From a [WT_NSENS][WT_NWS][N] state block."""
        return cls(np.array(state[:, 0]), np.array(state[:, 1]))

    def block(self) -> np.ndarray:
        """The (NSENS, NWS, N) block again."""
        return np.stack([self.n_routed, self.n_lost], axis=1)
