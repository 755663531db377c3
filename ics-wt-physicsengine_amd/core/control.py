"""Per-reactor PI dosing programs that run on the device at every PLC scan (include/wtphys.h,
``wt_ensemble_control_*``).

They stand in for the master side of the reference's loop (``__main__.py:227-271``): what a Modbus master computes
from the input image and writes into the holding registers between two scans.  Loop 0 doses chlorine (holding words
2-3), loop 1 acid (words 0-1).  This module only builds and checks the parameter block and unpacks the state; the
update itself runs in ``csrc/wt_ctl.hpp``.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional, Union

import numpy as np

from . import _native
from ._program import SENSOR_NAMES, check, codes, field_rows

LOOPS = ("chlorine", "acid")            # loop index order of the blocks
NC, NCS = 9, 8                          # WT_NC, WT_NCS
PARAM_ROWS = ("enable", "sensor", "direction", "setpoint", "kp", "ki", "bias", "out_min", "out_max")
STATE_ROWS = ("integral", "output", "ise", "iae", "dose", "n_exec", "n_held", "n_sat")
HOLDING_WORD = {"chlorine": 2, "acid": 0}    # first holding word of each loop's float32 output
COMMAND_LIMIT = {"chlorine": 1.0, "acid": 2.0}   # validate_flow_rate's maxima (__main__.py:57-63, :236-242)

Scalar = Union[float, int, np.ndarray]


@dataclass
class PILoop:
    """One PI loop's parameters; every field takes a scalar or an (N,) array.  ``sensor`` is a name of
    :data:`SENSOR_NAMES` or its index.  ``direction`` +1 (direct: output rises while the reading is below the
    setpoint) or -1 (reverse).  ``ki`` is per second.  ``out_max=None`` is the actuator's command limit."""

    sensor: Union[str, int, np.ndarray]
    setpoint: Scalar
    kp: Scalar = 0.0
    ki: Scalar = 0.0
    direction: Scalar = 1
    bias: Scalar = 0.0
    out_min: Scalar = 0.0
    out_max: Optional[Scalar] = None
    enable: Scalar = 1


@dataclass
class LoopState:
    """State of one loop, (N,) float64 each (counts are whole numbers)."""

    integral: np.ndarray
    output: np.ndarray
    ise: np.ndarray        # integral of e^2 dt over the executed scans
    iae: np.ndarray        # integral of |e| dt
    dose: np.ndarray       # integral of the output dt
    n_exec: np.ndarray
    n_held: np.ndarray     # scans without a valid reading (not finite, or a sensor fault)
    n_sat: np.ndarray      # executed scans whose output was clamped


@dataclass
class ControlState:
    """``ReactorEnsemble.control_state()``: one :class:`LoopState` per loop, indexed by reactor."""

    chlorine: LoopState
    acid: LoopState

    @classmethod
    def from_block(cls, block: np.ndarray) -> "ControlState":
        """From a [WT_CTL_LOOPS][WT_NCS][N] block."""
        return cls(*(LoopState(*(np.array(block[l, k]) for k in range(NCS))) for l in range(len(LOOPS))))

    def block(self) -> np.ndarray:
        """The (2, NCS, N) block again."""
        return np.stack([np.stack([getattr(getattr(self, loop), k) for k in STATE_ROWS]) for loop in LOOPS])


def _off_rows(n: int) -> np.ndarray:
    rows = np.zeros((NC, n))
    rows[PARAM_ROWS.index("direction")] = 1.0
    return rows


def loop_rows(loop: Optional[PILoop], name: str, n: int) -> np.ndarray:
    """(NC, N) rows of one loop; ``None`` or ``False`` is a disabled loop."""
    if loop is None or loop is False:
        return _off_rows(n)
    if not isinstance(loop, PILoop):
        raise TypeError(f"{name}: expected a PILoop, got {type(loop).__name__}")
    return field_rows(loop, PARAM_ROWS, n, name, sensor=codes(loop.sensor, SENSOR_NAMES, "sensor"),
                      out_max=COMMAND_LIMIT[name] if loop.out_max is None else loop.out_max)


def control_block(n_reactors: int, chlorine: Optional[PILoop] = None, acid: Optional[PILoop] = None) -> np.ndarray:
    """The [WT_CTL_LOOPS][WT_NC][N] float64 parameter block of ``wt_ensemble_control_enable``, checked by the
    library."""
    n = int(n_reactors)
    block = np.ascontiguousarray(np.stack([loop_rows(chlorine, "chlorine", n), loop_rows(acid, "acid", n)]))
    check(_native.WT_PROG_CONTROL, block)
    return block
