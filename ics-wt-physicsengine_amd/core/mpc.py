"""Per-reactor model predictive controllers that run on the device at the PLC scans (include/wtphys.h,
``wt_ensemble_mpc_*``).

Dynamic matrix control (DMC) on a step-response model: the controller keeps a prediction of the reading over the next
64 controller periods, corrects it by the difference between reading and prediction (the bias feedback that takes the
place of a PI's integral), and moves its output by the dot product of a gain row with the predicted errors.  The dead
time of sample lines, pipes and wires is inside the model, where a PI loop can only be detuned until it survives it.
One controller per dosing loop, with the loop indices of :mod:`.control`: loop 0 doses chlorine (holding words 2-3),
loop 1 acid (words 0-1).

This module builds the three blocks (parameters, step response, gain row) and unpacks the state; the library checks the
blocks (``wt_mpc_check``), and the controller itself runs in ``csrc/wt_mpc.hpp``.  :func:`fopdt_step` and
:func:`dmc_gain` produce a model and a gain row on the host, in plain numpy: they are input data of the controller, not
part of what it computes.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional, Tuple, Union

import numpy as np

from . import _native
from ._program import SENSOR_NAMES, codes, field_rows
from .control import COMMAND_LIMIT, LOOPS

NM, NMS, H = 10, 14, 64                 # WT_NM, WT_NMS, WT_MPC_H
PARAM_ROWS = ("enable", "sensor", "setpoint", "every", "horizon", "u0", "out_min", "out_max", "du_max", "t_start")
STATE_ROWS = ("phase", "output", "count", "bias", "move", "t_exec", "ise", "iae", "dose", "n_exec", "n_held", "n_sat",
              "n_rate", "n_skipped")
PHASES = ("waiting", "running")         # the codes of ``LoopMpc.phase``

Scalar = Union[float, int, np.ndarray]


def fopdt_step(gain: float, tau: float, dead_time: float, period: float, n: int = H) -> np.ndarray:
    """Step response of a first-order lag with dead time, sampled at the controller period: entry j - 1 is
    ``gain * (1 - exp(-(j * period - dead_time) / tau))`` where ``j * period > dead_time`` and 0 before, j = 1..n."""
    if not (tau > 0 and period > 0 and dead_time >= 0):
        raise ValueError("fopdt_step: tau and period must be > 0 and dead_time >= 0")
    t = np.arange(1, int(n) + 1, dtype=np.float64) * float(period) - float(dead_time)
    return np.where(t > 0, float(gain) * (1.0 - np.exp(-np.maximum(t, 0.0) / float(tau))), 0.0)


def dmc_gain(step, horizon: int, moves: int, move_penalty: float) -> np.ndarray:
    """The DMC gain row: the first row of ``(S^T S + move_penalty I)^-1 S^T`` for the ``horizon`` x ``moves`` dynamic
    matrix ``S[i, j] = step[i - j]`` (0 above the diagonal), i.e. the first of the ``moves`` moves that minimise the
    squared predicted errors over the horizon plus ``move_penalty`` times the squared moves.  Returns (horizon,)."""
    a = np.asarray(step, dtype=np.float64)
    p, m = int(horizon), int(moves)
    if a.ndim != 1 or not 1 <= p <= len(a):
        raise ValueError(f"dmc_gain: step must be one-dimensional with at least horizon = {p} entries")
    if not 1 <= m <= p:
        raise ValueError("dmc_gain: moves must be in 1..horizon")
    if not move_penalty >= 0:
        raise ValueError("dmc_gain: move_penalty must be >= 0")
    S = np.zeros((p, m))
    for j in range(m):
        S[j:, j] = a[:p - j]
    return np.linalg.solve(S.T @ S + float(move_penalty) * np.eye(m), S.T)[0]


@dataclass
class DMCLoop:
    """One loop's controller.  The scalar fields take a scalar or an (N,) array; ``sensor`` is a name of
    :data:`SENSOR_NAMES` or its index.  ``step`` and ``gain`` are (h,) or (h, N) with h <= 64: entry i of ``step`` is the
    change of the reading i + 1 controller periods after a unit move of the output (negative for a loop that lowers its
    reading, as acid does the pH) and is continued with its last value; ``gain`` weights the predicted errors and is
    continued with zeros.  ``horizon``: entries of ``gain`` used (default: all given).  ``every``: controller period in
    scans.  ``u0``: output before the first move.  ``du_max``: largest move.  ``out_max=None`` is the actuator's command
    limit.  The controller takes the loop at the first scan whose loop time reaches ``t_start``."""

    sensor: Union[str, int, np.ndarray]
    setpoint: Scalar
    step: np.ndarray
    gain: np.ndarray
    horizon: Optional[Scalar] = None
    every: Scalar = 1
    u0: Scalar = 0.0
    out_min: Scalar = 0.0
    out_max: Optional[Scalar] = None
    du_max: Scalar = float("inf")
    t_start: Scalar = 0.0
    enable: Scalar = 1

    @classmethod
    def from_step_response(cls, sensor, setpoint, step, horizon: Optional[int] = None, moves: int = 1,
                           move_penalty: float = 0.0, **kwargs) -> "DMCLoop":
        """A controller for the (h,) step response ``step``, its gain row from :func:`dmc_gain` over ``horizon``
        entries (default: all of them)."""
        a = np.asarray(step, dtype=np.float64)
        p = len(a) if horizon is None else int(horizon)
        return cls(sensor, setpoint, a, dmc_gain(a, p, moves, move_penalty), horizon=p, **kwargs)

    @classmethod
    def from_fopdt(cls, sensor, setpoint, gain: float, tau: float, dead_time: float, period: float,
                   horizon: int = H, moves: int = 1, move_penalty: float = 0.0, **kwargs) -> "DMCLoop":
        """A controller for a first-order lag with dead time (:func:`fopdt_step`); ``period`` is the controller period
        in seconds: the scan interval times ``every``."""
        return cls.from_step_response(sensor, setpoint, fopdt_step(gain, tau, dead_time, period), horizon, moves,
                                      move_penalty, **kwargs)


@dataclass
class LoopMpc:
    """State of one loop's controller, (N,) float64 each (codes and counts are whole numbers)."""

    phase: np.ndarray          # 0 waiting, 1 running
    output: np.ndarray
    count: np.ndarray          # scans since the last due one
    bias: np.ndarray           # reading minus prediction at the last execution
    move: np.ndarray           # the last move as applied
    t_exec: np.ndarray         # loop time of the last execution
    ise: np.ndarray            # integral of e^2 dt over the executions
    iae: np.ndarray            # integral of |e| dt
    dose: np.ndarray           # integral of the output dt
    n_exec: np.ndarray
    n_held: np.ndarray         # due scans without a valid reading (not finite, or a sensor fault)
    n_sat: np.ndarray          # executions whose output was clamped
    n_rate: np.ndarray         # executions whose move was clamped
    n_skipped: np.ndarray      # scans in which a relay experiment had the loop


@dataclass
class MpcState:
    """``ReactorEnsemble.mpc_state()``: one :class:`LoopMpc` per loop, indexed by reactor."""

    chlorine: LoopMpc
    acid: LoopMpc

    @classmethod
    def from_block(cls, block: np.ndarray) -> "MpcState":
        """From a [WT_MPC_LOOPS][WT_NMS][N] block."""
        return cls(*(LoopMpc(*(np.array(block[l, k]) for k in range(NMS))) for l in range(len(LOOPS))))

    def block(self) -> np.ndarray:
        """The (2, NMS, N) block again."""
        return np.stack([np.stack([getattr(getattr(self, loop), k) for k in STATE_ROWS]) for loop in LOOPS])


def _off_rows(n: int) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    rows = np.zeros((NM, n))
    for k, v in (("every", 1.0), ("horizon", 1.0), ("du_max", np.inf)):
        rows[PARAM_ROWS.index(k)] = v
    return rows, np.zeros((H, n)), np.zeros((H, n))


def _model_rows(a, n: int, name: str, pad_last: bool) -> Tuple[np.ndarray, int]:
    """(H, n) rows of a (h,) or (h, n) model array, and h."""
    a = np.asarray(a, dtype=np.float64)
    if a.ndim == 1:
        a = np.broadcast_to(a[:, None], (len(a), n))
    if a.ndim != 2 or a.shape[1] != n or not 1 <= a.shape[0] <= H:
        raise ValueError(f"{name}: expected (h,) or (h, {n}) values with 1 <= h <= {H}, got shape {np.shape(a)}")
    h = a.shape[0]
    rows = np.zeros((H, n))
    rows[:h] = a
    if pad_last:
        rows[h:] = a[-1]
    return rows, h


def loop_rows(loop: Optional[DMCLoop], name: str, n: int) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """(NM, N) parameter rows and (H, N) step and gain rows of one loop; ``None`` or ``False`` is a disabled loop."""
    if loop is None or loop is False:
        return _off_rows(n)
    if not isinstance(loop, DMCLoop):
        raise TypeError(f"{name}: expected a DMCLoop, got {type(loop).__name__}")
    step, _ = _model_rows(loop.step, n, f"{name}.step", True)
    gain, h = _model_rows(loop.gain, n, f"{name}.gain", False)
    rows = field_rows(loop, PARAM_ROWS, n, name, sensor=codes(loop.sensor, SENSOR_NAMES, "sensor"),
                      horizon=h if loop.horizon is None else loop.horizon,
                      out_max=COMMAND_LIMIT[name] if loop.out_max is None else loop.out_max)
    return rows, step, gain


def mpc_block(n_reactors: int, chlorine: Optional[DMCLoop] = None,
              acid: Optional[DMCLoop] = None) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """The [WT_MPC_LOOPS][WT_NM][N] parameter block and the [WT_MPC_LOOPS][WT_MPC_H][N] step and gain blocks of
    ``wt_ensemble_mpc_set``, checked by the library."""
    n = int(n_reactors)
    loops = [loop_rows(chlorine, "chlorine", n), loop_rows(acid, "acid", n)]
    params, step, gain = (np.ascontiguousarray(np.stack([rows[k] for rows in loops])) for k in range(3))
    try:
        _native.check(_native.lib().wt_mpc_check(n, _native.dptr(params), _native.dptr(step), _native.dptr(gain)))
    except _native.WtError as e:   # WT_E_ARG is the only error it returns
        raise ValueError(e.message) from None
    return params, step, gain
