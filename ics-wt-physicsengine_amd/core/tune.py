"""Per-reactor relay autotune programs that run on the device at every PLC scan (include/wtphys.h,
``wt_ensemble_tune_*``).

The standard commissioning experiment (Astrom-Hagglund): a relay with hysteresis around the setpoint replaces the
controller, the loop settles into its limit cycle, and the cycle's period Pu and amplitude a give the ultimate gain
``Ku = 4 d / (pi sqrt(a^2 - eps^2))``, to which a tuning rule is applied.  One tuner per PI loop, with the loop indices
of :mod:`.control`: loop 0 doses chlorine (holding words 2-3), loop 1 acid (words 0-1).  This module only builds the
parameter block and unpacks the state; the library checks the block (``wt_program_check``), and the experiment itself runs
in ``csrc/wt_tun.hpp``.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional, Tuple, Union

import numpy as np

from . import _native
from ._program import SENSOR_NAMES, check, codes, field_rows
from .control import COMMAND_LIMIT, LOOPS

NU, NUS = 14, 20                        # WT_NU, WT_NUS
PARAM_ROWS = ("enable", "sensor", "direction", "setpoint", "bias", "amplitude", "hysteresis", "t_start", "t_max", "settle",
              "cycles", "kp_factor", "ti_factor", "commission")
STATE_ROWS = ("phase", "relay", "output", "n_up", "t_up", "e_max", "e_min", "sum_period", "sum_amp", "n_cycles", "period",
              "amplitude", "ku", "kp", "ki", "t_begin", "t_done", "n_exec", "n_held", "commissioned")
PHASES = ("waiting", "running", "done", "failed")     # the codes of ``LoopTune.phase``
# (kp_factor, ti_factor): kp = kp_factor * Ku, ki = kp / (ti_factor * Pu); ti_factor 0: ki = 0
TUNE_RULES = {"ziegler_nichols_pi": (0.45, 1.0 / 1.2), "tyreus_luyben_pi": (1.0 / 3.2, 2.2), "p_only": (0.5, 0.0)}

Scalar = Union[float, int, np.ndarray]


@dataclass
class RelayTune:
    """One loop's relay experiment; every field but ``rule`` takes a scalar or an (N,) array.  ``sensor`` is a name of
    :data:`SENSOR_NAMES` or its index.  The relay's output is ``bias + amplitude`` while the error
    ``direction * (setpoint - reading)`` is above ``hysteresis`` (and until it falls below ``-hysteresis``), else
    ``bias - amplitude``; both must lie inside the loop's command range (:data:`COMMAND_LIMIT`).  The experiment begins
    at the first scan whose loop time reaches ``start``, discards ``settle`` whole cycles, measures ``cycles`` and
    fails ``timeout`` seconds after it began.  ``rule``: a name of :data:`TUNE_RULES` or a ``(kp_factor, ti_factor)``
    pair.  ``commission``: hand the loop to the PI program (:meth:`ReactorEnsemble.enable_control`) with the gains
    found, its integral set so that the output continues from ``bias``."""

    sensor: Union[str, int, np.ndarray]
    setpoint: Scalar
    amplitude: Scalar
    bias: Scalar
    hysteresis: Scalar = 0.0
    direction: Scalar = 1
    start: Scalar = 0.0
    timeout: Scalar = float("inf")
    settle: Scalar = 2
    cycles: Scalar = 4
    rule: Union[str, Tuple[Scalar, Scalar]] = "ziegler_nichols_pi"
    commission: Scalar = False
    enable: Scalar = 1


@dataclass
class LoopTune:
    """State of one loop's tuner, (N,) float64 each (codes and counts are whole numbers)."""

    phase: np.ndarray          # 0 waiting, 1 running, 2 done, 3 failed (timed out, or amplitude <= hysteresis)
    relay: np.ndarray          # -1, 0 (not yet decided) or +1
    output: np.ndarray
    n_up: np.ndarray           # up-switches so far
    t_up: np.ndarray           # loop time of the last one
    e_max: np.ndarray          # extremes of the error since the last up-switch
    e_min: np.ndarray
    sum_period: np.ndarray
    sum_amp: np.ndarray
    n_cycles: np.ndarray       # cycles measured
    period: np.ndarray         # Pu [s]
    amplitude: np.ndarray      # a
    ku: np.ndarray
    kp: np.ndarray
    ki: np.ndarray             # per second
    t_begin: np.ndarray
    t_done: np.ndarray
    n_exec: np.ndarray
    n_held: np.ndarray         # running scans without a valid reading (not finite, or a sensor fault)
    commissioned: np.ndarray   # 1: the gains were written into the PI loop's record


@dataclass
class TunerState:
    """``ReactorEnsemble.tuner_state()``: one :class:`LoopTune` per loop, indexed by reactor."""

    chlorine: LoopTune
    acid: LoopTune

    @classmethod
    def from_block(cls, block: np.ndarray) -> "TunerState":
        """From a [WT_TUN_LOOPS][WT_NUS][N] block."""
        return cls(*(LoopTune(*(np.array(block[l, k]) for k in range(NUS))) for l in range(len(LOOPS))))

    def block(self) -> np.ndarray:
        """The (2, NUS, N) block again."""
        return np.stack([np.stack([getattr(getattr(self, loop), k) for k in STATE_ROWS]) for loop in LOOPS])


def _rule_factors(rule, name: str):
    if isinstance(rule, str):
        if rule not in TUNE_RULES:
            raise ValueError(f"unknown rule {rule!r}: one of {tuple(TUNE_RULES)}")
        return TUNE_RULES[rule]
    try:
        kp_factor, ti_factor = rule
    except (TypeError, ValueError):
        raise ValueError(f"{name}.rule: expected a name of TUNE_RULES or a (kp_factor, ti_factor) pair") from None
    return kp_factor, ti_factor


def loop_rows(tune: Optional[RelayTune], name: str, n: int) -> np.ndarray:
    """(NU, N) rows of one loop; ``None`` or ``False`` is a disabled loop."""
    if tune is None or tune is False:
        return np.zeros((NU, n))
    if not isinstance(tune, RelayTune):
        raise TypeError(f"{name}: expected a RelayTune, got {type(tune).__name__}")
    kp_factor, ti_factor = _rule_factors(tune.rule, name)
    return field_rows(tune, PARAM_ROWS, n, name, sensor=codes(tune.sensor, SENSOR_NAMES, "sensor"), t_start=tune.start,
                      t_max=tune.timeout, kp_factor=kp_factor, ti_factor=ti_factor)


def tune_block(n_reactors: int, chlorine: Optional[RelayTune] = None, acid: Optional[RelayTune] = None) -> np.ndarray:
    """The [WT_TUN_LOOPS][WT_NU][N] float64 parameter block of ``wt_ensemble_tune_set``, checked by the library."""
    n = int(n_reactors)
    block = np.ascontiguousarray(np.stack([loop_rows(chlorine, "chlorine", n), loop_rows(acid, "acid", n)]))
    check(_native.WT_PROG_TUNE, block)
    return block
