"""Per-reactor anomaly detector programs that run on the device at every PLC scan (include/wtphys.h,
``wt_ensemble_detect_*``): the change-detection statistic an intrusion- or fault-detection study evaluates.

A program has up to four slots.  A slot keeps a statistic of the residual of one sensor reading -- the scan's image
copy, after any injection program, or the instrument's own field reading -- against a constant, a second reading or
its own tracked baseline: a two-sided CUSUM, an EWMA chart or a flat-line (replay) timer.  Its alarm stands while the
statistic exceeds the slot's limit, and every scan is counted against the reactor's ground-truth attack window.  With
one reactor per threshold an ensemble is a whole ROC curve in one call.  This module builds and checks the parameter
block and unpacks the state; the evaluation itself runs in ``csrc/wt_det.hpp``.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional, Union

import numpy as np

from . import _native
from ._program import SENSOR_NAMES, codes, field_rows, slot_block

SLOTS, NK, NKS, NKR = 4, 12, 16, 2       # WT_DET_SLOTS, WT_NK, WT_NKS, WT_NKR
PARAM_ROWS = ("kind", "sensor", "source", "ref", "ref_arg", "ref_source", "mu", "sigma", "slack", "limit", "t_arm", "on_bad")
STATE_ROWS = ("gp", "gn", "baseline", "x_prev", "stat", "stat_max", "alarm", "n_eval", "n_bad", "n_alarm", "n_raise",
              "t_first", "t_detect", "n_tp", "n_fp", "n_fn")
LABEL_ROWS = ("label_start", "label_end")
KINDS = ("off", "cusum", "ewma", "flatline")
SOURCES = ("image", "field")
REFS = ("const", "sensor", "track")
ON_BAD = ("hold", "alarm")
DEFAULT_SLACK = (0.0, 0.5, 0.2, 0.0)     # per kind: CUSUM k = 0.5 sigma, EWMA lambda = 0.2, FLATLINE eps = 0

Value = Union[float, int, str, np.ndarray]


@dataclass
class Detector:
    """One slot.  ``sensor``: a name of :data:`SENSOR_NAMES` or its index; ``kind``: "cusum", "ewma" or "flatline"
    (or "off"); ``limit``: the threshold on the statistic (FLATLINE: seconds without a change).  The residual is
    z = ((x - base) - mu) / sigma with ``ref`` naming the base: "const" (``ref_value``), "track" (the slot's own
    first-order baseline with time constant ``tau`` seconds) or the name of a second sensor, read from ``ref_source``.
    ``slack``: CUSUM k >= 0, EWMA lambda in (0, 1], FLATLINE eps >= 0 in the sensor's units (default per kind: 0.5,
    0.2, 0).  ``source``: "image" (the scan's copy after any injection program) or "field" (the instrument's own
    reading); ``t_arm``: the slot is skipped while t < t_arm; ``on_bad``: "hold" (a NaN or faulted reading changes
    nothing but the count) or "alarm" (it raises the alarm).  Every field takes a scalar or an (N,) array."""

    sensor: Value
    kind: Value
    limit: Value
    slack: Optional[Value] = None
    sigma: Value = 1.0
    mu: Value = 0.0
    ref: Value = "const"
    ref_value: Value = 0.0
    tau: Optional[Value] = None
    source: Value = "image"
    ref_source: Value = "image"
    t_arm: Value = -np.inf
    on_bad: Value = "hold"


@dataclass
class DetectorState:
    """``ReactorEnsemble.detector_state()``: slot fields (SLOTS, N), ``t_prev`` and the label (N,), float64."""

    gp: np.ndarray             # CUSUM upper arm, EWMA value, FLATLINE seconds without a change
    gn: np.ndarray             # CUSUM lower arm
    baseline: np.ndarray       # TRACK reference (NaN: no good reading yet)
    x_prev: np.ndarray         # last good reading (NaN: none)
    stat: np.ndarray
    stat_max: np.ndarray
    alarm: np.ndarray
    n_eval: np.ndarray         # scans evaluated (armed, reactor stepped)
    n_bad: np.ndarray          # of them with a NaN or faulted reading
    n_alarm: np.ndarray        # scans in alarm
    n_raise: np.ndarray        # alarm rising edges
    t_first: np.ndarray        # loop time of the first alarm scan (NaN: never)
    t_detect: np.ndarray       # loop time of the first alarm scan at or after label_start (NaN: never)
    n_tp: np.ndarray           # alarm scans inside the attack window
    n_fp: np.ndarray           # alarm scans outside it
    n_fn: np.ndarray           # silent scans inside it
    t_prev: np.ndarray
    label_start: Optional[np.ndarray] = None
    label_end: Optional[np.ndarray] = None

    @classmethod
    def from_block(cls, slot_block: np.ndarray, t_prev: np.ndarray, labels: Optional[np.ndarray] = None) -> "DetectorState":
        """From a [WT_DET_SLOTS][WT_NKS][N] block, a [N] t_prev and, if known, the [WT_NKR][N] label block."""
        lab = (None, None) if labels is None else (np.array(labels[0]), np.array(labels[1]))
        return cls(*(np.array(slot_block[:, k]) for k in range(NKS)), np.array(t_prev), *lab)

    def block(self):
        """The (SLOTS, NKS, N) block and t_prev again."""
        return np.stack([getattr(self, k) for k in STATE_ROWS], axis=1), self.t_prev

    def rates(self):
        """Per slot and reactor, (SLOTS, N) each: ``tpr`` = n_tp / (n_tp + n_fn), ``fpr`` = n_fp / (n_eval - n_tp -
        n_fn) and ``delay`` = t_detect - label_start; NaN where undefined (no scan inside / outside the window, no
        detection, no label)."""
        pos = self.n_tp + self.n_fn
        neg = self.n_eval - pos
        with np.errstate(invalid="ignore", divide="ignore"):
            tpr = np.where(pos > 0, self.n_tp / pos, np.nan)
            fpr = np.where(neg > 0, self.n_fp / neg, np.nan)
            if self.label_start is None:
                delay = np.full_like(self.t_detect, np.nan)
            else:
                delay = np.where(np.isfinite(self.label_start), self.t_detect - self.label_start, np.nan)
        return tpr, fpr, delay


def _ref_rows(det: Detector, name: str):
    """``ref`` (names) -> the ref code and ref_arg rows, scalars or arrays."""
    names = np.asarray(det.ref)
    if names.dtype.kind not in "US":
        raise ValueError(f"{name}.ref: expected 'const', 'track' or a sensor name, got {det.ref!r}")
    bad = [str(s) for s in names.ravel() if str(s) not in ("const", "track") + SENSOR_NAMES]
    if bad:
        raise ValueError(f"unknown ref {bad[0]!r}: 'const', 'track' or one of {SENSOR_NAMES}")
    is_const, is_track = names == "const", names == "track"
    if is_track.any() and det.tau is None:
        raise ValueError(f"{name}: a 'track' reference needs tau")
    index = np.vectorize(lambda s: float(SENSOR_NAMES.index(str(s))) if str(s) in SENSOR_NAMES else 0.0, otypes=[np.float64])(names)
    code = np.where(is_const, 0.0, np.where(is_track, 2.0, 1.0))
    tau = 0.0 if det.tau is None else np.asarray(det.tau, dtype=np.float64)
    arg = np.where(is_const, np.asarray(det.ref_value, dtype=np.float64), np.where(is_track, tau, index))
    return code, arg


def slot_rows(det: Detector, n: int, name: str = "detector") -> np.ndarray:
    """(NK, N) rows of one slot."""
    if not isinstance(det, Detector):
        raise TypeError(f"{name}: expected a Detector, got {type(det).__name__}")
    kind = codes(det.kind, KINDS, "kind")
    ref, ref_arg = _ref_rows(det, name)
    slack = det.slack
    if slack is None:     # a kind code out of range is refused with the block
        slack = np.asarray(DEFAULT_SLACK)[np.clip(np.nan_to_num(kind), 0, len(KINDS) - 1).astype(np.int64)]
    return field_rows(det, PARAM_ROWS, n, name, kind=kind, sensor=codes(det.sensor, SENSOR_NAMES, "sensor"),
                      source=codes(det.source, SOURCES, "source"), ref=ref, ref_arg=ref_arg,
                      ref_source=codes(det.ref_source, SOURCES, "ref_source"), slack=slack,
                      on_bad=codes(det.on_bad, ON_BAD, "on_bad"))


def detector_block(n_reactors: int, *detectors: Detector) -> np.ndarray:
    """The [WT_DET_SLOTS][WT_NK][N] float64 block of ``wt_ensemble_detect_set``, checked by the library: slot k is the
    k-th detector, the slots after the last are off."""
    n = int(n_reactors)
    return slot_block(detectors, n, SLOTS, "detector", slot_rows, np.zeros((NK, n)), _native.WT_PROG_DETECT)


def label_block(n_reactors: int, attack=None) -> np.ndarray:
    """The [WT_NKR][N] float64 label block: ``attack`` = (start, end), scalars or (N,) arrays; None: never attacked
    (+inf, +inf).  The set call checks it."""
    n = int(n_reactors)
    start, end = (np.inf, np.inf) if attack is None else attack
    try:
        return np.ascontiguousarray(np.stack([np.broadcast_to(np.asarray(start, dtype=np.float64), (n,)),
                                              np.broadcast_to(np.asarray(end, dtype=np.float64), (n,))]))
    except ValueError:
        raise ValueError(f"attack: expected (start, end) of scalars or ({n},) values") from None
