"""CPU checks of the per-reactor score programs: the restatement (score_ref.py) against hand-worked answers, the
block of ``score_block`` with the library's checks, the fan's bin rule at its edges, ``ScoreCurve.quantiles`` on a
hand-built fan, and the C ABI symbols."""
import importlib
import os
import re

import numpy as np
import pytest

import score_ref as SR
from program_helpers import refused_as_checked
from score_ref import ScoreRef, fan_bin

INF, NAN = np.inf, np.nan
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def scr(native):
    return importlib.import_module("ics-wt-physicsengine_amd.core.score")


def _block(*slots, n=1):
    """(4, 8, n) from (kind, quantity, reduce, zone, lo, hi, t_start, t_end) tuples; the rest off."""
    p = np.zeros((4, 8, n))
    p[:, 3], p[:, 4], p[:, 5], p[:, 6], p[:, 7] = -1.0, -INF, INF, -INF, INF
    for k, s in enumerate(slots):
        p[k] = np.asarray(s, dtype=np.float64)[:, None]
    return p


def _run(p, cl, times, stepped=None, t0=0.0, pH=None, T=None, **curve):
    """One reactor: chlorine rows (K, n) at ``times``; pH and temperature default to constants."""
    cl = np.asarray(cl, dtype=np.float64)
    ref = ScoreRef(p, [t0], **curve)
    for k, t in enumerate(times):
        x = cl[k][None, :]
        ref.step(x * 0 + 7.0 if pH is None else np.asarray(pH[k], dtype=np.float64)[None, :], x,
                 x * 0 + 20.0 if T is None else np.asarray(T[k], dtype=np.float64)[None, :], np.array([t]),
                 [True if stepped is None else stepped[k]])
    return ref


def _row(ref, slot, row):
    return ref.st[slot, row, 0]


def test_band_crossed_twice():
    """Outlet chlorine 0.5, 0.1, 0.3, 0.9, 0.15, 0.4 at t = 10..60 against [0.2, 0.8]: below at 20 and 50, above at 40
    (the run 40..50 is one excursion: it goes from above straight to below)."""
    p = _block((1, 1, 0, -1, 0.2, 0.8, -INF, INF))
    v = [0.5, 0.1, 0.3, 0.9, 0.15, 0.4]
    ref = _run(p, [[9.0, x] for x in v], [10.0, 20.0, 30.0, 40.0, 50.0, 60.0], curve=8)
    assert _row(ref, 0, SR.S_N_EVAL) == 6 and _row(ref, 0, SR.S_TIME) == 60.0
    integral = 0.0
    for x in v:
        integral = integral + x * 10.0
    assert _row(ref, 0, SR.S_INTEGRAL) == integral
    assert _row(ref, 0, SR.S_T_LOW) == 20.0 and _row(ref, 0, SR.S_T_HIGH) == 10.0
    assert _row(ref, 0, SR.S_AREA_LOW) == (0.2 - 0.1) * 10.0 + (0.2 - 0.15) * 10.0
    assert _row(ref, 0, SR.S_AREA_HIGH) == (0.9 - 0.8) * 10.0
    assert _row(ref, 0, SR.S_V_MIN) == 0.1 and _row(ref, 0, SR.S_V_MAX) == 0.9 and _row(ref, 0, SR.S_LAST) == 0.4
    assert _row(ref, 0, SR.S_N_EXC) == 2 and _row(ref, 0, SR.S_T_FIRST_OUT) == 20.0
    assert _row(ref, 0, SR.S_OUT) == 0 and _row(ref, 0, SR.S_RUN) == 0 and _row(ref, 0, SR.S_RUN_MAX) == 20.0
    assert ref.t_prev[0] == 60.0
    assert ref.counts[:, 0].tolist() == [[1, 0, 0], [1, 1, 0], [1, 0, 0], [1, 0, 1], [1, 1, 0], [1, 0, 0], [0, 0, 0], [0, 0, 0]]
    assert not ref.counts[:, 1:].any()
    # the off slots keep their set-time values
    assert np.all(ref.st[1:, SR.S_N_EVAL] == 0) and np.all(np.isnan(ref.st[1:, SR.S_V_MIN]))


def test_min_max_mean_and_zone_on_three_zones():
    p = _block((1, 1, 1, -1, 0.25, INF, -INF, INF),      # MIN of chlorine
               (1, 2, 2, -1, -INF, 21.0, -INF, INF),     # MAX of temperature
               (1, 0, 3, -1, 6.5, 7.5, -INF, INF),       # MEAN of pH
               (1, 1, 0, 1, 0.0, 0.45, -INF, INF))       # chlorine of zone 1
    cl = [[0.3, 0.5, 0.2], [0.6, 0.4, 0.7]]
    T = [[20.0, 22.0, 21.0], [19.0, 18.0, 20.5]]
    pH = [[7.1, 7.3, 8.3], [0.1, 0.2, 0.3]]
    ref = _run(p, cl, [5.0, 15.0], pH=pH, T=T)
    assert _row(ref, 0, SR.S_V_MIN) == 0.2 and _row(ref, 0, SR.S_LAST) == 0.4 and _row(ref, 0, SR.S_T_LOW) == 5.0
    assert _row(ref, 0, SR.S_AREA_LOW) == (0.25 - 0.2) * 5.0
    assert _row(ref, 1, SR.S_V_MAX) == 22.0 and _row(ref, 1, SR.S_LAST) == 20.5 and _row(ref, 1, SR.S_T_HIGH) == 5.0
    assert _row(ref, 1, SR.S_AREA_HIGH) == (22.0 - 21.0) * 5.0 and _row(ref, 1, SR.S_OUT) == 0
    m0, m1 = ((7.1 + 7.3) + 8.3) / 3.0, ((0.1 + 0.2) + 0.3) / 3.0      # ascending zone order
    assert _row(ref, 2, SR.S_V_MAX) == m0 and _row(ref, 2, SR.S_LAST) == m1
    assert _row(ref, 2, SR.S_T_HIGH) == 5.0 and _row(ref, 2, SR.S_T_LOW) == 10.0 and _row(ref, 2, SR.S_N_EXC) == 1
    assert _row(ref, 2, SR.S_RUN_MAX) == 15.0 and _row(ref, 2, SR.S_OUT) == 1
    assert _row(ref, 2, SR.S_INTEGRAL) == m0 * 5.0 + m1 * 10.0
    assert _row(ref, 3, SR.S_V_MAX) == 0.5 and _row(ref, 3, SR.S_LAST) == 0.4 and _row(ref, 3, SR.S_T_HIGH) == 5.0


def test_window_edges():
    """t_start <= t < t_end: the step at t_start is scored, the one at t_end is not; h is the reactor's step, also
    for the first evaluation inside the window."""
    p = _block((1, 1, 0, -1, 0.5, INF, 20.0, 40.0), (1, 1, 0, -1, 0.5, INF, 25.0, 25.0))
    ref = _run(p, [[0.1]] * 5, [10.0, 20.0, 30.0, 40.0, 50.0], curve=5)
    assert _row(ref, 0, SR.S_N_EVAL) == 2 and _row(ref, 0, SR.S_TIME) == 20.0 and _row(ref, 0, SR.S_T_LOW) == 20.0
    assert _row(ref, 0, SR.S_T_FIRST_OUT) == 20.0 and _row(ref, 0, SR.S_OUT) == 1 and _row(ref, 0, SR.S_RUN) == 20.0
    assert _row(ref, 1, SR.S_N_EVAL) == 0 and np.isnan(_row(ref, 1, SR.S_LAST))        # an empty window
    assert ref.counts[:, 0, 0].tolist() == [0, 1, 1, 0, 0] and ref.counts[:, 0, 1].tolist() == [0, 1, 1, 0, 0]
    assert ref.t_prev[0] == 50.0


def test_reactor_that_freezes_half_way():
    p = _block((1, 1, 0, -1, 0.5, INF, -INF, INF), n=2)
    ref = ScoreRef(p, [0.0, 0.0], curve=4)
    x = np.full((2, 1), 0.1)
    for k, t in enumerate([10.0, 20.0, 30.0, 40.0]):
        live = np.array([True, k < 2])
        ref.step(x, x, x, np.array([t, min(t, 20.0)]), live)
    assert ref.st[0, SR.S_N_EVAL].tolist() == [4, 2] and ref.st[0, SR.S_T_LOW].tolist() == [40.0, 20.0]
    assert ref.t_prev.tolist() == [40.0, 20.0] and ref.st[0, SR.S_RUN_MAX].tolist() == [40.0, 20.0]
    assert ref.counts[:, 0, 0].tolist() == [2, 2, 1, 1] and ref.counts[:, 0, 1].tolist() == [2, 2, 1, 1]


def test_run_takes_stepped_from_time_and_status():
    p = _block((1, 1, 0, -1, -INF, INF, -INF, INF), n=3)
    time = np.array([[10.0, 10.0, 10.0], [20.0, 10.0, 20.0], [30.0, 10.0, 20.0]])
    status = np.array([[0, 0, 0], [0, 1, 32], [0, 1, 32]], dtype=np.uint32)       # reactor 1 raised in step 2, 2 after it
    x = np.full((3, 3, 2), 0.4)
    ref = ScoreRef(p, np.zeros(3)).run(x, x, x, time, status)
    assert ref.st[0, SR.S_N_EVAL].tolist() == [3, 1, 1] and ref.t_prev.tolist() == [30.0, 10.0, 10.0]


def test_fan_bin_rule_at_its_edges():
    lo, hi, B = 0.2, 1.0, 8
    scale = B / (hi - lo)
    below = np.nextafter(lo, -INF)
    assert fan_bin([below, lo, np.nextafter(lo, INF)], lo, hi, scale, B).tolist() == [0, 1, 1]
    assert fan_bin([np.nextafter(hi, -INF), hi, 5.0], lo, hi, scale, B).tolist() == [B, B + 1, B + 1]
    assert fan_bin([0.124, 0.125, 0.95], 0.0, 1.0, 8.0, 8).tolist() == [1, 2, 8]     # an inner edge belongs to the bin above
    # the last bin's upper rounding: (v - lo) * scale may round up to B just below hi; the bin stays B
    lo, hi, B = 0.05, 1.9, 10
    scale = B / (hi - lo)
    v = np.nextafter(hi, -INF)
    assert (v - lo) * scale >= B and fan_bin([v], lo, hi, scale, B).tolist() == [B]
    # one bin: everything inside the range
    assert fan_bin([0.1, 0.4, 0.69], 0.1, 0.7, 1 / 0.6, 1).tolist() == [1, 1, 1]


def test_fan_counts_follow_the_rule():
    p = _block((1, 1, 0, -1, 0.2, 0.8, -INF, INF), n=4)
    ref = ScoreRef(p, np.zeros(4), curve=2, bins=4, fan_lo=0.0, fan_hi=1.0)
    cl = np.array([[-0.1], [0.0], [0.26], [1.0]])
    ref.step(cl, cl, cl, np.full(4, 10.0), np.array([True, True, True, False]))
    assert ref.fan[0, 0].tolist() == [1, 1, 1, 0, 0, 0] and not ref.fan[1:].any() and not ref.fan[0, 1:].any()
    assert ref.counts[0, 0].tolist() == [3, 2, 0]


def test_quantiles_on_a_hand_built_fan(scr):
    edges = scr.fan_edges([0.0] * 4, [4.0, 1.0, 1.0, 1.0], 4)
    assert edges.shape == (4, 5) and edges[0].tolist() == [0.0, 1.0, 2.0, 3.0, 4.0]
    fan = np.zeros((2, 4, 6), dtype=np.int32)
    fan[0, 0] = [0, 2, 2, 4, 2, 0]          # 10 values inside the range
    fan[1, 0] = [5, 0, 0, 0, 0, 5]          # half below, half above
    z = np.zeros((2, 4), dtype=np.int32)
    c = scr.ScoreCurve(z, z, z, fan, edges)
    q = c.quantiles([0.1, 0.5, 0.9])
    assert q.shape == (3, 2, 4)
    assert q[:, 0, 0].tolist() == [0.5, 2.25, 3.5]
    assert q[:, 1, 0].tolist() == [0.0, 0.0, 4.0]
    assert np.all(np.isnan(q[:, :, 1:]))
    with pytest.raises(ValueError, match="no fan"):
        scr.ScoreCurve(z, z, z).quantiles(0.5)


def test_block_packing(scr, wt):
    N = 3
    blk = scr.score_block(N, wt.Score("chlorine", lo=0.2, hi=[1.0, 2.0, 3.0]),
                          wt.Score("pH", 6.5, 8.5, reduce="mean", t_start=100.0),
                          wt.Score(2, hi=30.0, reduce="max", zone=1, t_end=500.0))
    assert blk.shape == (4, 8, N) and blk.flags["C_CONTIGUOUS"]
    assert np.all(blk[0, :, 1] == [1, 1, 0, -1, 0.2, 2.0, -INF, INF])
    assert np.all(blk[1, :, 0] == [1, 0, 3, -1, 6.5, 8.5, 100.0, INF])
    assert np.all(blk[2, :, 2] == [1, 2, 2, 1, -INF, 30.0, -INF, 500.0])
    assert np.all(blk[3] == scr.OFF_ROW[:, None]) and np.all(blk[3, 0] == 0)
    assert np.all(scr.score_block(1, wt.Score("temperature", kind="off"))[0, :2, 0] == [0, 2])
    with pytest.raises(ValueError, match="at most 4"):
        scr.score_block(1, *[wt.Score("pH")] * 5)
    with pytest.raises(ValueError, match="unknown quantity"):
        scr.score_block(1, wt.Score("turbidity"))
    with pytest.raises(ValueError, match="unknown reduce"):
        scr.score_block(1, wt.Score("pH", reduce="median"))
    with pytest.raises(ValueError, match="lo must be <= hi"):
        scr.score_block(1, wt.Score("pH", lo=8.0, hi=7.0))


@pytest.mark.parametrize("slot, msg", [
    ((2, 1, 0, -1, 0, 1, 0, INF), "kind must be 0"),
    ((0.5, 1, 0, -1, 0, 1, 0, INF), "kind must be 0"),
    ((NAN, 1, 0, -1, 0, 1, 0, INF), "kind must be 0"),
    ((1, 3, 0, -1, 0, 1, 0, INF), "quantity must be"),
    ((1, -1, 0, -1, 0, 1, 0, INF), "quantity must be"),
    ((1, 1.5, 0, -1, 0, 1, 0, INF), "quantity must be"),
    ((1, 1, 4, -1, 0, 1, 0, INF), "reduce must be"),
    ((1, 1, -1, -1, 0, 1, 0, INF), "reduce must be"),
    ((1, 1, 0, -2, 0, 1, 0, INF), "zone must be an integer in -1..31"),
    ((1, 1, 0, 32, 0, 1, 0, INF), "zone must be an integer in -1..31"),
    ((1, 1, 0, 0.5, 0, 1, 0, INF), "zone must be an integer in -1..31"),
    ((1, 1, 0, -1, NAN, 1, 0, INF), "must not be NaN"),
    ((1, 1, 0, -1, 0, NAN, 0, INF), "must not be NaN"),
    ((1, 1, 0, -1, 2, 1, 0, INF), "lo must be <= hi"),
    ((1, 1, 0, -1, 0, 1, 10, 5), "t_end must be >= t_start"),
    ((1, 1, 0, -1, 0, 1, NAN, INF), "t_end must be >= t_start"),
    ((1, 1, 0, -1, 0, 1, 0, NAN), "t_end must be >= t_start"),
    ((0, 1, 0, -1, 0, 1, 10, 5), "t_end must be >= t_start"),        # an OFF slot is checked like any other
])
def test_program_check_refusals(native, slot, msg):
    blk = np.ascontiguousarray(_block((1, 1, 0, -1, 0.2, 0.8, -INF, INF), slot, n=2))
    assert native.lib().wt_program_check(native.WT_PROG_SCORE, native.dptr(blk), 2) == native.WT_E_ARG
    assert msg in native.lib().wt_last_error().decode()
    assert refused_as_checked(native, native.WT_PROG_SCORE, blk)


def test_program_check_accepts_valid_blocks(native):
    blk = np.ascontiguousarray(_block((1, 0, 3, 31, -INF, INF, -INF, INF), (1, 2, 2, 0, 5.0, 5.0, 7.0, 7.0),
                                      (1, 1, 1, -1, -INF, -INF, INF, INF), (0, 0, 0, -1, INF, INF, -INF, -INF)))
    assert native.lib().wt_program_check(native.WT_PROG_SCORE, native.dptr(blk), 1) == native.WT_OK


def test_symbols_declared_and_exported(native, wt):
    header = open(os.path.join(ROOT, "include", "wtphys.h")).read()
    for name in ("wt_ensemble_score_set", "wt_ensemble_score_get", "wt_ensemble_score_curve", "wt_ensemble_score_reset",
                 "wt_ensemble_score_clear", "wt_program_check"):
        assert re.search(r"\bint " + name + r"\(", header), name
        assert hasattr(native.lib(), name), name
    for pattern in (r"#define WT_SCR_SLOTS 4\b", r"#define WT_SCR_MAX_BINS 32\b", r"WT_SCR_BAND = 1\b", r"WT_SQ_TEMPERATURE = 2\b",
                    r"WT_SR_MEAN = 3\b", r"WT_NSP = 8\b", r"WT_NSS = 15\b", r"WT_SS_RUN_MAX = 14\b", r"WT_PROG_SCORE = 5\b"):
        assert re.search(pattern, header), pattern
    assert native.WT_PROG_SCORE == 5 and "wt_scr.hpp" in native.BUILD_SOURCES
    for name in ("Score", "ScoreState", "ScoreCurve", "score_block"):
        assert name in wt.__all__ and hasattr(wt, name), name
    for name in ("set_scores", "score_state", "score_curve", "reset_scores", "clear_scores"):
        assert callable(getattr(wt.ReactorEnsemble, name)), name
    scr = importlib.import_module("ics-wt-physicsengine_amd.core.score")
    assert len(scr.PARAM_ROWS) == scr.NSP == 8 and len(scr.STATE_ROWS) == scr.NSS == 15
    assert [f for f in scr.ScoreState.__dataclass_fields__][:15] == list(scr.STATE_ROWS)
