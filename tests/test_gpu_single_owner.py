"""The handle is the single owner of what a ``ReactorEnsemble`` has switched on, of every capacity and of the boundary
block last uploaded (include/wtphys.h ``wt_ensemble_set_boundary``, ``wt_ensemble_info``):
``set_boundary`` skips an upload exactly when the device still holds the bytes, every writer of the device's block ends
that, calls on the raw handle and calls through the object see one state, and the object keeps nothing of its own."""
import ctypes as C

import numpy as np
import pytest

from program_helpers import assert_all_equal, plant
from train_ref import feed_rows, params

pytestmark = pytest.mark.gpu

N, n, DT = 6, 4, 1.0
OWN = {"n_reactors", "n_zones", "device", "columns", "constants", "_h"}


def _open(wt, seed=1):
    cols, bc = wt.make_ensemble(N, seed=seed)
    ens = wt.ReactorEnsemble(cols, n_zones=n)
    ens.set_boundary(bc)
    return ens, cols, bc


def _uploads(native, ens):
    return ens.info(native.WT_INFO_BOUNDARY_UPLOADS)


def _resent(native, ens, bc, expected, what):
    """``set_boundary`` of the very block sent before, after something wrote the device's block: it is uploaded, and
    the device then holds ``expected``."""
    before = _uploads(native, ens)
    ens.set_boundary(bc)
    assert _uploads(native, ens) == before + 1, what
    assert np.array_equal(ens.boundary(), expected), what


def _fields(obj):
    return tuple(v for v in vars(obj).values() if v is not None)


# ---- 1. the skip happens, and only when it may
def test_an_equal_block_is_not_uploaded_again(gpu, wt, native):
    ens, _, bc = _open(wt)
    assert _uploads(native, ens) == 1 and set(vars(ens)) == OWN
    ens.set_boundary(bc)
    ens.set_boundary(bc.copy())
    ens.step(DT, bc)
    assert _uploads(native, ens) == 1
    other = bc.copy()
    other[8, N - 1] += 0.5
    ens.set_boundary(other)
    assert _uploads(native, ens) == 2 and np.array_equal(ens.boundary(), other)
    ens.step(DT, other)
    assert _uploads(native, ens) == 2
    ens.close()


# ---- 2. the comparison is by bytes
def test_a_block_that_differs_in_a_sign_bit_is_uploaded(gpu, wt, native):
    ens, _, bc = _open(wt)
    plus = bc.copy()
    plus[4] = 0.0
    ens.set_boundary(plus)
    assert not np.signbit(ens.boundary()[4]).any()
    minus = plus.copy()
    minus[4] = -0.0
    assert np.array_equal(minus, plus)              # equal as numbers
    before = _uploads(native, ens)
    ens.set_boundary(minus)
    assert _uploads(native, ens) == before + 1
    assert np.signbit(ens.boundary()[4]).all()
    ens.close()


# ---- 3. every writer of the device's block ends the skip
def test_a_plc_scan_dirties_the_block(gpu, wt, native):
    cols, bc = wt.make_ensemble(N, seed=2)
    ens = plant(wt, cols, bc, n)
    ens.write_commands(1.5, 0.75, 9.0)
    ens.step(DT, n_steps=2)
    assert not np.array_equal(ens.boundary(), bc)
    _resent(native, ens, bc, bc, "plant I/O scan")
    ens.close()


def test_a_disturbance_program_dirties_the_block(gpu, wt, native):
    """Under a running program ``set_boundary`` recomposes the targeted row from the current offset (include/wtphys.h):
    the device holds ``bc`` with row 3 = bc[3] + a, and the program's base is ``bc`` itself."""
    ens, _, bc = _open(wt, seed=3)
    a = 1.0
    ens.set_disturbances(wt.Disturbance.step("inlet_temperature", a, start=0.5))
    ens.step(DT, n_steps=1)
    expected = bc.copy()
    expected[3] = np.clip(bc[3] + a, 0.0, 100.0)
    _resent(native, ens, bc, expected, "set_disturbances, one step")
    assert np.array_equal(ens.disturbance_state().base, bc)
    ens.clear_disturbances()
    _resent(native, ens, bc, bc, "clear_disturbances")
    ens.set_boundary(bc)                            # and from here on the block is the host's again
    assert _uploads(native, ens) == 3
    ens.close()


def test_a_train_program_dirties_the_block(gpu, wt, native):
    """Rows 1..3 of a linked stage hold the upstream's outlet (tests/train_ref.py), the rest of the block is ``bc``."""
    ens, cols, bc = _open(wt, seed=4)
    link, rows = params(N, 2)
    fed = lambda: feed_rows(bc.copy(), ens.state, link, rows, np.ones(N, dtype=bool))
    ens.set_trains(2)
    assert not np.array_equal(fed(), bc)
    _resent(native, ens, bc, fed(), "set_trains")
    ens.step(DT, n_steps=2)
    _resent(native, ens, bc, fed(), "a step under trains")
    shape = (N, n)
    ens.set_state(np.broadcast_to(np.linspace(6.6, 7.6, N)[:, None], shape), np.broadcast_to(np.linspace(0.5, 1.5, N)[:, None], shape),
                  np.broadcast_to(np.linspace(12.0, 22.0, N)[:, None], shape))
    _resent(native, ens, bc, fed(), "set_state under trains")
    ens.set_pipes(1)                                # every line full of the upstream's outlet as it is now
    _resent(native, ens, bc, fed(), "set_pipes")
    ens.clear_trains()
    _resent(native, ens, bc, bc, "clear_trains")
    ens.close()


def test_a_scheduled_step_leaves_its_last_row_known(gpu, wt, native):
    ens, _, bc = _open(wt, seed=5)
    S = wt.make_boundary_schedule(bc, 3, seed=6)
    assert not np.array_equal(S[-1], bc)
    ens.step(DT, n_steps=3, boundary_schedule=S)
    before = _uploads(native, ens)
    ens.set_boundary(S[-1])
    ens.step(DT, S[-1])
    assert _uploads(native, ens) == before and np.array_equal(ens.boundary(), S[-1])
    _resent(native, ens, bc, bc, "another block")
    ens.close()


# ---- 4. the raw handle and the object agree
def test_programs_set_on_the_raw_handle_download_through_the_object(gpu, wt, native):
    L = native.lib()
    cols, bc = wt.make_ensemble(N, seed=7)
    trd = (wt.Trend("image_value", "chlorine_outlet"), wt.Trend("command", "acid"))
    scr = (wt.Score("pH", 6.5, 8.5), wt.Score("temperature", hi=25.0, reduce="max"))
    dst = (wt.Disturbance.step("ambient_temperature", 2.0, start=0.5),)
    det = (wt.Detector("chlorine_outlet", "cusum", 5.0, sigma=0.05),)
    lo, hi = np.zeros(4), np.full(4, 30.0)
    lab = wt.core.detect.label_block(N, (1.0, 2.5))
    got = []
    for raw in (True, False):
        ens = plant(wt, cols, bc, n)
        if raw:
            h = ens._h
            for rc in (L.wt_ensemble_trend_set(h, native.dptr(wt.trend_block(N, *trd)), 4, 0),
                       L.wt_ensemble_score_set(h, native.dptr(wt.score_block(N, *scr)), 3, 2, native.dptr(lo), native.dptr(hi)),
                       L.wt_ensemble_disturb_set(h, native.dptr(wt.disturbance_block(N, *dst)), C.c_uint64(9), 0, 2),
                       L.wt_ensemble_detect_set(h, native.dptr(wt.detector_block(N, *det)), native.dptr(lab))):
                native.check(rc)
        else:
            ens.set_trends(*trd, capacity=4)
            ens.set_scores(*scr, curve=3, bins=2, fan_range=(0.0, 30.0))
            ens.set_disturbances(*dst, seed=9, history=2)
            ens.set_detectors(*det, attack=(1.0, 2.5))
        ens.write_commands(0.5, 0.25, 6.0)
        ens.step(DT, n_steps=3, fused=False, download=False)
        data, curve, (off, filled), ds = ens.trend_data(), ens.score_curve(), ens.disturbance_history(), ens.detector_state()
        assert data.time.shape == data.value.shape == (8, 4, N) and (data.count[:2] == 3).all()
        assert curve.n_scored.shape == (3, 4) and curve.fan.shape == (3, 4, 4) and curve.edges.shape == (4, 3)
        assert np.array_equal(curve.edges[0], [0.0, 15.0, 30.0])
        assert off.shape == (2, 4, N) and (filled == 2).all() and (off[:, 0] == [[0.0], [2.0]]).all()
        assert np.array_equal(ds.label_start, lab[0]) and np.array_equal(ds.label_end, lab[1]) and (ds.n_eval[0] == 3).all()
        got.append(_fields(data) + _fields(curve) + (off, filled) + _fields(ds))
        assert set(vars(ens)) == OWN
        ens.close()
    assert len(got[0]) == len(got[1])
    assert_all_equal(got[1], got[0], "raw handle against methods")


# ---- 5. a refused replacement changes nothing
def test_a_refused_set_leaves_the_old_capacity(gpu, wt, native):
    cols, bc = wt.make_ensemble(N, seed=8)
    ens = plant(wt, cols, bc, n)
    ens.set_trends(wt.Trend("image_value", "pH_outlet"), capacity=4)
    with pytest.raises(ValueError):
        ens.set_trends(wt.Trend("image_value", "pH_outlet", every=0), capacity=9)
    bad = wt.trend_block(N, wt.Trend("image_value", "pH_outlet"))
    bad[0, 2] = 0.0                                 # every = 0, past the builder's check
    assert native.lib().wt_ensemble_trend_set(ens._h, native.dptr(bad), 9, 0) == native.WT_E_ARG
    assert ens.info(native.WT_INFO_TREND_CAPACITY) == 4
    ens.step(DT, n_steps=2, fused=False, download=False)
    data = ens.trend_data()
    assert data.time.shape[1] == 4 and (data.count[0] == 2).all()
    ens.close()


# ---- 6. calls before their part exists
def test_sensor_history_before_the_sensors_is_the_librarys_refusal(gpu, wt, native):
    ens, _, _ = _open(wt)
    with pytest.raises(native.WtError) as e:
        ens.sensor_history()
    assert e.value.code == native.WT_E_STATE
    assert e.value.message in ("sensor suite not enabled", "sensor history not enabled")
    with pytest.raises(ValueError, match="no train program is set"):
        ens.set_pipes(1)
    assert ens.wave_diag() is None and ens.wave_diag().shape[1] == native.lib().wt_wave_diag_slots()
    ens.close()
    cols, _ = wt.make_ensemble(N, seed=1)
    ens = wt.ReactorEnsemble(cols, n_zones=n)       # no boundary yet
    with pytest.raises(ValueError, match="set_boundary must precede step"):
        ens.step(DT)
    ens.close()


# ---- 7. no mirror creeps back
def test_the_object_keeps_only_what_it_was_constructed_with(gpu, wt, native):
    cols, bc = wt.make_ensemble(N, seed=9)
    ens = plant(wt, cols, bc, n, history=4)
    assert set(vars(ens)) == OWN
    ens.write_commands(0.5, 0.25, 6.0)
    ens.record(every=1, capacity=4)
    chlorine = wt.PILoop("chlorine_outlet", setpoint=1.0, kp=0.5, ki=1e-3, bias=0.2)
    ens.enable_control(chlorine)
    ens.retune_control(acid=wt.PILoop("pH_outlet", setpoint=7.0, kp=0.2, direction=-1))
    ens.set_injections(wt.Injection("chlorine_outlet", "bias", a=0.1))
    ens.set_alarms(wt.Alarm("pH_outlet", "high", 8.0))
    ens.set_actuators(wt.Actuator("acid", tau=5.0))
    ens.set_disturbances(wt.Disturbance.step("ambient_temperature", 1.0), history=2)
    ens.set_scores(wt.Score("pH", 6.5, 8.5), curve=3, bins=2, fan_range=(0.0, 14.0))
    ens.set_detectors(wt.Detector("chlorine_outlet", "cusum", 5.0), attack=(1.0, 2.0))
    ens.set_trends(wt.Trend("image_value", "chlorine_outlet"), capacity=4)
    ens.set_trains(2)
    ens.set_pipes(1)
    assert ens.wave_diag() is None
    ens.step(DT, n_steps=2, fused=False, download=False)
    assert ens.wave_diag() is not None
    ens.set_boundary(bc)
    ens.step(DT, bc, n_steps=1)
    for read in (ens.sensor_history, ens.trajectory, ens.control_state, ens.injection_state, ens.alarm_state, ens.actuator_state,
                 ens.disturbance_state, ens.disturbance_history, ens.score_state, ens.score_curve, ens.detector_state,
                 ens.trend_state, ens.trend_data, ens.train_state, ens.pipe_state, ens.pipe_lines, ens.boundary):
        read()
    assert [ens.info(native.WT_INFO_PROGRAM + p) for p in range(8)] == [1] * 8
    assert [ens.info(w) for w in (native.WT_INFO_PLANT_IO, native.WT_INFO_TRAIN, native.WT_INFO_PIPE, native.WT_INFO_SENSOR_HISTORY,
                                  native.WT_INFO_DISTURB_HISTORY, native.WT_INFO_SCORE_CURVE, native.WT_INFO_SCORE_BINS,
                                  native.WT_INFO_TREND_CAPACITY, native.WT_INFO_TRAIN_LENGTH, native.WT_INFO_WAVE_DIAG)] \
        == [1, 1, 1, 4, 2, 3, 2, 4, 2, 1]
    assert set(vars(ens)) == OWN
    for clear in (ens.clear_pipes, ens.clear_trains, ens.clear_trends, ens.clear_detectors, ens.clear_scores, ens.clear_disturbances,
                  ens.clear_actuators, ens.clear_alarms, ens.clear_injections, ens.disable_control):
        clear()
    assert [ens.info(native.WT_INFO_PROGRAM + p) for p in range(8)] == [0] * 8
    assert [ens.info(w) for w in (native.WT_INFO_TRAIN, native.WT_INFO_PIPE, native.WT_INFO_DISTURB_HISTORY, native.WT_INFO_SCORE_CURVE,
                                  native.WT_INFO_SCORE_BINS, native.WT_INFO_TREND_CAPACITY, native.WT_INFO_TRAIN_LENGTH,
                                  native.WT_INFO_WAVE_DIAG)] == [0] * 8
    with pytest.raises(native.WtError) as e:
        ens.info(99)
    assert (e.value.code, e.value.message) == (native.WT_E_ARG, "unknown info code")
    assert set(vars(ens)) == OWN
    ens.close()


# ---- 8. a loop that retune keeps, keeps its bits
def test_retune_keeps_the_other_loops_rows_bit_for_bit(gpu, wt, native):
    cols, bc = wt.make_ensemble(N, seed=10)
    ens = plant(wt, cols, bc, n)
    u = np.random.default_rng(11).random((3, N))
    chlorine = wt.PILoop("chlorine_outlet", setpoint=cols["initial_chlorine"] + u[0], kp=0.2 + u[1], ki=1e-3 * u[2], bias=1.0 / 3.0)
    acid = wt.PILoop("pH_outlet", setpoint=7.1, kp=0.3, ki=2e-4, direction=-1, bias=0.1)
    sent = wt.control_block(N, chlorine)

    def held():
        blk = np.empty_like(sent)
        native.check(native.lib().wt_ensemble_program_params(ens._h, native.WT_PROG_CONTROL, native.dptr(blk)))
        return blk

    with pytest.raises(ValueError, match="control is off"):
        ens.retune_control(None, acid)
    ens.enable_control(chlorine)
    before = held()
    assert before.tobytes() == sent.tobytes()
    ens.step(DT, n_steps=2, fused=False, download=False)
    ens.retune_control(None, acid)
    after = held()
    assert after[0].tobytes() == before[0].tobytes()
    assert after[1].tobytes() == wt.control_block(N, None, acid)[1].tobytes() and after[1, 0].all()
    ens.retune_control(chlorine, False)
    assert held().tobytes() == sent.tobytes()
    ens.close()
