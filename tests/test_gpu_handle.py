"""The ensemble handle's lifecycle (include/wtphys.h): the refusals of calls made out of order, with their exact messages,
for every one of the ten per-reactor programs; a handle whose sensor history, plant I/O, recording and ten programs
are released and set again mid-run giving the bits of one that was set up once; and a cleared program leaving nothing
behind."""
import ctypes as C
from typing import NamedTuple, Optional

import numpy as np
import pytest

from program_helpers import DT, MASTER, assert_all_equal, pi_loops, plant, plant_state

pytestmark = pytest.mark.gpu

N, n = 96, 8


class Program(NamedTuple):
    """One row per program: its set (enable) entry point, a valid block for ``n_reactors`` reactors and the arguments after
    it, the messages of a NULL handle and of a NULL block, of the precondition and of the zone limit, the "not set"
    message, the ``ReactorEnsemble`` calls that need a program set (get, reset, the other reads), the clear method."""
    name: str
    set: object
    block: np.ndarray
    rest: tuple
    null_handle: str
    null_block: str
    needs: str
    zones: Optional[str]
    not_set: str
    reads: tuple
    clear: str


def _table(wt, native, cols):
    L, nr = native.lib(), len(cols["initial_chlorine"])
    chlorine, acid = pi_loops(wt, cols)
    null = "NULL argument"
    return (
        Program("control", L.wt_ensemble_control_enable, wt.control_block(nr, chlorine, acid), (), "NULL handle", "params is NULL",
                "control writes the holding image: enable plant I/O first", None,
                "control is off (wt_ensemble_control_enable)", ("control_state",), "disable_control"),
        Program("inject", L.wt_ensemble_inject_set, wt.injection_block(nr, wt.Injection("chlorine_outlet", "bias", a=0.1)), (), null, null,
                "injection acts on the plant I/O images: enable plant I/O first",
                "injection programs run in the kernels for up to 32 zones",
                "no injection program is set (wt_ensemble_inject_set)", ("injection_state",), "clear_injections"),
        Program("alarm", L.wt_ensemble_alarm_set, wt.alarm_block(nr, wt.Alarm("pH_outlet", "high", 8.0)), (), null, null,
                "alarms act on the plant I/O scan: enable plant I/O first", "alarm programs run in the kernels for up to 32 zones",
                "no alarm program is set (wt_ensemble_alarm_set)", ("alarm_state", "reset_alarms", "alarm_words"), "clear_alarms"),
        Program("actuator", L.wt_ensemble_actuator_set, wt.actuator_block(nr, wt.Actuator("acid", tau=5.0)), (), null, null,
                "actuators act on the plant I/O scan: enable plant I/O first",
                "actuator programs run in the kernels for up to 32 zones",
                "no actuator program is set (wt_ensemble_actuator_set)", ("actuator_state",), "clear_actuators"),
        Program("disturb", L.wt_ensemble_disturb_set, wt.disturbance_block(nr, wt.Disturbance.step("inlet_temperature", 1.0)),
                (C.c_uint64(1), 0, 0), null, null, "set_state and set_boundary must precede disturb_set",
                "disturbance programs run in the kernels for up to 32 zones",
                "no disturbance program is set (wt_ensemble_disturb_set)", ("disturbance_state", "disturbance_history"),
                "clear_disturbances"),
        Program("score", L.wt_ensemble_score_set, wt.score_block(nr, wt.Score("pH", 6.5, 8.5)), (0, 0, None, None), null, null,
                "set_state must precede score_set", "score programs run in the kernels for up to 32 zones",
                "no score program is set (wt_ensemble_score_set)", ("score_state", "reset_scores", "score_curve"), "clear_scores"),
        Program("detect", L.wt_ensemble_detect_set, wt.detector_block(nr, wt.Detector("chlorine_outlet", "cusum", 5.0)),
                (native.dptr(_labels(wt, nr)),), null, null, "detectors read the plant I/O scan: enable plant I/O first",
                "detector programs run in the kernels for up to 32 zones",
                "no detector program is set (wt_ensemble_detect_set)", ("detector_state", "reset_detectors"), "clear_detectors"),
        Program("trend", L.wt_ensemble_trend_set, wt.trend_block(nr, wt.Trend("image_value", "chlorine_outlet")), (4, 0), null, null,
                "trends read the plant I/O scan: enable plant I/O first", "trend programs run in the kernels for up to 32 zones",
                "no trend program is set (wt_ensemble_trend_set)", ("trend_state", "reset_trends", "trend_data"), "clear_trends"),
        Program("service", L.wt_ensemble_service_set, wt.service_block(nr, wt.Service("chlorine_outlet", "calibrate", at=60.0)), (),
                null, null, "the sensor suite is not enabled (wt_ensemble_sensors_enable)",
                "service programs run in the kernels for up to 32 zones",
                "no service program is set (wt_ensemble_service_set)", ("service_state", "service_params", "reset_services"),
                "clear_services"),
        Program("tune", L.wt_ensemble_tune_set, wt.tune_block(nr, wt.RelayTune("chlorine_outlet", 1.5, 0.25, 0.5)), (), null, null,
                "tuners act on the plant I/O scan: enable plant I/O first", "tune programs run in the kernels for up to 32 zones",
                "no tune program is set (wt_ensemble_tune_set)", ("tuner_state", "tuner_params", "reset_tuners"), "clear_tuners"),
    )


_LABELS = {}


def _labels(wt, nr):
    """The never-attacked label block of ``nr`` reactors (kept alive: the table holds a pointer to it)."""
    if nr not in _LABELS:
        _LABELS[nr] = np.ascontiguousarray(wt.core.detect.label_block(nr))
    return _LABELS[nr]


def _refused(native, code, msg, call, *args):
    assert call(*args) == code, msg
    assert native.lib().wt_last_error() == msg.encode()


def _raises(native, msg, call, *args):
    """A ``ReactorEnsemble`` call that the library refuses with WT_E_STATE and exactly ``msg``."""
    with pytest.raises(ValueError) as e:
        call(*args)
    assert str(e.value) == msg and native.lib().wt_last_error() == msg.encode()


def _raw_handle(native, ens):
    """A handle of ``ens``'s shape straight from wt_ensemble_create: neither state nor boundary set."""
    h = C.c_void_p()
    native.check(native.lib().wt_ensemble_create(ens.n_reactors, ens.n_zones, 0, native.dptr(np.ascontiguousarray(ens.constants)),
                                                 C.byref(h)))
    return h


def test_calls_out_of_order_are_refused_with_their_messages(gpu, wt, native):
    cols, bc = wt.make_ensemble(N, seed=3)
    ens = wt.ReactorEnsemble(cols, n_zones=n)       # the state is set, the boundary is not
    L, h, S, A = native.lib(), ens._h, native.WT_E_STATE, native.WT_E_ARG
    raw = _raw_handle(native, ens)                  # not even the state
    table = _table(wt, native, cols)
    _refused(native, S, "the register image publishes sensor readings: enable the sensor suite first", L.wt_ensemble_plc_enable, h)
    for p in table:
        _refused(native, A, p.null_handle, p.set, None, native.dptr(p.block), *p.rest)
        _refused(native, A, p.null_block, p.set, h, None, *p.rest)
        _refused(native, S, p.needs, p.set, raw if p.name == "score" else h, native.dptr(p.block), *p.rest)
        for read in p.reads:   # get, reset and the other read calls before any set
            _raises(native, p.not_set, getattr(ens, read))
    word = C.c_void_p()
    _refused(native, S, table[2].not_set, L.wt_ensemble_alarm_device, h, C.byref(word))
    L.wt_ensemble_destroy(raw)
    with pytest.raises(native.WtError) as e:
        ens.trajectory()
    assert (e.value.code, e.value.message) == (S, "recording is off (wt_ensemble_record)")
    ens.set_boundary(bc)
    ens.enable_sensors(seed=1)
    with pytest.raises(native.WtError) as e:
        ens.enable_sensors(seed=1)
    assert (e.value.code, e.value.message) == (S, "sensor suite already enabled")
    with pytest.raises(native.WtError) as e:
        ens.sensor_history()
    assert (e.value.code, e.value.message) == (S, "sensor history not enabled")
    ens.enable_plant_io()
    _refused(native, S, "plant I/O already enabled", L.wt_ensemble_plc_enable, h)
    _refused(native, S, table[0].not_set, L.wt_ensemble_control_retune, h, native.dptr(table[0].block))   # nothing to retune
    for p in table:   # accepted once what the program needs is there
        assert p.set(h, native.dptr(p.block), *p.rest) == native.WT_OK, p.name
    ens.close()


def test_programs_above_32_zones_are_refused_with_their_messages(gpu, wt, native):
    cols, bc = wt.make_ensemble(3, seed=4)
    ens = plant(wt, cols, bc, 33)
    for p in _table(wt, native, cols):
        if p.zones is None:    # every kernel carries the PI programs
            assert p.set(ens._h, native.dptr(p.block), *p.rest) == native.WT_OK, p.name
        else:
            _refused(native, native.WT_E_STATE, p.zones, p.set, ens._h, native.dptr(p.block), *p.rest)
    ens.close()


def _programs(wt, cols):
    chlorine, acid = pi_loops(wt, cols)
    temp = np.asarray(cols["temperature"])
    return ((chlorine, acid),
            (wt.Injection("chlorine_outlet", "bias", start=50.0, end=400.0, a=0.3),
             wt.Injection("acid_flow_rate", "gain", start=100.0, end=300.0, a=1.5)),
            (wt.Alarm("temp_outlet", "high", temp + 0.1, latch=True, action="trip_acid", trip_value=0.5),
             wt.Alarm("chlorine_outlet", "low", 0.05, source="field", on_bad="alarm")),
            (wt.Actuator("acid", tau=20.0, delay=2), wt.Actuator("chlorine", rate=0.01, backlash=0.02),
             wt.Actuator("inlet", tau=5.0)),
            (wt.Disturbance.step("inlet_temperature", 1.5, start=30.0), wt.Disturbance.ou("inlet_pH", 0.05, 200.0),
             wt.Disturbance.ramp("ambient_temperature", 1e-3)),
            (wt.Score("chlorine", 0.5, 3.0), wt.Score("pH", 6.5, 8.5, reduce="mean"), wt.Score("temperature", hi=25.0, reduce="max")),
            (wt.Detector("chlorine_outlet", "cusum", 5.0, sigma=0.05, ref="track", tau=100.0),
             wt.Detector("pH_outlet", "ewma", 3.0, sigma=0.1, ref_value=7.0, source="field")),
            (wt.Trend("image_value", "chlorine_outlet"), wt.Trend("command", "acid", every=2),
             wt.Trend("control", ("chlorine", "output"), deadband=0.01), wt.Trend("alarm_word")),
            (wt.Service("chlorine_outlet", "calibrate", at=60.0, every=50.0, ref_mode="trim"), wt.Service("pH_outlet", "rinse", at=30.0)),
            (wt.RelayTune("chlorine_outlet", np.asarray(cols["initial_chlorine"]), 0.2, 0.3, start=40.0, settle=0, cycles=1), None))


def _set_all(ens, progs, history, curve, bins, capacity):
    ctl, inj, alm, act, dst, scr, det, trd, svc, tun = progs
    ens.enable_control(*ctl)
    ens.set_injections(*inj)
    ens.set_alarms(*alm)
    ens.set_actuators(*act)
    ens.set_disturbances(*dst, seed=9, history=history)
    ens.set_scores(*scr, curve=curve, bins=bins, fan_range=(0.0, 30.0))
    ens.set_detectors(*det, attack=(60.0, 150.0))
    ens.set_trends(*trd, capacity=capacity, wrap=True)
    ens.set_services(*svc)
    ens.set_tuners(*tun)


def _fields(obj):
    return tuple(v for v in vars(obj).values() if v is not None)


def _observe(ens):
    return (plant_state(ens) + ens.input_image() + ens.sensor_history() + (ens.control_state().block(),)
            + (ens.injection_state().block(),) + ens.alarm_state().block() + (ens.alarm_words(),)
            + ens.actuator_state().block() + tuple(vars(ens.trajectory()).values())
            + _fields(ens.disturbance_state()) + ens.disturbance_history() + _fields(ens.score_state()) + _fields(ens.score_curve())
            + _fields(ens.detector_state()) + _fields(ens.trend_state()) + _fields(ens.trend_data())
            + _fields(ens.service_state()) + (ens.tuner_state().block(),))


def test_released_and_reset_groups_give_the_bits_of_a_handle_set_up_once(gpu, wt):
    cols, bc = wt.make_ensemble(N, seed=17)
    progs = _programs(wt, cols)
    got = []
    for cycle in (True, False):
        ens = plant(wt, cols, bc, n, history=24)
        ens.set_schedule(0, 3)
        ens.write_commands(*MASTER)
        ens.record(every=2, capacity=8)
        _set_all(ens, progs, history=8, curve=6, bins=4, capacity=8)
        ens.step(DT, n_steps=12, download=False)
        if cycle:   # every group released and allocated again
            ens.disable_control(); ens.clear_injections(); ens.clear_alarms(); ens.clear_actuators()
            ens.clear_disturbances(); ens.clear_scores(); ens.clear_detectors(); ens.clear_trends()
            ens.clear_services(); ens.clear_tuners()
            ens.record(capacity=0)
        # otherwise: set calls that replace the programs in place, at the new capacities
        _set_all(ens, progs, history=16, curve=12, bins=8, capacity=16)
        ens.record(every=3, capacity=5)
        ens.step(DT, n_steps=12, download=False)
        obs = _observe(ens)
        assert len(ens.trajectory()) == 4 and not obs[5].any()
        assert ens.disturbance_history()[0].shape[0] == 16 and ens.score_curve().n_scored.shape == (12, 4)
        assert ens.score_curve().fan.shape == (12, 4, 10) and ens.trend_data().time.shape[1] == 16
        got.append(obs)
        ens.close()   # everything still set
    assert len(got[0]) == len(got[1])
    assert_all_equal(got[1], got[0], "cycle")


def test_a_cleared_program_is_refused_again_and_leaves_no_capacity_behind(gpu, wt, native):
    cols, bc = wt.make_ensemble(N, seed=21)
    progs = _programs(wt, cols)
    ens = plant(wt, cols, bc, n)
    _set_all(ens, progs, history=8, curve=6, bins=4, capacity=8)
    ens.step(DT, n_steps=3, download=False)
    for p in _table(wt, native, cols):
        getattr(ens, p.clear)()
        for read in p.reads:
            _raises(native, p.not_set, getattr(ens, read))
    # the smallest capacities after the larger ones: nothing of the released arrays' sizes is left in the handle
    dst, scr, trd = progs[4], progs[5], progs[7]
    ens.set_disturbances(*dst, history=0)
    ens.set_scores(*scr)
    ens.set_trends(*trd, capacity=1)
    ens.step(DT, n_steps=3, download=False)
    assert ens.disturbance_history()[0].shape[0] == 0
    curve = ens.score_curve()
    assert curve.n_scored.shape == (0, 4) and curve.fan is None
    data = ens.trend_data()
    assert data.time.shape[1] == 1 and data.value.shape[1] == 1
    ens.close()
