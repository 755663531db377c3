"""The ensemble handle's lifecycle (include/wtphys.h): the refusals of calls made out of order, with their exact messages,
and a handle whose sensor history, plant I/O, recording and four scan programs are released and set again mid-run giving
the bits of one that was set up once."""
import numpy as np
import pytest

from program_helpers import DT, MASTER, assert_all_equal, pi_loops, plant, plant_state

pytestmark = pytest.mark.gpu

N, n = 96, 8


def _refused(native, code, msg, call, *args):
    assert call(*args) == code, msg
    assert native.lib().wt_last_error() == msg.encode()


def test_calls_out_of_order_are_refused_with_their_messages(gpu, wt, native):
    cols, bc = wt.make_ensemble(N, seed=3)
    ens = wt.ReactorEnsemble(cols, n_zones=n)
    ens.set_boundary(bc)
    L, h, S = native.lib(), ens._h, native.WT_E_STATE
    _refused(native, S, "the register image publishes sensor readings: enable the sensor suite first", L.wt_ensemble_plc_enable, h)
    chlorine, acid = pi_loops(wt, cols)
    blocks = [(L.wt_ensemble_control_enable, wt.control_block(N, chlorine, acid),
               "control writes the holding image: enable plant I/O first"),
              (L.wt_ensemble_inject_set, wt.injection_block(N, wt.Injection("chlorine_outlet", "bias", a=0.1)),
               "injection acts on the plant I/O images: enable plant I/O first"),
              (L.wt_ensemble_alarm_set, wt.alarm_block(N, wt.Alarm("pH_outlet", "high", 8.0)),
               "alarms act on the plant I/O scan: enable plant I/O first"),
              (L.wt_ensemble_actuator_set, wt.actuator_block(N, wt.Actuator("acid", tau=5.0)),
               "actuators act on the plant I/O scan: enable plant I/O first")]
    for call, blk, msg in blocks:
        _refused(native, S, msg, call, h, native.dptr(blk))
    with pytest.raises(native.WtError) as e:
        ens.trajectory()
    assert (e.value.code, e.value.message) == (S, "recording is off (wt_ensemble_record)")
    ens.enable_sensors(seed=1)
    with pytest.raises(native.WtError) as e:
        ens.enable_sensors(seed=1)
    assert (e.value.code, e.value.message) == (S, "sensor suite already enabled")
    with pytest.raises(native.WtError) as e:
        ens.sensor_history()
    assert (e.value.code, e.value.message) == (S, "sensor history not enabled")
    ens.enable_plant_io()
    _refused(native, S, "plant I/O already enabled", L.wt_ensemble_plc_enable, h)
    for call, blk, _ in blocks:   # accepted once plant I/O is on
        assert call(h, native.dptr(blk)) == native.WT_OK
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
             wt.Actuator("inlet", tau=5.0)))


def _set_all(ens, progs):
    ctl, inj, alm, act = progs
    ens.enable_control(*ctl)
    ens.set_injections(*inj)
    ens.set_alarms(*alm)
    ens.set_actuators(*act)


def _observe(ens):
    return (plant_state(ens) + ens.input_image() + ens.sensor_history() + (ens.control_state().block(),)
            + (ens.injection_state().block(),) + ens.alarm_state().block() + (ens.alarm_words(),)
            + ens.actuator_state().block() + tuple(vars(ens.trajectory()).values()))


def test_released_and_reset_groups_give_the_bits_of_a_handle_set_up_once(gpu, wt):
    cols, bc = wt.make_ensemble(N, seed=17)
    progs = _programs(wt, cols)
    got = []
    for cycle in (True, False):
        ens = plant(wt, cols, bc, n, history=24)
        ens.set_schedule(0, 3)
        ens.write_commands(*MASTER)
        ens.record(every=2, capacity=8)
        _set_all(ens, progs)
        ens.step(DT, n_steps=12, download=False)
        if cycle:   # every group released and allocated again
            ens.disable_control(); ens.clear_injections(); ens.clear_alarms(); ens.clear_actuators()
            ens.record(capacity=0)
        _set_all(ens, progs)   # otherwise: set calls that replace the programs in place
        ens.record(every=3, capacity=5)
        ens.step(DT, n_steps=12, download=False)
        obs = _observe(ens)
        assert len(ens.trajectory()) == 4 and not obs[5].any()
        got.append(obs)
        ens.close()   # everything still set
    assert_all_equal(got[1], got[0], "cycle")
