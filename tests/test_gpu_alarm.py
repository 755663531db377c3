"""Per-reactor alarm and interlock programs at every PLC scan (include/wtphys.h ``wt_ensemble_alarm_*``): a fused call
with alarms and trips gives the bits of the host loop it replaces, and the device's alarm state and words follow the
restatement in alarm_ref.py."""
import numpy as np
import pytest

from alarm_ref import AlarmRef
from conftest import golden_json
from control_ref import ControlRef
from inject_ref import InjectRef
from program_helpers import (DT, K, MASTER, HostScan, alarms, assert_all_equal, everything, pi_loops, plant, ref_alarms,
                             refused_as_checked)

pytestmark = pytest.mark.gpu


def _program(wt, cols, seed=3):
    """Four slots with per-reactor limits around each reactor's own start: both trips, both sources, latches,
    deadbands, on-delays and both bad-reading policies."""
    N = len(cols["initial_chlorine"])
    rng = np.random.default_rng(seed)
    cl0, temp = np.asarray(cols["initial_chlorine"]), np.asarray(cols["temperature"])
    return [
        wt.Alarm("chlorine_outlet", "high", cl0 + rng.uniform(-0.3, 0.6, N), deadband=rng.uniform(0, 0.2, N),
                 on_delay=rng.uniform(0, 100, N), latch=rng.random(N) < 0.5, action="trip_chlorine",
                 trip_value=rng.uniform(0, 0.3, N)),
        wt.Alarm("pH_outlet", "low", rng.uniform(6.8, 7.6, N), deadband=0.1, source="field",
                 on_bad=np.where(rng.random(N) < 0.5, "hold", "alarm"), action="trip_acid", trip_value=rng.uniform(0, 2, N)),
        wt.Alarm("temp_outlet", "high", temp + rng.uniform(-0.5, 0.5, N), latch=True),
        wt.Alarm("chlorine_outlet", "low", cl0 + rng.uniform(-1.0, 0.2, N), source="field", on_bad="alarm",
                 on_delay=rng.uniform(0, 50, N), action="trip_chlorine", trip_value=0.5),
    ]


def test_inert_program_is_bit_invisible(gpu, wt):
    N, n = 1000, 8
    cols, bc = wt.make_ensemble(N, seed=41)
    chlorine, acid = pi_loops(wt, cols)
    progs = [[wt.Alarm(np.arange(N) % 7, "off", 5.0, action="trip_acid", trip_value=1.0)] * 4,
             [wt.Alarm("chlorine_outlet", "high", 1e6, action="trip_chlorine", trip_value=0.0, on_bad="hold"),
              wt.Alarm("flow_main", "low", -1e6, source="field", action="trip_acid", trip_value=2.0)]]
    got = []
    for prog in [None] + progs + ["cleared"]:
        ens = plant(wt, cols, bc, n)
        ens.set_schedule(0, 7)
        ens.enable_control(chlorine, acid)
        if prog == "cleared":
            ens.set_alarms(*_program(wt, cols))
            ens.clear_alarms()
        elif prog is not None:
            ens.set_alarms(*prog)
        ens.step(DT, n_steps=K, download=False)
        got.append(everything(ens, programs=("control",)))
        if prog not in (None, "cleared"):
            st = ens.alarm_state()
            assert not st.active.any() and not st.n_act.any() and np.isnan(st.ovr_acid).all()
            assert not st.n_ovr_acid.any() and not st.n_ovr_chlorine.any() and not ens.alarm_words().any()
        ens.close()
    for g in got[1:]:
        assert_all_equal(got[0], g, "inert")


@pytest.mark.parametrize("n, N", [(4, 2000), (8, 2000), (20, 1000), (32, 500)])
def test_fused_alarms_equal_the_host_loop(gpu, wt, n, N):
    cols, bc = wt.make_ensemble(N, seed=777)
    chlorine, acid = pi_loops(wt, cols)
    prog = _program(wt, cols, seed=n)
    block = wt.alarm_block(N, *prog)
    cblock = wt.control_block(N, chlorine, acid)
    for interval in (1, 7, 50):
        ens = plant(wt, cols, bc, n)
        ens.set_schedule(0, interval)
        ctl, alm = ControlRef(cblock, np.zeros(N)), AlarmRef(block, np.zeros(N))
        HostScan(N, ctl=ctl, alm=alm, emulated=True).run(ens, K, interval)     # PI and alarms without the feature
        ref = everything(ens, programs=())
        assert not ref[5].any()
        assert np.mean(alm.st[:, 3].sum(axis=0) > 0) > 0.2, (n, interval)     # alarms activate in many reactors
        assert alm.rst[4:].sum() > 0, (n, interval)                          # and trips act
        ens.close()
        ens = plant(wt, cols, bc, n)
        ens.set_schedule(0, interval)
        ens.set_alarms(*prog)
        ens.enable_control(chlorine, acid)
        ens.step(DT, n_steps=K, download=False)
        assert_all_equal(ref, everything(ens, programs=()), (n, interval))
        assert np.array_equal(ens.control_state().block(), ctl.st), (n, interval)
        assert_all_equal(ref_alarms(alm), alarms(ens), (n, interval, "alarms"))
        ens.close()


def test_field_and_image_under_spoofing(gpu, wt):
    N, n, c = 1000, 8, 5
    cols, bc = wt.make_ensemble(N, seed=91)
    trip = 0.05
    spoof = wt.Injection("chlorine_outlet", "constant", a=0.0)
    prog = [wt.Alarm("chlorine_outlet", "high", 0.2, action="trip_chlorine", trip_value=trip),
            wt.Alarm("chlorine_outlet", "high", 0.2, source="field", latch=True, action="trip_chlorine", trip_value=trip)]
    ens = plant(wt, cols, bc, n, history=K)
    ens.set_schedule(0, c)
    ens.write_commands(*MASTER)
    ens.enable_control(chlorine=wt.PILoop("chlorine_outlet", setpoint=cols["initial_chlorine"], kp=2.0, ki=1e-3))
    ens.set_injections(spoof)
    ens.set_alarms(*prog)
    ens.step(DT, n_steps=K, download=False)
    st = ens.alarm_state()
    assert not st.n_act[0].any() and not st.active[0].any()               # the spoofed image never reads high
    assert (st.n_act[1] > 0).mean() > 0.9                                 # the independent transmitter trips
    # the device's state is the restatement fed with the instruments' own history and the tampered image
    vh, _, fh, filled = ens.sensor_history()
    assert np.all(filled == K)
    inj, ref = InjectRef(wt.injection_block(N, spoof)), AlarmRef(wt.alarm_block(N, *prog), np.zeros(N))
    hs = HostScan(N, inj=inj, alm=ref)
    k = -1
    for steps in hs.calls(K, c):
        k += steps
        vt, _ = hs.scan(vh[k], fh[k], np.zeros((3, N), dtype=np.float32))
        assert not vt[3].any()
    assert_all_equal(ref_alarms(ref), alarms(ens), "spoofed")
    # from the scan after activation on, the plant doses the trip value
    on = st.t_first[1] < hs.lt[0]
    assert on.mean() > 0.9
    assert np.all(ens.boundary()[6][on] == float(np.float32(trip)))
    ens.close()


def test_override_is_downstream_of_command_tampering(gpu, wt):
    N, n = 512, 8
    cols, bc = wt.make_ensemble(N, seed=23)
    trip = 0.3
    ens = plant(wt, cols, bc, n)
    ens.set_schedule(0, 4)
    ens.write_commands(*MASTER)
    ens.set_injections(wt.Injection("chlorine_flow_rate", "constant", a=1.0))
    ens.set_alarms(wt.Alarm("flow_main", "high", -1.0, source="field", on_bad="alarm", action="trip_chlorine",
                            trip_value=trip))
    ens.step(DT, n_steps=4, download=False)                               # first scan: the tamper acts, the slot trips
    assert np.all(ens.boundary()[6] == 1.0)
    ens.step(DT, n_steps=8, download=False)                               # two more scans: the trip wins
    want = float(np.float32(trip))
    b = ens.boundary()
    assert np.all(b[6] == want) and np.all(b[4] == float(np.float32(MASTER[0])))
    st = ens.alarm_state()
    assert np.all(st.n_ovr_chlorine == 2) and not st.n_ovr_acid.any() and np.all(st.ovr_chlorine == trip)
    assert np.all(ens.alarm_words() == (1 | (1 << 4) | (1 << 9) | (1 << 12)))
    ens.close()


def test_latch_and_masked_reset_across_calls(gpu, wt):
    N, n, c = 1000, 8, 5
    cols, bc = wt.make_ensemble(N, seed=33)
    temp = np.asarray(cols["temperature"])
    rng = np.random.default_rng(4)
    prog = [wt.Alarm("temp_outlet", "high", temp + rng.uniform(-0.5, 0.5, N), latch=True, action="trip_acid",
                     trip_value=0.0),
            wt.Alarm("flow_main", "high", -1.0, source="field", on_bad="alarm", latch=True, action="trip_chlorine",
                     trip_value=0.1),
            wt.Alarm("chlorine_outlet", "low", np.asarray(cols["initial_chlorine"]) + rng.uniform(-0.5, 0.5, N),
                     deadband=0.05, latch=rng.random(N) < 0.5)]
    mask = rng.random(N) < 0.5
    ens = plant(wt, cols, bc, n, history=2 * K)
    ens.set_schedule(0, c)
    ens.write_commands(*MASTER)
    ens.set_alarms(*prog)
    ens.step(DT, n_steps=K, download=False)
    ens.reset_alarms(mask)
    ref_mid = alarms(ens)
    ens.step(DT, n_steps=K, download=False)
    vh, _, fh, _ = ens.sensor_history()
    ref = AlarmRef(wt.alarm_block(N, *prog), np.zeros(N))
    hs = HostScan(N, alm=ref)
    k = -1
    for call in range(2):
        for steps in hs.calls(K, c):
            k += steps
            hs.scan(vh[k], fh[k], np.zeros((3, N), dtype=np.float32))
        if call == 0:
            ref.reset(mask)
            assert_all_equal(ref_alarms(ref), ref_mid, "after reset")
    assert_all_equal(ref_alarms(ref), alarms(ens), "second call")
    assert np.all(ens.alarm_state().active[1] == 1)                      # a standing condition is never reset
    ens.reset_alarms()
    assert np.all(ens.alarm_state().active[1] == 1)
    ens.close()


def test_pH_warm_up(gpu, wt):
    N, n, c = 256, 4, 5
    cols, bc = wt.make_ensemble(N, seed=5)
    for on_bad in ("alarm", "hold"):
        ens = plant(wt, cols, bc, n)
        ens.set_schedule(0, c)
        ens.write_commands(*MASTER)
        ens.set_alarms(wt.Alarm("pH_outlet", "high", 100.0, source="field", on_bad=on_bad))
        ens.step(DT, n_steps=170, download=False)                          # 34 scans, all inside the 1800 s warm-up
        st = ens.alarm_state()
        assert np.all(st.n_bad[0] == 34), on_bad
        if on_bad == "alarm":
            assert np.all(st.t_first[0] == c * DT) and np.all(st.active[0] == 1) and np.all(st.first_out == 0)
        else:
            assert not st.n_act.any() and not st.active.any() and not st.cond.any()
        ens.close()


def test_schedules_placement_and_frozen_reactors(gpu, wt):
    N, n = 3000, 8
    cols, bc = wt.make_ensemble(N, seed=2024)
    chlorine, acid = pi_loops(wt, cols, seed=9)
    prog = _program(wt, cols, seed=23)
    got = []
    for v in (dict(streams=0, chunk=1), dict(streams=3, chunk=1), dict(streams=0, chunk=1, fused=False),
              dict(streams=0, chunk=1, adaptive=True)):
        ens = plant(wt, cols, bc, n)
        ens.set_placement(v.get("adaptive", False))
        ens.set_schedule(v["streams"], v["chunk"])
        ens.enable_control(chlorine, acid)
        ens.set_injections(wt.Injection("chlorine_outlet", "bias", start=300.0, end=1500.0, a=0.3))
        ens.set_alarms(*prog)
        for _ in range(5):
            ens.step(DT, n_steps=40, fused=v.get("fused", True), download=False)
        if v.get("adaptive"):
            assert ens.schedule()["redeals"] >= 1 and not np.array_equal(ens.placement()[1], np.arange(N))
        got.append(everything(ens, programs=("control", "alarm")))
        ens.close()
    assert got[0][-3][:, 3].sum() > 0                                     # some slot activated
    for g, v in zip(got[1:], range(1, 4)):
        assert_all_equal(got[0], g, v)
    # a reactor frozen by WT_ST_T_RANGE is not read, so its alarms are not evaluated any more
    g = golden_json("g4_faults.json")["cold_run"]
    cfg = wt.ReactorConfiguration(**g["config"])
    b = wt.BoundaryConditions(**dict(zip(wt.params.BOUNDARY_FIELDS, g["bc"])))
    ens = wt.ReactorEnsemble([cfg, wt.ReactorConfiguration(n_zones=4)])
    ens.set_boundary([b, wt.BoundaryConditions()])
    ens.enable_sensors(seed=1)
    ens.enable_plant_io()
    ens.write_commands([b.acid_flow_rate, 0.0], [b.chlorine_flow_rate, 0.0], [b.inlet_flow_rate, 1.0])
    ens.set_schedule(0, 1)
    ens.set_alarms(wt.Alarm("flow_main", "high", -1.0, source="field", on_bad="alarm", action="trip_acid", trip_value=0.0))
    Kc = 60
    es = ens.step(1.0, n_steps=Kc)
    st = ens.alarm_state()
    assert es.status[0] & 1 and es.time[0] < Kc and es.time[1] == Kc
    assert st.t_prev[0] == es.time[0] and st.t_last[0, 0] == es.time[0] and st.t_prev[1] == Kc
    assert st.time_active[0, 0] == es.time[0] - 1.0 and st.n_ovr_acid[0] == es.time[0] - 1.0
    assert st.n_ovr_acid[1] == Kc - 1
    ens.close()


def test_errors_and_lifetime(gpu, wt):
    from importlib import import_module
    nat = import_module("ics-wt-physicsengine_amd.core._native")
    N, n = 256, 4
    cols, bc = wt.make_ensemble(N, seed=12)
    high = wt.Alarm("chlorine_outlet", "high", 0.1, source="field", on_bad="alarm", action="trip_chlorine", trip_value=0.0)
    ens = wt.ReactorEnsemble(cols, n_zones=n)
    ens.set_boundary(bc)
    with pytest.raises(ValueError, match="plant I/O"):
        ens.set_alarms(high)
    ens.enable_sensors(seed=4)
    with pytest.raises(ValueError, match="plant I/O"):
        ens.set_alarms(high)
    ens.enable_plant_io()
    for call in (ens.alarm_state, ens.alarm_words, ens.reset_alarms):
        with pytest.raises(ValueError, match="no alarm program"):
            call()
    # the n > 32 kernel carries no alarm section: such an ensemble refuses a program
    for big in (33, 40):
        other = plant(wt, cols, bc, big)
        with pytest.raises(ValueError, match="up to 32 zones"):
            other.set_alarms(high)
        with pytest.raises(ValueError, match="no alarm program"):
            other.alarm_state()
        other.close()
    with pytest.raises(ValueError, match="at most 4"):
        ens.set_alarms(*[high] * 5)
    with pytest.raises(ValueError, match="trip_chlorine slot"):
        ens.set_alarms(wt.Alarm(3, "high", 1.0, action="trip_chlorine", trip_value=1.5))
    good = wt.alarm_block(N, high, wt.Alarm("pH_inlet", "low", 6.0, action="trip_acid", trip_value=2.0))
    for slot, row, value in ((0, 0, 3.0), (0, 0, 0.5), (0, 1, 7.0), (0, 2, 2.0), (0, 3, np.nan), (0, 4, -0.5),
                             (0, 5, -1.0), (0, 5, np.inf), (0, 6, 0.5), (0, 7, 2.0), (0, 8, 3.0), (0, 9, 1.5),
                             (1, 9, 2.5), (1, 9, -0.25)):
        bad = good.copy()
        bad[slot, row, 17] = value
        assert nat.lib().wt_ensemble_alarm_set(ens._h, nat.dptr(bad)) == nat.WT_E_ARG, (slot, row, value)
        assert refused_as_checked(nat, nat.WT_PROG_ALARM, bad), (slot, row, value)
    with pytest.raises(ValueError, match="no alarm program"):
        ens.alarm_state()                                      # a refused program leaves none behind
    ens.set_schedule(0, 5)
    ens.write_commands(*MASTER)
    ens.step(DT, n_steps=10, download=False)
    ens.set_alarms(high)
    st = ens.alarm_state()
    assert np.all(st.t_prev == 100.0) and np.all(st.first_out == -1) and np.isnan(st.pending).all()
    ens.step(DT, n_steps=30, download=False)
    st = ens.alarm_state()
    assert np.all(st.n_act[0] == 1) and np.all(st.t_first[0] == 150.0) and np.all(st.n_ovr_chlorine == 5)
    assert np.all(ens.boundary()[6] == 0.0)
    ptr = nat.C.c_void_p()
    assert nat.lib().wt_ensemble_alarm_device(ens._h, nat.C.byref(ptr)) == 0 and ptr.value
    ens.set_alarms(high, wt.Alarm(3, "low", 0.0))                # a new program starts from a fresh state
    st = ens.alarm_state()
    assert not st.n_act.any() and np.isnan(st.t_first).all() and np.all(st.t_prev == 400.0)
    assert not ens.alarm_words().any()
    ens.clear_alarms()
    with pytest.raises(ValueError, match="no alarm program"):
        ens.alarm_state()
    ens.clear_alarms()                                           # no effect while none is set
    ens.step(DT, n_steps=5, download=False)                      # the trip ends with the program
    assert np.all(ens.boundary()[6] == float(np.float32(MASTER[1])))
    ens.close()
