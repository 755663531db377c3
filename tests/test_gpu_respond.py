"""Per-reactor response programs at the PLC scans (include/wtphys.h ``wt_ensemble_respond_*``): a scripted cause with a
known answer, a fused call against the host master it replaces (tests/respond_ref.py) beside tuner, controller, PI,
alarm, detector and injection programs, the lifecycle and the checkpoints.  Shapes: five wavefront-groups plus one
reactor at n = 8 (row mode), 5 (non-row) and 20, and 33 reactors of 2 zones (32 scan lanes in one wavefront and a
wavefront with one), each with the library's own spreading and with full wavefronts, a scan every step and every
third step."""
import numpy as np
import pytest

import respond_ref as RR
from checkpoint_helpers import holding_words
from control_ref import float32_words
from program_helpers import (DT, HostScan, assert_all_equal, assert_equal_by_reactor, commands, packing, plant,  # noqa: F401
                             plant_state, ragged_size, ref_alarms, alarms, words)
from respond_cases import MASTER, SCANS, Scenario, not_vacuous

pytestmark = pytest.mark.gpu

ZONES = (8, 5, 20, 2)
INTERVALS = (1, 3)


def ensemble(wt, n, seed=0):
    R, N = (32, 33) if n == 2 else ragged_size(n)
    cols, bc = wt.make_ensemble(N, seed=6100 + n + seed)
    return R, N, cols, bc


def observed(ens):
    """State, readings, boundary, input image and holding image of every reactor."""
    return plant_state(ens) + ens.input_image() + (holding_words(ens),)


def responses(ens):
    return ens.response_state().block()


def around(ens):
    """PI, controller, tuner, alarm and detector state."""
    return ((ens.control_state().block(), ens.mpc_state().block(), ens.mpc_prediction(), ens.tuner_state().block())
            + tuple(alarms(ens)) + tuple(ens.detector_state().block()))


def ref_around(refs):
    det = refs["det"]
    return ((refs["ctl"].st, refs["mpc"].st, refs["mpc"].pred, refs["tun"].st) + tuple(ref_alarms(refs["alm"]))
            + (det.st, det.t_prev))


@pytest.mark.parametrize("interval", INTERVALS)
@pytest.mark.parametrize("n", ZONES)
def test_scripted_cause_has_the_known_answer(gpu, wt, packing, n, interval):
    """An injection program holds the outlet analyser's reading at 1.25 and drops it out during scans 3 ... 8.  Slot 0 ramps the acid word
    from the master's 0.5 towards 1.0 at 1/128 per second after a reaction time of two scans: it engages at scan 5 and
    owns scans 5 ... 8; slot 1 holds the chlorine word at the master's 0.25 at once, scans 3 ... 8.  Both release at
    scan 9, the first clear one.  All numbers are dyadic, in float32 too; nothing here comes from the restatement.  The
    instrument's own fault codes are causes as well, and an injected value leaves them alone: the answer is asserted for
    the reactors whose analyser reported none at any scan (the history says which)."""
    W, scans = interval * DT, 12
    R, N, cols, bc = ensemble(wt, n)
    ens = packing.place(plant(wt, cols, bc, n, history=scans * interval))
    ens.set_schedule(0, interval)
    ens.write_commands(*MASTER)
    ens.set_injections(wt.Injection("chlorine_outlet", "constant", a=1.25), wt.Injection("chlorine_outlet", "dropout", start=3 * W, end=9 * W))
    ens.set_responses(wt.Response("bad", "chlorine_outlet", "acid", action="ramp", value=1.0, rate=1.0 / 128.0, delay=2 * W),
                      wt.Response("bad", "chlorine_outlet", "chlorine", action="hold"))
    assert ens.info(gpu.WT_INFO_RESPOND) == 1
    ens.step(DT, n_steps=scans * interval, download=False)
    packing.check(ens)
    st = ens.response_state()
    _, _, fault, filled = ens.sensor_history()
    assert np.all(filled == scans * interval)
    at_scans = slice(interval - 1, None, interval)
    clean = ~fault[at_scans, 3].astype(bool).any(axis=0)
    print("n", n, "interval", interval, "clean", int(clean.sum()), "of", N)
    assert clean.sum() >= N - 4 and clean[:R].any() and clean[-1:].any()
    ones = np.ones(int(clean.sum()))
    step = W / 128.0
    ramp = [min(1.0, 0.5 + step * (k + 1)) for k in range(4)]
    nan = np.nan
    want = dict(phase=(0, 0), pending=(nan, nan), clearing=(nan, nan), output=(ramp[3], 0.25), t_first=(5 * W, 3 * W),
                t_engaged=(5 * W, 3 * W), t_released=(9 * W, 9 * W), n_engaged=(1, 1), time_engaged=(4 * W, 6 * W), n_owned=(4, 6),
                n_blocked=(0, 0), n_cause=(6, 6), n_tracked=(0, 0), n_handback=(0, 0))
    for name, (a, b) in want.items():
        got = getattr(st, name)
        assert_equal_by_reactor((a * ones, b * ones), (got[0][clean], got[1][clean]), (name, n, interval), R)
    assert np.array_equal(st.owner_chlorine[clean], -ones) and np.array_equal(st.owner_acid[clean], -ones)
    assert np.array_equal(st.t_prev, np.full(N, scans * W)) and not st.n_engaged[2:].any()
    hr = holding_words(ens)
    assert np.array_equal(hr[clean, 0:2], np.broadcast_to(float32_words(ramp[3]), (len(ones), 2)))
    assert np.array_equal(hr[clean, 2:4], np.broadcast_to(float32_words(0.25), (len(ones), 2)))
    assert np.array_equal(ens.boundary()[4, clean], ramp[3] * ones)      # the last word has reached the plant
    ens.close()


@pytest.mark.parametrize("interval", INTERVALS)
@pytest.mark.parametrize("n", ZONES)
def test_fused_call_equals_the_host_master(gpu, wt, packing, n, interval):
    """The host master: calls of one scan interval, the words of the restatements written before each, their scan after
    each -- tuner, response, controller, PI, alarm and detector in HostScan, the injection program on both devices.  Two
    reactors never step (a non-finite state) and one stops half way (a zone above 100 degC), on both sides.  The script
    (tests/respond_cases.py) varies every parameter by reactor: all three causes; delays of 0, one and several scans
    and two never reached; all three actions; latched and unlatched slots; both hand-backs; two slots on one loop; a
    loop under a relay experiment; a loop under a model predictive controller."""
    STEPS, STOP_AT = SCANS * interval, (SCANS // 2) * interval
    R, N, cols, bc = ensemble(wt, n, seed=1)
    sc = Scenario(wt, N, interval * DT)
    never, stopped = np.array([1, min(R + 2, N - 2)]), np.array([4])

    def start(ens):
        packing.place(ens)
        ens.set_schedule(0, interval)
        s = ens.state
        pH = s.pH.copy()
        pH[never, 0] = np.nan
        ens.set_state(pH, s.chlorine, s.temperature)

    def stop(ens):
        s = ens.state
        T = s.temperature.copy()
        T[stopped, 0] = 150.0
        ens.set_state(s.pH, s.chlorine, T)

    twin = plant(wt, cols, bc, n)
    start(twin)
    sc.device(twin, respond=False, around=False)
    hs, refs = sc.host(HostScan, words, DT)
    t_before, done = np.zeros(N), 0
    for c in hs.calls(STEPS, interval):
        if done == STOP_AT:
            stop(twin)
        w = hs.holding()
        twin.write_holding(w)
        twin.step(DT, n_steps=c, download=False)
        done += c
        t_now = twin.state.time
        stepped = t_now != t_before
        t_before = t_now
        v, _, f = twin.sensor_readings()
        hs.scan(v, f, commands(w), stepped)
    want = plant_state(twin) + twin.input_image() + (refs["ctl"].holding,)
    twin.close()
    ens = plant(wt, cols, bc, n)
    start(ens)
    sc.device(ens)
    ens.step(DT, n_steps=STOP_AT, download=False)
    stop(ens)
    ens.step(DT, n_steps=STEPS - STOP_AT, download=False)
    packing.check(ens)
    got_st, got_rst = responses(ens)
    params = ens.response_params()
    # no vacuous pass: from the device's own state
    not_vacuous(params, got_st, (n, interval))
    assert_all_equal((sc.blocks["respond"],), (params,), "params")
    rsp = refs["rsp"]
    assert_equal_by_reactor(want, observed(ens), ("plant", n, interval), R)
    assert_equal_by_reactor((rsp.st, rsp.rst), (got_st, got_rst), ("response", n, interval), R)
    assert_equal_by_reactor(ref_around(refs), around(ens), ("PI, controller, tuner, alarm, detector", n, interval), R)
    es = ens.state
    ens.close()
    took = np.full(N, float(STEPS))
    took[never], took[stopped] = 0.0, float(STOP_AT)
    assert np.array_equal(es.time, took * DT)
    assert not got_st[:, RR.RS_N_CAUSE][:, never].any() and np.isnan(got_st[:, RR.RS_PENDING][:, never]).all()
    assert np.all(got_rst[RR.RR_T_PREV][stopped] == STOP_AT * DT) and got_st[:, RR.RS_N_CAUSE][:, stopped].any()
    r = sc.r
    through = took == STEPS
    print("n", n, "interval", interval, "engagements by slot", got_st[:, RR.RS_N_ENGAGED].sum(axis=1).tolist(), "blocked",
          int(got_st[:, RR.RS_N_BLOCKED].sum()), "tracked", int(got_st[:, RR.RS_N_TRACKED].sum()), "hand-backs",
          got_st[:, RR.RS_N_HANDBACK].sum(axis=1).tolist())
    # delays reached and not reached (an analyser in fault makes the alarm's reading bad, which holds the alarm: counted
    # by reactor); latched slots stand at the end
    assert (through & (r % 5 >= 3) & (got_st[0, RR.RS_N_ENGAGED] == 0) & (got_st[0, RR.RS_N_CAUSE] > 0)).sum() >= 2
    for g in range(3):
        assert (through & (r % 5 == g) & (got_st[0, RR.RS_N_ENGAGED] > 0)).any(), g
    assert (through & (r % 3 == 0) & (got_st[3, RR.RS_PHASE] == 1)).any()
    assert (through & (r % 3 != 0) & (got_st[3, RR.RS_N_ENGAGED] > 0) & (got_st[3, RR.RS_PHASE] == 0)).any()
    assert (got_st[0, RR.RS_N_HANDBACK] > 0).any() and (got_st[2, RR.RS_N_HANDBACK] > 0).any()
    assert (refs["mpc"].st[0, 13][r % 4 == 3] > 0).any() and (got_st[0, RR.RS_N_BLOCKED][r % 4 == 2] > 0).any()


def test_lifecycle(gpu, wt, packing):
    L = gpu.lib()
    n, W = 8, DT
    R, N, cols, bc = ensemble(wt, n, seed=3)
    slot = wt.Response("bad", "chlorine_outlet", "chlorine", action="manual", value=0.5, latch=True)
    block = wt.response_block(N, slot)
    ens = packing.place(wt.ReactorEnsemble(cols, n_zones=n))
    ens.set_boundary(bc)
    assert ens.info(gpu.WT_INFO_RESPOND) == 0
    ens.enable_sensors(seed=4)                                  # the sensor suite alone is not what a response needs
    assert L.wt_ensemble_respond_set(ens._h, gpu.dptr(block)) == gpu.WT_E_STATE
    assert L.wt_last_error().decode() == "response programs act on the plant I/O scan: enable plant I/O first"
    with pytest.raises(ValueError, match="plant I/O"):
        ens.set_responses(slot)
    ens.enable_plant_io()
    ens.set_schedule(0, 1)
    ens.clear_responses()                                       # no effect while none is set
    for call in (ens.response_state, ens.response_params, ens.reset_responses):
        with pytest.raises(ValueError, match="no response program is set"):
            call()
    bad = block.copy()
    bad[0, RR.R_VALUE, N - 1] = 1.5
    assert L.wt_ensemble_respond_set(ens._h, gpu.dptr(bad)) == gpu.WT_E_ARG
    msg = L.wt_last_error()
    assert L.wt_respond_check(N, gpu.dptr(bad)) == gpu.WT_E_ARG and L.wt_last_error() == msg
    assert msg.decode() == f"value must be within 0 and the loop's command limit (1.0 chlorine, 2.0 acid) (slot 0, reactor {N - 1})"
    assert ens.info(gpu.WT_INFO_RESPOND) == 0
    ens.write_commands(*MASTER)
    ens.set_injections(wt.Injection("chlorine_outlet", "constant", a=1.25), wt.Injection("chlorine_outlet", "dropout", start=3 * W, end=5 * W))
    pi = wt.PILoop("chlorine_outlet", setpoint=1.5, kp=0.3, ki=1e-3, bias=0.2)
    ens.enable_control(pi)
    ens.set_responses(slot)
    assert ens.info(gpu.WT_INFO_RESPOND) == 1
    fresh = RR.RespondRef(block, np.zeros(N))
    assert_all_equal((fresh.st, fresh.rst), responses(ens), "state at set")
    assert_all_equal((block,), (ens.response_params(),), "params")
    only = np.empty((3, N))
    gpu.check(L.wt_ensemble_respond_state(ens._h, None, gpu.dptr(only)))
    assert np.array_equal(only, fresh.rst)
    ens.step(DT, n_steps=10, download=False)
    st = ens.response_state()
    assert np.all(st.phase[0] == 1) and np.all(st.n_owned[0] >= 8) and np.all(st.owner_chlorine == 0)    # latched: it stands
    hr = holding_words(ens)
    assert np.array_equal(hr[:, 2:4], np.broadcast_to(float32_words(0.5), (N, 2)))
    held = ens.control_state().chlorine
    assert np.all(held.n_exec + held.n_held == 10 - st.n_owned[0])           # the PI ran only before the engagement
    # reset: every slot idle again, the latched one included, the words kept; the PI resumes
    ens.reset_responses()
    again = RR.RespondRef(block, np.full(N, 10 * DT))
    assert_all_equal((again.st, again.rst), responses(ens), "state at reset")
    assert np.array_equal(holding_words(ens), hr)
    ens.step(DT, n_steps=3, download=False)
    now = ens.control_state().chlorine
    idle = ens.response_state().n_engaged[0] == 0               # (an analyser in fault of its own is a cause again)
    assert idle.sum() >= N - 4 and np.all((now.n_exec + now.n_held)[idle] == (held.n_exec + held.n_held)[idle] + 3)
    # set over a program in force replaces it and restarts; clear switches it off and leaves the words
    ens.set_responses(wt.Response("bad", "chlorine_outlet", "acid"))
    assert ens.response_params()[0, RR.R_LOOP].all() and not ens.response_state().n_cause.any()
    hr = holding_words(ens)
    ens.clear_responses()
    assert ens.info(gpu.WT_INFO_RESPOND) == 0 and np.array_equal(holding_words(ens), hr)
    with pytest.raises(ValueError, match="no response program is set"):
        ens.response_state()
    ens.step(DT, n_steps=2, download=False)
    packing.check(ens)
    ens.close()
    # 33 zones and more: the n > 32 kernel carries no program
    cfg = wt.ReactorConfiguration(n_zones=33)
    big = wt.ReactorEnsemble([cfg, cfg]); big.set_boundary(wt.BoundaryConditions())
    big.enable_sensors(seed=3); big.enable_plant_io()
    small = wt.response_block(2, slot)
    assert L.wt_ensemble_respond_set(big._h, gpu.dptr(small)) == gpu.WT_E_STATE
    assert L.wt_last_error().decode() == "response programs run in the kernels for up to 32 zones"
    assert big.info(gpu.WT_INFO_RESPOND) == 0
    big.close()


@pytest.mark.parametrize("n", ZONES)
def test_every_slot_off_equals_no_program_equals_plant_io_alone(gpu, wt, packing, n):
    """Beside a running PI program: a response program whose slots are all off against none, bit for bit; and without
    any program, plant I/O with the switch on against plant I/O alone."""
    R, N, cols, bc = ensemble(wt, n, seed=5)
    pi = wt.PILoop("chlorine_outlet", setpoint=np.asarray(cols["initial_chlorine"]) + 2.0, kp=0.3, ki=1e-3, bias=0.2)
    off = wt.Response("off", 0, "acid", action="manual", value=1.0)
    out = {}
    for controlled in (True, False):
        for program in (False, True):
            ens = packing.place(plant(wt, cols, bc, n))
            ens.set_schedule(0, 1)
            ens.write_commands(*MASTER)
            if controlled:
                ens.enable_control(pi)
            if program:
                ens.set_responses(off, off)
                assert ens.info(gpu.WT_INFO_RESPOND) == 1
            ens.step(DT, n_steps=40, download=False)
            out[controlled, program] = observed(ens) + ((ens.control_state().block(),) if controlled else ())
            if program:
                st, rst = responses(ens)
                idle = RR.RespondRef(ens.response_params(), np.zeros(N))
                assert np.array_equal(st, idle.st, equal_nan=True) and np.array_equal(rst[1:], idle.rst[1:])
                assert np.array_equal(rst[0], ens.state.time)      # t_prev alone moves
                packing.check(ens)
            ens.close()
    assert_equal_by_reactor(out[True, False], out[True, True], "slots off beside a PI", R)
    assert_equal_by_reactor(out[False, False], out[False, True], "slots off on plant I/O alone", R)


def test_checkpoints_carry_a_response_mid_engagement(gpu, wt, packing):
    """Saved while slots are engaged: the restored handle, the clone and a mark / rewind each continue with the bits of
    the handle that was never saved, response state and parameters included."""
    n = 5
    R, N, cols, bc = ensemble(wt, n, seed=4)
    sc = Scenario(wt, N, DT)

    def fresh():
        ens = packing.place(plant(wt, cols, bc, n))
        ens.set_schedule(0, 1)
        sc.device(ens)
        return ens

    def full(ens):
        return observed(ens) + responses(ens) + (ens.response_params(),) + around(ens)

    SAVE, REST = 13, SCANS - 13
    never = fresh(); never.step(DT, n_steps=SAVE, download=False); never.step(DT, n_steps=REST, download=False)
    want = full(never); never.close()
    a = fresh(); a.step(DT, n_steps=SAVE, download=False)
    mid = responses(a)
    assert (mid[0][0, RR.RS_PHASE] == 1).any() and (mid[0][2, RR.RS_PHASE] == 1).any() and (mid[0][:, RR.RS_PENDING] > 0).any()
    assert (mid[1][RR.RR_OWNER_CHLORINE] >= 0).any() and (mid[1][RR.RR_OWNER_ACID] == 2).any()
    blob = a.checkpoint()
    bare = wt.ReactorEnsemble(cols, n_zones=n); bare.set_boundary(bc)
    no_io = bare.checkpoint()
    b = plant(wt, cols, bc, n, seed=1); b.restore(blob)
    c = a.clone()
    a.mark()
    for name, ens in (("original", a), ("restored", b), ("clone", c)):
        assert ens.info(gpu.WT_INFO_RESPOND) == 1
        ens.step(DT, n_steps=REST, download=False)
        assert_equal_by_reactor(want, full(ens), name, R)
    a.rewind()
    assert_all_equal(mid, responses(a), "rewound state")
    a.step(DT, n_steps=REST, download=False)
    assert_equal_by_reactor(want, full(a), "rewound", R)
    packing.check(a)
    not_vacuous(a.response_params(), responses(a)[0], "checkpoints")
    # a blob taken without plant I/O takes the program away
    b.restore(no_io)
    assert b.info(gpu.WT_INFO_RESPOND) == 0 and b.info(gpu.WT_INFO_PLANT_IO) == 0
    b.enable_sensors(seed=2); b.enable_plant_io()
    assert b.info(gpu.WT_INFO_RESPOND) == 0
    with pytest.raises(ValueError, match="no response program is set"):
        b.response_state()
    for ens in (a, b, c, bare):
        ens.close()
