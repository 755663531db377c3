"""Per-reactor link programs at the PLC scans (include/wtphys.h ``wt_ensemble_link_*``): a scripted delay and replay
with their exact answers, a fused call against the host master it replaces (tests/link_ref.py) beside injection, PI,
controller, detector and response programs, a wired remote analyser behind a link, the lifecycle and the checkpoints.
Shapes: five wavefront-groups plus one reactor at n = 8 (row mode), 5 (non-row) and 20, and 33 reactors of 2 zones, each
with the library's own spreading and with full wavefronts, a scan every step and every third step."""
import ctypes

import numpy as np
import pytest

import link_ref as LR
import plc_oracle as PO
from checkpoint_helpers import holding_words
from control_ref import ControlRef
from link_cases import MASTER, SCANS, SEED, Scenario, not_vacuous
from program_helpers import (DT, HostScan, assert_all_equal, assert_equal_by_reactor, packing, plant, plant_state,  # noqa: F401
                             ragged_size, words)
from wire_ref import WireRef, WireScan, host_wired_loop, took_the_step

pytestmark = pytest.mark.gpu

ZONES = (8, 5, 20, 2)
INTERVALS = (1, 3)
FLOW, T_IN = 4, 5
REG = {FLOW: 10, T_IN: 12}            # first input register of the two linked instruments


def ensemble(wt, n, seed=0):
    R, N = (32, 33) if n == 2 else ragged_size(n)
    cols, bc = wt.make_ensemble(N, seed=6300 + n + seed)
    return R, N, cols, bc


def image_of(values, faults, sim_time):
    """What update_modbus_inputs leaves in the device's image layout, from the oracle: (N, 20) words, update_ok (N,)."""
    N = values.shape[1]
    img, ok = np.zeros((N, 20), dtype=np.uint16), np.zeros(N, dtype=bool)
    for r in range(N):
        io = PO.PlantIO()
        ok[r] = io.update_inputs([float(x) for x in values[:, r]], [int(x) for x in faults[:, r]], float(sim_time[r]))
        img[r, :16], img[r, 16:19] = io.ir[:16], io.ir[100:103]
        img[r, 19] = io.di[0] | (io.di[1] << 1) | (io.di[2] << 2)
    return img, ok


def observed(ens):
    """State, readings, boundary, input image and holding image of every reactor."""
    return plant_state(ens) + ens.input_image() + (holding_words(ens),)


def links(ens):
    """Parameters, state and the rings in recording order."""
    return (ens.link_params(), ens.link_state().block()) + tuple(ens.link_ring())


def around(ens):
    """Injection, PI, controller, detector and response state."""
    return ((ens.injection_state().block(), ens.control_state().block(), ens.mpc_state().block(), ens.mpc_prediction())
            + tuple(ens.detector_state().block()) + tuple(ens.response_state().block()))


def ref_around(refs):
    det, rsp = refs["det"], refs["rsp"]
    return (refs["inj"].st, refs["ctl"].st, refs["mpc"].st, refs["mpc"].pred, det.st, det.t_prev, rsp.st, rsp.rst)


def word_value(x):
    """The float32 the image carries for a reading: NaN and the infinities become 0.0."""
    x = np.asarray(x, dtype=np.float32)
    return np.where(np.isfinite(x), x, np.float32(0.0))


@pytest.mark.parametrize("interval", INTERVALS)
@pytest.mark.parametrize("n", ZONES)
def test_scripted_delay_and_replay_have_their_exact_answers(gpu, wt, packing, n, interval):
    """Slot 0 delays the flow meter by three scans from the first scan on; slot 1 replays the inlet thermometer's scans
    1 ... 4 during scans 5 ... 9 (the window [6 W, 11 W)) and is live again at scan 10.  The sensor history holds what
    the instruments read at every step: the image word of scan k is the flow meter's reading of scan max(k - 3, 0) and
    the thermometer's of scan 1 + (k - 5) % 4, the rings hold the history's samples in order, and the counters are the
    numbers of scans.  Nothing here comes from the restatement.  Eight scans in one call, then four calls of a scan."""
    W, scans = interval * DT, 12
    R, N, cols, bc = ensemble(wt, n)
    ens = packing.place(plant(wt, cols, bc, n, history=scans * interval))
    ens.set_schedule(0, interval)
    ens.write_commands(*MASTER)
    ens.set_links(wt.Link.delay("flow_main", 3), wt.Link.replay("temp_inlet", 4, start=6 * W, end=11 * W))
    assert ens.info(gpu.WT_INFO_LINK) == 1
    ens.step(DT, n_steps=8 * interval, download=False)
    seen = {}
    for k in range(8, scans):
        ens.step(DT, n_steps=interval, download=False)
        img, ok = ens.input_image()
        assert ok.all()
        seen[k] = {s: wt.ReactorEnsemble.decode_float32(img[:, REG[s]:REG[s] + 2]) for s in REG}
    packing.check(ens)
    vh, _, fh, filled = ens.sensor_history()
    assert np.all(filled == scans * interval)
    at = lambda k: (k + 1) * interval - 1                                  # the step that scan k closes
    for k in range(8, scans):
        assert_equal_by_reactor((word_value(vh[at(k - 3), FLOW]),), (seen[k][FLOW],), ("delayed flow", n, interval, k), R)
        src = 1 + (k - 5) % 4 if k < 10 else k
        assert_equal_by_reactor((word_value(vh[at(src), T_IN]),), (seen[k][T_IN],), ("replayed temperature", n, interval, k), R)
    assert any((seen[k][FLOW] != word_value(vh[at(k), FLOW])).any() for k in seen)        # the delay shows
    st = ens.link_state()
    ones = np.ones(N)
    nan = np.nan
    want = dict(n_rec=(12, 7), n_applied=(12, 5), n_fresh=(12, 5), n_lost=(0, 0), n_timeout=(0, 0), n_draw=(0, 0),
                t_fresh=(12 * W, 12 * W), held_fault=(fh[at(8), FLOW].astype(float), fh[at(11), T_IN].astype(float)), tape_end=(nan, nan))
    for name, (a, b) in want.items():
        got = getattr(st, name)
        assert_equal_by_reactor((a * ones, b * ones), (got[0], got[1]), (name, n, interval), R)
    assert_equal_by_reactor((vh[at(8), FLOW].astype(np.float64), vh[at(11), T_IN].astype(np.float64)), (st.held_value[0], st.held_value[1]),
                            ("held", n, interval), R)
    values, faults, n_rec = ens.link_ring()
    every = [at(k) for k in range(scans)]
    taped = [at(k) for k in (0, 1, 2, 3, 4, 10, 11)]
    assert_equal_by_reactor((vh[every, FLOW].astype(np.float64), fh[every, FLOW].astype(np.float64), vh[taped, T_IN].astype(np.float64),
                             fh[taped, T_IN].astype(np.float64)),
                            (values[0, :12], faults[0, :12], values[1, :7], faults[1, :7]), ("rings", n, interval), R)
    assert np.isnan(values[0, 12:]).all() and np.isnan(values[1, 7:]).all() and not faults[0, 12:].any()
    assert np.array_equal(n_rec[:2], np.array([[12.0], [7.0]]) * ones) and np.all(n_rec[2:] == 12)   # slots that are off record too
    ens.close()


@pytest.mark.parametrize("interval", INTERVALS)
@pytest.mark.parametrize("n", ZONES)
def test_fused_call_equals_the_host_master(gpu, wt, packing, n, interval):
    """The host master: a handle with plant I/O alone, calls of one scan interval, before each the words that the
    restated link and injection leave of the controllers' words, after each the restated scan of ``sensor_readings()``
    -- link, injection, response, controller, PI and detector in HostScan.  Two reactors never step (a non-finite state)
    and one stops half way (a zone above 100 degC), on both sides.  The script (tests/link_cases.py) has all three modes
    on reading and command channels, delays of 0, 1, 3 and 63 scans, jitter, loss of 0, 0.5 and 1, a timeout that is
    reached and one that is not, two slots chained on one channel and an injection on the same channel."""
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
    twin.write_commands(*MASTER)
    first_img = twin.input_image()
    hs, refs = sc.host(HostScan, words, DT)
    taking = np.ones(N, dtype=bool)
    taking[never] = False
    seen_v, seen_f, seen_t = np.zeros((7, N), dtype=np.float32), np.zeros((7, N), dtype=np.int64), np.zeros(N)
    t_before, done = np.zeros(N), 0
    moved = np.zeros(N, dtype=bool)                 # the flow meter's image left its valid field reading inside the replay window
    for c in hs.calls(STEPS, interval):
        if done == STOP_AT:
            stop(twin)
            taking[stopped] = False
        hs.inj.stepped = taking                     # the command path of this call's scan, emulated in the words
        twin.write_holding(hs.holding())
        twin.step(DT, n_steps=c, download=False)
        done += c
        t_now = twin.state.time
        stepped = t_now != t_before
        t_before = t_now
        assert np.array_equal(stepped, taking), done
        v, _, f = twin.sensor_readings()
        vt, ft = hs.scan(v, f, None, stepped)
        seen_v[:, stepped], seen_f[:, stepped], seen_t[stepped] = vt[:, stepped], ft[:, stepped], (hs.lt - DT)[stepped]
        valid = stepped & np.isfinite(v[FLOW]) & np.isfinite(vt[FLOW]) & (f[FLOW] == 0) & (ft[FLOW] == 0)
        with np.errstate(invalid="ignore"):
            moved |= valid & (hs.lt >= sc.labels[0]) & (hs.lt < sc.labels[1]) & (np.abs(vt[FLOW].astype(np.float64) - v[FLOW]) >= 0.01)
    lnk = refs["lnk"]
    # the script alone shows every branch, on the restatement ...
    not_vacuous(lnk.p, lnk.st, ("restated", n, interval))
    want_img, want_ok = image_of(seen_v, seen_f, seen_t)
    want_img[never], want_ok[never] = first_img[0][never], first_img[1][never]
    want = plant_state(twin) + (want_img, want_ok, refs["ctl"].holding)
    twin.close()
    ens = plant(wt, cols, bc, n)
    start(ens)
    sc.device(ens)
    ens.step(DT, n_steps=STOP_AT, download=False)
    stop(ens)
    ens.step(DT, n_steps=STEPS - STOP_AT, download=False)
    packing.check(ens)
    params, got_st, got_v, got_f, got_n = links(ens)
    # ... and on the device's own state, before anything is compared
    not_vacuous(params, got_st, ("device", n, interval))
    det, rsp = ens.detector_state(), ens.response_state()
    through = taking & sc.replayed
    print("n", n, "interval", interval, "applied", got_st[:, LR.LS_N_APPLIED].sum(axis=1).tolist(), "lost", got_st[:, LR.LS_N_LOST].sum(axis=1).tolist(),
          "timeouts", got_st[:, LR.LS_N_TIMEOUT].sum(axis=1).tolist(), "detector raised in", int((det.n_raise[0][through] > 0).sum()), "of",
          int(through.sum()), "response engaged in", int((rsp.n_engaged[0] > 0).sum()))
    # (a flow meter out of its range reports a fault, which the detector holds on: the reactors whose valid image left
    # the valid field reading by ten sigma inside the window are the ones that must have fired)
    assert moved[through].sum() >= through.sum() // 3 and (det.n_tp[0][through & moved] > 0).all(), "the IMAGE-against-FIELD detector fires under REPLAY"
    even = taking & (sc.r % 2 == 0)
    # (an instrument's own fault just before the timeout engages the slot earlier: counted by reactor)
    assert np.mean(rsp.t_engaged[0][even] == 34 * sc.W) > 0.8 and np.all(rsp.n_engaged[0][even] > 0), "the BAD cause is the timed-out reading"
    assert_all_equal((sc.blocks["link"],), (params,), "params")
    assert_equal_by_reactor(want, observed(ens), ("plant", n, interval), R)
    assert_equal_by_reactor((lnk.st,) + lnk.in_order(), (got_st, got_v, got_f, got_n), ("link", n, interval), R)
    assert_equal_by_reactor(ref_around(refs), around(ens), ("injection, PI, controller, detector, response", n, interval), R)
    es = ens.state
    ens.close()
    took = np.full(N, float(STEPS))
    took[never], took[stopped] = 0.0, float(STOP_AT)
    assert np.array_equal(es.time, took * DT)
    assert not got_st[:, :LR.LS_T_FRESH][:, :, never].any() and np.isnan(got_st[:, LR.LS_T_FRESH][:, never]).all()
    assert np.all(got_st[:, LR.LS_N_REC][:, stopped] <= SCANS // 2) and got_st[:, LR.LS_N_REC][:, stopped].all()


@pytest.mark.parametrize("interval", INTERVALS)
def test_a_wired_remote_analyser_behind_a_link(gpu, wt, interval):
    """Trains of two tanks: the first stage's PI doses on the second stage's flow meter, which reaches it over a wire and
    then a link that delays it by two scans (even trains) or loses every other poll at random (odd trains).  The host
    loop routes, links and controls; the fused call gives its bits."""
    n, L, K = 8, 2, 24 * interval
    N = 5 * 8 + L
    cols, bc = wt.make_ensemble(N, seed=6400 + interval)
    train = np.arange(N) // L
    wires = (wt.Wire("flow_main", 0, 1),)
    loop = wt.PILoop("flow_main", setpoint=6.0, kp=0.25, ki=1.0 / 1024.0, bias=0.25)
    link = wt.Link("flow_main", np.where(train % 2 == 0, 1, 2), start=4 * interval * DT, a=np.where(train % 2 == 0, 2.0, 0.5))

    def start():
        ens = plant(wt, cols, bc, n)
        ens.set_schedule(0, interval)
        ens.set_trains(L, linked=False)
        return ens

    a = start()
    a.enable_control(chlorine=loop)
    a.set_wires(*wires)
    a.set_links(link, seed=SEED)
    a.step(DT, n_steps=K, download=False)
    b = start()
    ctl, wir = ControlRef(wt.control_block(N, loop, None), np.zeros(N)), WireRef(wt.wire_block(N, L, *wires), L)
    lnk = LR.LinkRef(wt.link_block(N, link), seed=SEED)
    hs = WireScan(N, wir, ctl=ctl, inj=LR.LinkThenInject(lnk), emulated=True)
    v, f, t = host_wired_loop(b, hs, K, interval)
    assert_all_equal(plant_state(b), plant_state(a), "wired and linked")
    b.close()
    assert np.array_equal(a.control_state().block(), ctl.st) and np.array_equal(a.wire_state().block(), wir.state())
    assert_all_equal((lnk.st,) + lnk.in_order(), links(a)[1:], "link behind the wire")
    first = np.arange(N) % L == 0
    assert lnk.st[0, LR.LS_N_LOST][first & (train % 2 == 1)].any() and np.all(lnk.st[0, LR.LS_N_APPLIED] == 24 - 3)
    live = took_the_step(a.status())
    img, ok = a.input_image()
    want_img, want_ok = image_of(v[:, live], f[:, live], t[live])
    assert live.all() and np.array_equal(img[live], want_img) and np.array_equal(ok[live], want_ok)
    a.close()


def test_lifecycle(gpu, wt, packing):
    L = gpu.lib()
    n, W = 8, DT
    R, N, cols, bc = ensemble(wt, n, seed=3)
    slots = (wt.Link.delay("flow_main", 2), wt.Link.loss("acid_flow_rate", 1.0, start=4 * W, timeout=2 * W, fail=0.125))
    block = wt.link_block(N, *slots)
    ens = packing.place(wt.ReactorEnsemble(cols, n_zones=n))
    ens.set_boundary(bc)
    assert ens.info(gpu.WT_INFO_LINK) == 0
    ens.enable_sensors(seed=4)                                  # the sensor suite alone is not what a link needs
    assert L.wt_ensemble_link_set(ens._h, gpu.dptr(block), 0) == gpu.WT_E_STATE
    assert L.wt_last_error().decode() == "link programs act on the plant I/O scan: enable plant I/O first"
    with pytest.raises(ValueError, match="plant I/O"):
        ens.set_links(*slots)
    ens.enable_plant_io()
    ens.set_schedule(0, 1)
    ens.clear_links()                                           # no effect while none is set
    for call in (ens.link_state, ens.link_params, ens.link_ring, ens.reset_links):
        with pytest.raises(ValueError, match="no link program is set"):
            call()
    bad = block.copy()
    bad[1, LR.L_A, N - 1] = 1.5
    assert L.wt_ensemble_link_set(ens._h, gpu.dptr(bad), 0) == gpu.WT_E_ARG
    msg = L.wt_last_error()
    assert L.wt_link_check(N, gpu.dptr(bad)) == gpu.WT_E_ARG and L.wt_last_error() == msg
    assert msg.decode() == f"a LOSS slot's probability (a) must be within 0 and 1 (slot 1, reactor {N - 1})"
    assert ens.info(gpu.WT_INFO_LINK) == 0
    ens.write_commands(*MASTER)
    ens.set_links(*slots, seed=SEED)
    assert ens.info(gpu.WT_INFO_LINK) == 1
    fresh = LR.LinkRef(block)
    assert_all_equal((block, fresh.st) + fresh.in_order(), links(ens), "state at set")
    seed = ctypes.c_uint64(0)
    gpu.check(L.wt_ensemble_link_params(ens._h, None, ctypes.byref(seed)))
    assert seed.value == SEED
    ens.step(DT, n_steps=10, download=False)
    st = ens.link_state()
    assert np.all(st.n_rec == 10) and np.all(st.n_applied[0] == 10) and np.all(st.n_applied[1] == 7) and np.all(st.n_timeout[1] == 5)
    assert np.all(st.t_fresh[1] == 3 * W) and np.all(st.held_value[1] == 0.5)
    assert np.array_equal(ens.boundary()[4], np.full(N, 0.125))                  # the fail-safe has reached the plant
    assert np.array_equal(holding_words(ens)[:, 0:2], np.broadcast_to(words(np.array([[0.5], [0.0], [0.0]]))[0, 0:2], (N, 2)))   # the image is the master's
    # reset: state and rings as set left them, parameters and seed kept; the window is still open, so the held command
    # is the first sample after the reset and the timeout runs again from there
    ens.reset_links()
    assert_all_equal((block, fresh.st) + fresh.in_order(), links(ens), "state at reset")
    ens.step(DT, n_steps=4, download=False)
    st = ens.link_state()
    assert np.all(st.n_rec == 4) and np.all(st.n_lost[1] == 4) and np.all(st.n_fresh[1] == 1) and np.all(st.n_timeout[1] == 1)
    assert np.all(st.t_fresh[1] == 11 * W)
    # set over a program in force replaces it and restarts; clear switches it off
    ens.set_links(wt.Link.replay("temp_inlet", 3, start=1e9))
    assert np.all(ens.link_params()[0, LR.L_MODE] == LR.REPLAY) and not ens.link_state().n_rec.any()
    ens.clear_links()
    assert ens.info(gpu.WT_INFO_LINK) == 0
    with pytest.raises(ValueError, match="no link program is set"):
        ens.link_state()
    ens.step(DT, n_steps=2, download=False)
    assert np.array_equal(ens.boundary()[4], np.full(N, 0.5))                    # the master's command again
    packing.check(ens)
    ens.close()
    # 33 zones and more: the n > 32 kernel carries no program
    cfg = wt.ReactorConfiguration(n_zones=33)
    big = wt.ReactorEnsemble([cfg, cfg]); big.set_boundary(wt.BoundaryConditions())
    big.enable_sensors(seed=3); big.enable_plant_io()
    small = wt.link_block(2, *slots)
    assert L.wt_ensemble_link_set(big._h, gpu.dptr(small), 0) == gpu.WT_E_STATE
    assert L.wt_last_error().decode() == "link programs run in the kernels for up to 32 zones"
    assert big.info(gpu.WT_INFO_LINK) == 0
    big.close()


@pytest.mark.parametrize("n", ZONES)
def test_every_slot_off_equals_no_program_equals_plant_io_alone(gpu, wt, packing, n):
    """Beside a running PI program: a link program whose slots are all off, and one whose windows never open, against
    none, bit for bit; and without any program, plant I/O with the switch on against plant I/O alone."""
    R, N, cols, bc = ensemble(wt, n, seed=5)
    pi = wt.PILoop("flow_main", setpoint=6.0, kp=0.3, ki=1e-3, bias=0.2)
    off = wt.Link("chlorine_flow_rate", "off", start=0.0, end=1e9)
    never = (wt.Link.delay("flow_main", 5, start=1e9), wt.Link.loss("chlorine_flow_rate", 1.0, start=1e9, timeout=0.0, fail=0.5))
    out = {}
    for controlled in (True, False):
        for program in (None, "off", "never"):
            ens = packing.place(plant(wt, cols, bc, n))
            ens.set_schedule(0, 1)
            ens.write_commands(*MASTER)
            if controlled:
                ens.enable_control(pi)
            if program:
                ens.set_links(*((off, off) if program == "off" else never))
                assert ens.info(gpu.WT_INFO_LINK) == 1
            ens.step(DT, n_steps=40, download=False)
            out[controlled, program] = observed(ens) + ((ens.control_state().block(),) if controlled else ())
            if program:
                st = ens.link_state()
                assert np.all(st.n_rec == 40) and not st.n_applied.any() and np.array_equal(st.t_fresh, np.broadcast_to(ens.state.time, (4, N)))
                packing.check(ens)
            ens.close()
    for controlled in (True, False):
        for program in ("off", "never"):
            assert_equal_by_reactor(out[controlled, None], out[controlled, program], (program, "beside a PI" if controlled else "alone"), R)


def test_checkpoints_carry_a_link_mid_window(gpu, wt, packing):
    """Saved while the replay windows are open and a tape is running: the restored handle, the clone and a mark / rewind
    each continue with the bits of the handle that was never saved, link state, rings and parameters included."""
    n = 5
    R, N, cols, bc = ensemble(wt, n, seed=4)
    sc = Scenario(wt, N, DT)

    def fresh():
        ens = packing.place(plant(wt, cols, bc, n))
        ens.set_schedule(0, 1)
        sc.device(ens)
        return ens

    def full(ens):
        return observed(ens) + links(ens) + around(ens)

    SAVE, REST = 43, SCANS - 43
    never = fresh(); never.step(DT, n_steps=SAVE, download=False); never.step(DT, n_steps=REST, download=False)
    want = full(never); never.close()
    a = fresh(); a.step(DT, n_steps=SAVE, download=False)
    mid = links(a)
    st = mid[1]
    assert (st[0, LR.LS_TAPE_END] == 19).any() and (st[2, LR.LS_TAPE_END] == 39).any() and (st[1, LR.LS_N_TIMEOUT] > 0).any()
    blob = a.checkpoint()
    b = plant(wt, cols, bc, n, seed=1); b.restore(blob)
    c = a.clone()
    a.mark()
    for name, ens in (("original", a), ("restored", b), ("clone", c)):
        assert ens.info(gpu.WT_INFO_LINK) == 1
        ens.step(DT, n_steps=REST, download=False)
        assert_equal_by_reactor(want, full(ens), name, R)
    a.rewind()
    assert_all_equal(mid, links(a), "rewound link")
    a.step(DT, n_steps=REST, download=False)
    assert_equal_by_reactor(want, full(a), "rewound", R)
    packing.check(a)
    seed = ctypes.c_uint64(0)
    gpu.check(gpu.lib().wt_ensemble_link_params(b._h, None, ctypes.byref(seed)))
    assert seed.value == SEED                                   # the restored handle draws from the saved seed
    a.close(); b.close(); c.close()
