"""The wire program (include/wtphys.h ``wt_ensemble_wire_*``): a stage's PLC inputs wired to another stage's instruments
of the same train inside the step call.  The fused call gives the bits of the host loop -- a twin without the program,
calls of one scan interval, ``sensor_readings()`` routed by the restatement (wire_ref.py) and a host master -- at every
kernel instantiation that holds a train and both wavefront packings, whatever the schedule and the placement; an
all-own program and a cleared one are invisible; with every scan program on the device's state blocks are the
restatements'; a spoof lands at the receiver's slot, not at the source's; a stopped source is a dead loop; refusals and
lifetime.  The program only copies, so equality is bit for bit throughout."""
import numpy as np
import pytest

import actuator_ref as AR
import alarm_ref as LR
import detect_ref as KR
import trend_ref as TR
from control_ref import ControlRef
from inject_ref import InjectRef
from program_helpers import (DT, MASTER, acts, alarms, assert_all_equal, commands, full_waves, instantiation, pi_loops,  # noqa: F401
                             plant, plant_state, ref_acts, ref_alarms, words)
from test_gpu_inject import _image_of
from wire_ref import WireRef, WireScan, host_wired_loop, took_the_step

pytestmark = pytest.mark.gpu

E_FINITE = "wire parameters must be finite"
E_STAGE = "stage must be -1 (the reactor's own instrument) or a whole number in 0..length - 1 (a stage of the same train)"
E_SENSOR = "a wire's sensor must be a whole number in 0..6"
E_NO_TRAIN = "no train program is set (wt_ensemble_train_set)"
E_NO_IO = "wires carry readings into the plant I/O scan: enable plant I/O first"
E_NO_WIRE = "no wire program is set (wt_ensemble_wire_set)"
CL_OUT = 3                                         # chlorine_outlet, the slot most wires below end in
SHAPES = [(2, 4), (3, 2), (4, 3), (5, 5), (8, 2), (8, 8), (12, 2), (16, 2), (20, 3), (32, 2)]


def _wires(wt, N, L):
    """Dealt per train, in turn: the last stage's analyser to stage 0; a neighbour each way; the own stage with another
    sensor (and a second slot from the last stage); none."""
    t = np.arange(N // L) % 4
    return [wt.Wire("chlorine_outlet", 0, L - 1, trains=t == 0),
            wt.Wire("chlorine_outlet", 0, 1, trains=t == 1), wt.Wire("pH_outlet", L - 1, L - 2, trains=t == 1),
            wt.Wire("chlorine_outlet", L - 1, L - 1, source="chlorine_inlet", trains=t == 2),
            wt.Wire("flow_main", 0, L - 1, source="temp_outlet", trains=t == 2)]


def _start(wt, cols, bc, n, L, interval, pipes=None, adaptive=False, streams=0):
    ens = plant(wt, cols, bc, n)
    ens.set_placement(adaptive)
    ens.set_schedule(streams, interval)
    ens.write_commands(*MASTER)
    ens.set_trains(L)
    if pipes is not None:
        ens.set_pipes(pipes)
    return ens


def _seen(ens):
    """State, time, flow, status, readings and boundary, the solver counters and the input image."""
    return plant_state(ens) + (ens.solver_stats(),) + ens.input_image()


def _refused(fn, *args):
    with pytest.raises(ValueError) as ei:
        fn(*args)
    return str(ei.value)


def test_shapes_reach_every_instantiation_that_holds_a_train():
    assert {instantiation(n) for n, _ in SHAPES} == {(1, True), (2, False), (2, True), (3, False), (3, True), (4, False),
                                                     (4, True), (5, False)}
    assert all(2 <= L <= 64 // n for n, L in SHAPES)


# ---- 1. the fused call against the host loop, where the layout can go wrong
@pytest.mark.parametrize("full", [True, False], ids=["full_waves", "spread"])
@pytest.mark.parametrize("n, L", SHAPES)
def test_fused_equals_host_loop(gpu, wt, monkeypatch, n, L, full):
    if full:
        monkeypatch.setenv("WT_FULL_WAVES", "1")
    R = L * ((64 // n) // L) if full else L        # spread: a small ensemble gets one train per wavefront
    N, K, interval = 3 * R + L, 13, 3              # the last wavefront-group holds one train; scans at 3, 6, 9, 12, 13
    cols, bc = wt.make_ensemble(N, seed=300 + n + L)
    chlorine, acid = pi_loops(wt, cols)
    wires = _wires(wt, N, L)
    blk = wt.wire_block(N, L, *wires)
    pipes = np.arange(N) % 3                       # (the builder gives first stages 0)
    a = _start(wt, cols, bc, n, L, interval, pipes)
    a.enable_control(chlorine, acid)
    a.set_wires(*wires)
    assert a.train_state().per_wavefront == R and np.array_equal(a.wire_params(), blk)
    a.step(DT, n_steps=K, download=False)
    b = _start(wt, cols, bc, n, L, interval, pipes)
    ctl, ref = ControlRef(wt.control_block(N, chlorine, acid), np.zeros(N), holding=words(np.array(MASTER)[:, None].repeat(N, axis=1))), WireRef(blk, L)
    hs = WireScan(N, ref, ctl=ctl, emulated=True)
    v, f, t = host_wired_loop(b, hs, K, interval)
    what = (n, L, full)
    assert_all_equal(plant_state(b) + (b.solver_stats(),), plant_state(a) + (a.solver_stats(),), what)
    assert not a.status().any()
    assert np.array_equal(a.control_state().block(), ctl.st), what
    assert np.array_equal(a.wire_state().block(), ref.state()), what
    img, ok = a.input_image()
    want_img, want_ok = _image_of(v, f, t)
    assert np.array_equal(ok, want_ok) and np.array_equal(img, want_img), what
    # the case is one: wires delivered at every scan, the wired slots differ from the own instruments, the loops ran
    own = a.sensor_readings()[0]
    wired = blk[CL_OUT, 0] >= 0
    assert np.all(ref.n_routed[CL_OUT][wired] == 5) and not ref.n_lost.any() and (v[CL_OUT][wired] != own[CL_OUT][wired]).any()
    assert np.array_equal(v[CL_OUT][~wired], own[CL_OUT][~wired]) and (ctl.st[0, 5] > 0).mean() > 0.8   # n_exec
    # the holding image: with the loops off, one more scan decodes the words the loops last wrote
    a.disable_control()
    b.write_holding(ctl.holding)
    a.step(DT, n_steps=1, download=False)
    b.step(DT, n_steps=1, download=False)
    assert_all_equal(plant_state(b), plant_state(a), what + ("holding",))
    a.close(); b.close()


# ---- 2. the schedule and the placement change no bit
def test_schedule_and_placement_change_no_bit(gpu, wt, monkeypatch, full_waves):
    n, L, N, K = 8, 4, 100, 40                     # two trains per wavefront, the last group holds one
    cols, bc = wt.make_ensemble(N, seed=77)
    chlorine, acid = pi_loops(wt, cols)
    wires = _wires(wt, N, L)

    def run(chunk, streams=0, fused=True, calls=(K,), tickets=False, adaptive=False):
        if tickets:
            monkeypatch.setenv("WT_Q_TICKETS", "1")
        ens = _start(wt, cols, bc, n, L, chunk, np.arange(N) % 3, adaptive, streams)
        ens.enable_control(chlorine, acid)
        ens.set_wires(*wires)
        for c in calls:
            ens.step(DT, n_steps=c, fused=fused, download=False)
        out = _seen(ens) + (ens.control_state().block(), ens.wire_state().block())
        info = (ens.schedule(), ens.placement()[1])
        ens.close()
        monkeypatch.delenv("WT_Q_TICKETS", raising=False)
        return out, info

    every, seven, once = run(1)[0], run(7)[0], run(50)[0]
    wired = wt.wire_block(N, L, *wires)[CL_OUT, 0] >= 0
    for ref, scans in ((every, K), (seven, 6), (once, 1)):       # chunk 7: scans at 7 .. 35 and at the call's end
        assert not ref[5].any() and np.all(ref[-1][CL_OUT, 0][wired] == scans)
    # a scan after every outer step, however the steps are launched
    for v in (dict(chunk=1, streams=3), dict(chunk=7, fused=False), dict(chunk=50, calls=(1,) * K), dict(chunk=1, tickets=True)):
        assert_all_equal(every, run(**v)[0], v)
    for v in (dict(chunk=7, streams=3), dict(chunk=7, tickets=True)):
        assert_all_equal(seven, run(**v)[0], v)
    assert_all_equal(once, run(chunk=50, streams=3)[0], "streams, one scan")
    # adaptive placement: the second call re-deals (35 >= 33 steps of history) -- whole trains, in stage order
    got, (sched, perm) = run(chunk=7, adaptive=True, calls=(35, K - 35))
    assert_all_equal(seven, got, "adaptive")
    assert sched["redeals"] >= 1 and sorted(perm.tolist()) == list(range(N))
    assert not np.array_equal(perm, np.arange(N)), "the re-deal moved no train: the placement went untested"


# ---- 3. a program without a wire, and a cleared one, are invisible
def test_identity_cases(gpu, wt, full_waves):
    n, L, N, K = 8, 4, 36, 20
    cols, bc = wt.make_ensemble(N, seed=12)
    chlorine, acid = pi_loops(wt, cols)
    got = []
    for v in ("none", "own", "cleared"):
        ens = _start(wt, cols, bc, n, L, 3)
        ens.enable_control(chlorine, acid)
        if v == "own":
            ens.set_wires()
            assert ens.info(gpu.WT_INFO_WIRE) == 1
        if v == "cleared":
            ens.set_wires(*_wires(wt, N, L))
            ens.clear_wires()
            assert _refused(ens.wire_state) == E_NO_WIRE and ens.info(gpu.WT_INFO_WIRE) == 0
        ens.step(DT, n_steps=K, download=False)
        got.append(_seen(ens) + (ens.control_state().block(),))
        if v == "own":
            assert not ens.wire_state().block().any() and np.all(ens.wire_params()[:, 0] == -1)
        ens.close()
    assert_all_equal(got[0], got[1], "every slot -1")
    assert_all_equal(got[0], got[2], "set, then cleared")


# ---- 4. with every scan program on
def test_all_scan_programs_on(gpu, wt, full_waves):
    n, L, K, interval, cap = 8, 4, 36, 3, 16
    N = 2 * 8 + L                                   # two full wavefront-groups and one train in the last
    cols, bc = wt.make_ensemble(N, seed=91)
    r, stage = np.arange(N), np.arange(N) % L
    horizon = K * DT
    chlorine, acid = pi_loops(wt, cols)
    wires = [wt.Wire("chlorine_outlet", 0, L - 1), wt.Wire("temp_outlet", 1, 2, source="temp_inlet", trains=[0, 2, 4])]
    injections = [wt.Injection("chlorine_outlet", np.where(stage == 0, "bias", "off"), start=0.3 * horizon, end=0.7 * horizon, a=0.8),
                  wt.Injection("flow_main", np.where(r % 2 == 0, "fault", "off"), start=0.2 * horizon, a=3.0),
                  wt.Injection("chlorine_flow_rate", "gain", start=0.5 * horizon, end=0.8 * horizon, a=0.5)]
    cl0 = np.asarray(cols["initial_chlorine"])
    alarm_list = [wt.Alarm("chlorine_outlet", "low", cl0 + 0.05, deadband=0.01, source="image", action="trip_chlorine", trip_value=0.6),
                  wt.Alarm("chlorine_outlet", "low", cl0 + 0.05, deadband=0.01, source="field"),
                  wt.Alarm("flow_main", "high", 50.0, on_bad="alarm")]
    actuators = [wt.Actuator("chlorine", tau=40.0, rate=0.05), wt.Actuator("acid", delay=2)]
    detectors = [wt.Detector("chlorine_outlet", "cusum", 1.0, sigma=0.05, ref="track", tau=100.0),
                 wt.Detector("chlorine_outlet", "cusum", 1.0, sigma=0.05, ref="chlorine_outlet", ref_source="field"),
                 wt.Detector("temp_outlet", "ewma", 2.0, sigma=0.1, slack=0.3, ref="temp_outlet", ref_source="field", source="image"),
                 wt.Detector("chlorine_outlet", "cusum", 1.0, sigma=0.05, ref_value=cl0, source="field")]
    trends = [wt.Trend("image_value", "chlorine_outlet"), wt.Trend("field_value", "chlorine_outlet"),
              wt.Trend("image_fault", "flow_main"), wt.Trend("image_value", "temp_outlet", every=2),
              wt.Trend("control", ("chlorine", "output")), wt.Trend("command", r % 3, deadband=0.0),
              wt.Trend("alarm_word", deadband=0.0), wt.Trend("detect", (1, "stat"))]
    labels = np.array([[0.3 * horizon], [0.7 * horizon]]) * np.ones(N)
    ens = _start(wt, cols, bc, n, L, interval, np.arange(N) % 2)
    bc0 = ens.boundary()
    ens.enable_control(chlorine, acid)
    ens.set_injections(*injections)
    ens.set_alarms(*alarm_list)
    ens.set_actuators(*actuators)
    ens.set_detectors(*detectors, attack=(0.3 * horizon, 0.7 * horizon))
    ens.set_trends(*trends, capacity=cap)
    ens.set_wires(*wires)
    zero = np.zeros(N)
    master = words(np.array(MASTER)[:, None].repeat(N, axis=1))
    ctl = ControlRef(wt.control_block(N, chlorine, acid), zero, holding=master)
    ref = WireRef(wt.wire_block(N, L, *wires), L)
    hs = WireScan(N, ref, ctl=ctl, inj=InjectRef(wt.injection_block(N, *injections)), alm=LR.AlarmRef(wt.alarm_block(N, *alarm_list), zero),
                  act=AR.ActuatorRef(wt.actuator_block(N, *actuators), bc0, zero), det=KR.DetectRef(wt.detector_block(N, *detectors), labels, zero),
                  trd=TR.TrendRef(wt.trend_block(N, *trends), cap))
    for k, c in enumerate(hs.calls(K, interval)):
        cmd = commands(ctl.holding)                 # what this scan decodes: the loops' words of the scan before
        ens.step(DT, n_steps=c, download=False)
        v, _, f = ens.sensor_readings()
        vt, ft = hs.scan(v, f, cmd, took_the_step(ens.status()), tags={TR.COMMAND: ens.boundary()[[4, 6, 0]]})
        what = ("scan", k)
        assert np.array_equal(ens.control_state().block(), ctl.st), what
        assert np.array_equal(ens.injection_state().block(), hs.inj.st, equal_nan=True), what
        assert_all_equal(ref_alarms(hs.alm), alarms(ens), what + ("alarm",))
        assert_all_equal(ref_acts(hs.act), acts(ens), what + ("actuator",))
        assert_all_equal((hs.det.st, hs.det.t_prev), ens.detector_state().block(), what + ("detector",))
        assert np.array_equal(ens.trend_state().block(), hs.trd.st, equal_nan=True), what
        assert np.array_equal(ens.wire_state().block(), ref.state()), what
    assert not ens.status().any()
    d = ens.trend_data()
    assert_all_equal(hs.trd.data(), (d.time, d.value, d.count), "trend data")
    img, ok = ens.input_image()
    want_img, want_ok = _image_of(vt, ft, hs.lt - DT)
    assert np.array_equal(ok, want_ok) and np.array_equal(img, want_img)
    # a FIELD slot on a wired index still reads the reactor's own instrument, the IMAGE slot the remote one
    first = stage == 0
    scans = K // interval
    assert np.all(d.count[:2] == scans)
    own = ens.sensor_readings()[0][CL_OUT].astype(np.float64)
    assert np.array_equal(d.value[1, scans - 1], own, equal_nan=True)
    assert np.array_equal(d.value[0, scans - 1], vt[CL_OUT].astype(np.float64), equal_nan=True)
    assert np.array_equal(d.value[0, scans - 1][first], own[np.nonzero(first)[0] + L - 1], equal_nan=True)   # (the bias window is over)
    assert (d.value[0, :scans][:, first] != d.value[1, :scans][:, first]).all()
    assert np.array_equal(d.value[0, :scans][:, stage == 2], d.value[1, :scans][:, stage == 2], equal_nan=True)
    assert hs.inj.st[0, 0][first].min() > 0 and not hs.inj.st[0, 0][~first].any() and np.all(ref.n_routed[CL_OUT][first] == scans)
    ens.close()


# ---- 5. where a spoof lands
def test_a_spoof_lands_at_the_receivers_slot(gpu, wt):
    n, L, N, K = 8, 4, 8, 24
    cols, bc = wt.make_ensemble(N, seed=33)
    stage = np.arange(N) % L
    # only stage 0 doses, on the analyser of stage 3: nothing the source stage's controller does can reach stage 0
    # (setpoint: where the source's analyser starts, so that the output stays inside its limits with and without the bias)
    loop = wt.PILoop("chlorine_outlet", setpoint=np.roll(np.asarray(cols["initial_chlorine"]), -(L - 1)), kp=0.2, ki=1e-4, bias=0.5,
                     enable=stage == 0)

    def run(spoofed):
        ens = _start(wt, cols, bc, n, L, 2)
        ens.enable_control(chlorine=loop)
        ens.set_wires(wt.Wire("chlorine_outlet", 0, L - 1))
        if spoofed is not None:
            ens.set_injections(wt.Injection("chlorine_outlet", np.where(stage == spoofed, "bias", "off"), start=45.0, a=0.7))
        ens.step(DT, n_steps=K, download=False)
        out = (ens.control_state().block()[:, :, stage == 0], ens.boundary()[:, stage == 0], ens.state.chlorine[stage == 0])
        applied = ens.injection_state().n_applied[0] if spoofed is not None else None
        ens.close()
        return out, applied

    quiet, _ = run(None)
    at_receiver, n0 = run(0)
    at_source, n3 = run(L - 1)
    assert np.all(n0[stage == 0] == 10) and np.all(n3[stage == L - 1] == 10)       # scans at 50 .. 240 s
    print("stage 0's chlorine command, quiet / spoofed at the receiver:", quiet[0][0, 1], at_receiver[0][0, 1])
    assert (quiet[0][0, 1] > 0).all() and (quiet[0][0, 1] < 1).all()
    assert (at_receiver[0][0, 1] < quiet[0][0, 1]).all() and (at_receiver[1][6] != quiet[1][6]).all()   # the loop believes the bias
    assert_all_equal(quiet, at_source, "a spoof in the source stage's own image does not travel down the wire")


# ---- 6. a stopped source is a dead current loop
def test_a_stopped_source(gpu, wt):
    from conftest import golden_json
    g = golden_json("g4_faults.json")["cold_run"]
    cold = wt.ReactorConfiguration(**g["config"])
    cb = wt.BoundaryConditions(**dict(zip(wt.params.BOUNDARY_FIELDS, g["bc"])))
    warm, wb = wt.ReactorConfiguration(n_zones=cold.n_zones), wt.BoundaryConditions()
    cfgs, bcs, L, K, N = [warm, cold, warm, warm], [wb, cb, wb, wb], 2, 60, 4
    loop = wt.PILoop("chlorine_outlet", setpoint=1.5, kp=0.4, ki=1e-3, bias=0.2)
    wires = (wt.Wire("chlorine_outlet", 0, 1), wt.Wire("temp_inlet", 0, 1, source="temp_outlet", trains=0))

    def start():
        ens = wt.ReactorEnsemble(cfgs)
        ens.set_boundary(bcs)
        ens.enable_sensors(seed=7)
        ens.enable_plant_io()
        ens.set_schedule(0, 1)
        ens.set_trains(L, linked=False)             # (the cold tank's water stays where it is)
        return ens

    a = start()
    a.enable_control(chlorine=loop)
    a.set_wires(*wires)
    es = a.step(1.0, n_steps=K)
    assert es.status[1] & 1 and es.time[1] < K and not es.status[[0, 2, 3]].any() and np.all(es.time[[0, 2, 3]] == K)
    took = int(es.time[1])                          # (dt = 1: the scans the cold tank took part in)
    ws, cs = a.wire_state(), a.control_state().chlorine
    assert ws.n_routed[CL_OUT].tolist() == [took, 0, K, 0] and ws.n_lost[CL_OUT].tolist() == [K - took, 0, 0, 0]
    assert ws.n_lost[5].tolist() == [K - took, 0, 0, 0] and 0 < took < K - 5
    assert cs.n_held[0] >= K - took and cs.n_exec[0] + cs.n_held[0] == K and cs.n_held[2] < cs.n_held[0]
    img, ok = a.input_image()
    assert ok.all() and wt.ReactorEnsemble.decode_float32(img[:1, 8:10])[0] == 0.0 and img[0, 18] == 1 and img[2, 18] == 0
    b = start()
    ctl, ref = ControlRef(wt.control_block(N, loop, None), np.zeros(N)), WireRef(wt.wire_block(N, L, *wires), L)
    hs = WireScan(N, ref, ctl=ctl, emulated=True, dt=1.0)
    v, f, t = host_wired_loop(b, hs, K, 1)
    assert np.isnan(v[CL_OUT, 0]) and f[CL_OUT, 0] == 1 and np.isnan(v[5, 0]) and f[5, 0] == 1
    assert_all_equal(plant_state(b), plant_state(a), "stopped source")
    assert np.array_equal(a.control_state().block(), ctl.st) and np.array_equal(ws.block(), ref.state())
    live = took_the_step(a.status())
    want_img, want_ok = _image_of(v[:, live], f[:, live], t[live])
    assert np.array_equal(img[live], want_img) and np.array_equal(ok[live], want_ok)
    a.close(); b.close()


# ---- 7. errors and lifetime
def test_refusals_and_lifetime(gpu, wt, full_waves):
    L_ = gpu.lib()
    n, L, N, K = 8, 4, 24, 6
    cols, bc = wt.make_ensemble(N, seed=3)
    ens = wt.ReactorEnsemble(cols, n_zones=n)
    ens.set_boundary(bc)
    attrs = set(vars(ens))
    own = wt.wire_block(N, L)
    call = lambda blk: (L_.wt_ensemble_wire_set(ens._h, gpu.dptr(blk)), L_.wt_last_error().decode())
    assert _refused(ens.set_wires) == E_NO_TRAIN and _refused(ens.wire_state) == E_NO_WIRE and _refused(ens.wire_params) == E_NO_WIRE
    assert call(own) == (gpu.WT_E_STATE, E_NO_TRAIN)
    ens.clear_wires()                               # no effect while none is set
    ens.set_trains(L)
    assert _refused(ens.set_wires) == E_NO_IO and call(own) == (gpu.WT_E_STATE, E_NO_IO) and ens.info(gpu.WT_INFO_WIRE) == 0
    ens.enable_sensors(seed=5)
    ens.enable_plant_io()
    ens.set_schedule(0, 2)
    # the handle's own checks (the builder would stop these before the call), in the order of wt_wire_check
    def bad(*at):
        blk = own.copy()
        for slot, field, r, v in at:
            blk[slot, field, r] = v
        return call(blk)
    assert bad((3, 0, 1, np.nan)) == (gpu.WT_E_ARG, E_FINITE) and bad((3, 0, 1, 4.0)) == (gpu.WT_E_ARG, E_STAGE)
    assert bad((3, 0, 1, -2.0)) == (gpu.WT_E_ARG, E_STAGE) and bad((3, 1, 1, 7.0)) == (gpu.WT_E_ARG, E_SENSOR)
    assert bad((0, 1, 2, 9.0), (6, 0, 2, 7.0), (3, 0, 5, np.inf)) == (gpu.WT_E_ARG, E_STAGE)
    assert bad((0, 1, 2, 9.0), (6, 0, 2, np.inf), (3, 0, 5, 9.0)) == (gpu.WT_E_ARG, E_FINITE)
    assert L_.wt_ensemble_wire_set(ens._h, None) == gpu.WT_E_ARG
    assert _refused(ens.set_wires, wt.Wire(3, 0, L)) == E_STAGE and _refused(ens.wire_state) == E_NO_WIRE   # a refused set sets nothing
    ens.set_wires(wt.Wire("chlorine_outlet", 0, 3))
    assert ens.info(gpu.WT_INFO_WIRE) == 1 and not ens.wire_state().block().any()
    assert _refused(ens.set_wires, wt.Wire(3, 0, 1, source=9)) == E_SENSOR and ens.wire_params()[3, 0, 0] == 3   # ... and leaves the program
    ens.step(DT, n_steps=K, download=False)
    first = np.arange(N) % L == 0
    assert np.array_equal(ens.wire_state().n_routed[CL_OUT], np.where(first, K // 2, 0))
    # set twice replaces the program and restarts the counters
    ens.set_wires(wt.Wire("pH_outlet", 1, 0, source="pH_inlet", trains=[0, 2]))
    want = wt.wire_block(N, L, wt.Wire("pH_outlet", 1, 0, source="pH_inlet", trains=[0, 2]))
    assert np.array_equal(ens.wire_params(), want) and not ens.wire_state().block().any()
    ens.step(DT, n_steps=K, download=False)
    assert ens.wire_state().n_routed[1].tolist() == [0, 3, 0, 0, 0, 0, 0, 0, 0, 3] + [0] * 14 and not ens.wire_state().n_routed[CL_OUT].any()
    # set_state: a new state is a new plant -- the counters from the start, the program stays
    s = ens.state
    ens.set_state(s.pH, s.chlorine, s.temperature, s.time)
    assert not ens.wire_state().block().any() and np.array_equal(ens.wire_params(), want)
    # train_set over a program clears the wires, and so does train_clear
    ens.set_trains(2)
    assert _refused(ens.wire_state) == E_NO_WIRE and ens.info(gpu.WT_INFO_WIRE) == 0
    assert _refused(ens.set_wires, wt.Wire(3, 0, 2)) == E_STAGE                      # the length is the handle's
    ens.set_wires(wt.Wire(3, 0, 1))
    ens.clear_trains()
    assert _refused(ens.wire_state) == E_NO_WIRE and _refused(ens.set_wires) == E_NO_TRAIN and ens.info(gpu.WT_INFO_WIRE) == 0
    assert set(vars(ens)) == attrs                  # the object keeps no new attribute
    ens.step(DT, n_steps=2, download=False)
    ens.close()
    # destroying the handle with a program set
    ens = plant(wt, cols, bc, n)
    ens.set_trains(L)
    ens.set_wires(*_wires(wt, N, L))
    ens.step(DT, n_steps=2, download=False)
    ens.close()
