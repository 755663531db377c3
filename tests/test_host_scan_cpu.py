"""``program_helpers.HostScan`` without a device: with a detector and a trend recorder it leaves the bits the call sites'
hand-written sequences left, and the order of its scan, stated as facts about what a later link sees of an earlier one.
Six reactors, seven synthetic readings, ten scans; reactor 5 skips scan 4 and reactor 0 scan 6, pH_outlet reads NaN in
reactor 2 at scans 2 to 4 and flow_main carries a fault code in reactor 4 at scan 5."""
import numpy as np
import pytest

import detect_ref as KR
import trend_ref as TR
import tune_ref as UR
from actuator_ref import ActuatorRef
from alarm_ref import AlarmRef
from control_ref import ControlRef
from detect_ref import DetectRef
from inject_ref import InjectRef
from program_helpers import HostScan, assert_all_equal
from trend_ref import TrendRef

N, SCANS, INTERVAL = 6, 10, 3
CL, PH, FLOW = 3, 1, 4             # chlorine_outlet, pH_outlet, flow_main
SPOOF = 0.25
CS_OUTPUT = 1                      # control.STATE_ROWS


@pytest.fixture(scope="module")
def case(wt):
    rng = np.random.default_rng(17)
    v = rng.uniform([[6.5], [6.5], [0.5], [0.5], [4.0], [10.0], [10.0]], [[8.0], [8.0], [3.0], [3.0], [8.0], [25.0], [25.0]],
                    (SCANS, 7, N)).astype(np.float32)
    f = np.zeros((SCANS, 7, N), dtype=np.int64)
    v[2:5, PH, 2] = np.nan
    f[5, FLOW, 4] = 2
    stepped = np.ones((SCANS, N), dtype=bool)
    stepped[4, 5] = stepped[6, 0] = False
    cmd = np.stack([rng.uniform(-0.2, 2.2, (SCANS, N)), rng.uniform(-0.2, 1.2, (SCANS, N)), rng.uniform(0.0, 22.0, (SCANS, N))],
                   axis=1).astype(np.float32)
    cols, bc = wt.make_ensemble(N, seed=3)
    horizon = SCANS * INTERVAL * 10.0
    blocks = dict(
        ctl=wt.control_block(N, wt.PILoop("chlorine_inlet", setpoint=1.0 + rng.random(N), kp=0.2, ki=1e-3, bias=0.4),
                             wt.PILoop("pH_outlet", setpoint=7.0, kp=0.3, ki=1e-3, direction=-1, bias=0.1)),
        inj=wt.injection_block(N, wt.Injection("chlorine_outlet", "constant", a=SPOOF),
                               wt.Injection("chlorine_flow_rate", "gain", start=0.3 * horizon, end=0.7 * horizon, a=0.5)),
        alm=wt.alarm_block(N, wt.Alarm("chlorine_outlet", "high", 1.5 + rng.random(N), source="field", action="trip_chlorine",
                                       trip_value=0.1),
                           wt.Alarm("pH_outlet", "low", 7.2, on_bad="alarm")),
        act=wt.actuator_block(N, wt.Actuator("chlorine", tau=40.0, rate=0.05), wt.Actuator("acid", delay=2)),
        det=wt.detector_block(N, wt.Detector("chlorine_outlet", "cusum", 4.0, sigma=0.5, ref_value=1.5),
                              wt.Detector("chlorine_outlet", "cusum", 4.0, sigma=0.5, ref_value=1.5, source="field"),
                              wt.Detector("pH_outlet", "ewma", 1.0, sigma=0.3, ref_value=7.2, source="field", on_bad="alarm")),
        trd=wt.trend_block(N, wt.Trend("detect", (1, "stat")), wt.Trend("control", ("chlorine", "output")),
                           wt.Trend("alarm_word"), wt.Trend("image_value", "chlorine_outlet"),
                           wt.Trend("field_value", "chlorine_outlet", every=2), wt.Trend("command", "chlorine"),
                           wt.Trend("actuator", ("chlorine", "position"), deadband=0.0), wt.Trend("inject", (1, "n_applied"))))
    return dict(v=v, f=f, stepped=stepped, cmd=cmd, bc=bc, blocks=blocks, labels=np.array([[0.3 * horizon], [0.7 * horizon]]) * np.ones(N))


def _refs(case, *names):
    zero, b = np.zeros(N), case["blocks"]
    make = dict(ctl=lambda: ControlRef(b["ctl"], zero), inj=lambda: InjectRef(b["inj"]), alm=lambda: AlarmRef(b["alm"], zero),
                act=lambda: ActuatorRef(b["act"], case["bc"], zero), det=lambda: DetectRef(b["det"], case["labels"], zero),
                trd=lambda: TrendRef(b["trd"], SCANS))
    return {k: make[k]() for k in names}


def _state(refs):
    """Everything the refs hold, in a fixed order."""
    out = ()
    for k, attrs in (("ctl", ("st", "t_prev", "holding")), ("inj", ("st",)), ("alm", ("st", "rst", "words")),
                     ("act", ("st", "q", "t_prev")), ("det", ("st", "t_prev")), ("trd", ("st", "ring_t", "ring_x"))):
        if k in refs:
            out += tuple(getattr(refs[k], a) for a in attrs)
    return out


def _scans(*scanners):
    """The scan number, with every scanner's loop time advanced to it."""
    return (k for k, *_ in zip(range(SCANS), *(hs.calls(SCANS * INTERVAL, INTERVAL) for hs in scanners)))


def test_detector_after_injection_as_the_call_sites_wired_it(case):
    v, f = case["v"], case["f"]
    old, new = _refs(case, "inj", "det"), _refs(case, "inj", "det")
    hand, hs = HostScan(N, inj=old["inj"]), HostScan(N, **new)
    for k in _scans(hand, hs):
        # test_gpu_detect.py::_restate and tools/detect_probe.py, before HostScan took ``det``
        vt, ft = hand.scan(v[k], f[k])
        old["det"].scan(v[k], f[k], hand.lt, image=(vt, ft))
        hs.scan(v[k], f[k])
    assert_all_equal(_state(old), _state(new), "inj + det")
    assert old["det"].st[:3, KR.KS_N_EVAL].all() and (old["det"].st[0] != old["det"].st[1]).any()


def test_trend_with_supplied_values_as_the_call_sites_wired_it(case):
    v, f = case["v"], case["f"]
    rng = np.random.default_rng(5)
    old, new = _refs(case, "inj", "trd"), _refs(case, "inj", "trd")
    hand, hs = HostScan(N, inj=old["inj"]), HostScan(N, **new)
    for k in _scans(hand, hs):
        supplied = {TR.COMMAND: rng.random((3, N)), TR.CONTROL: rng.random((16, N)), TR.INJECT: rng.random((16, N)),
                    TR.ALARM: rng.random((32, N)), TR.ALARM_WORD: rng.integers(0, 9, N).astype(np.float64),
                    TR.ACTUATOR: rng.random((27, N)), TR.DETECT: rng.random((64, N))}
        # test_gpu_trend.py::_values and its loop, before HostScan took ``trd``
        vt, ft = hand.scan(v[k], f[k])
        vals = {TR.IMAGE_VALUE: vt.astype(np.float64), TR.IMAGE_FAULT: ft.astype(np.float64), TR.FIELD_VALUE: v[k].astype(np.float64),
                TR.FIELD_FAULT: f[k].astype(np.float64), **supplied}
        old["trd"].scan(vals, hand.lt)
        hs.scan(v[k], f[k], tags=supplied)
        assert hs.values.keys() == vals.keys()
        assert_all_equal(list(vals.values()), [hs.values[t] for t in vals], ("values", k))
    assert_all_equal(_state(old), _state(new), "inj + trd")
    assert np.all(old["trd"].st[[0, 1, 2, 3, 5, 7], TR.TS_N_RECORDED] == SCANS) and not np.isnan(old["trd"].ring_x[:, 0]).any()


@pytest.fixture(scope="module")
def all_six(case):
    """All six programs with commands and a stepped mask, hand-wired and through HostScan; per scan, what the hand-wired
    refs held when the scan was over, and the last values HostScan's detector slots 0 (IMAGE) and 1 (FIELD) saw."""
    v, f, cmd, stepped = case["v"], case["f"], case["cmd"], case["stepped"]
    names = ("ctl", "inj", "alm", "act", "det", "trd")
    old, new = _refs(case, *names), _refs(case, *names)
    hand, hs = HostScan(N, **{k: old[k] for k in names[:4]}), HostScan(N, **new)
    after = dict(stat=[], output=[], word=[], x_image=[], x_field=[])
    for k in _scans(hand, hs):
        command = {TR.COMMAND: cmd[k].astype(np.float64)}
        # test_gpu_program_shapes.py::test_everything_on_equals_the_restatements, before HostScan took ``det``, with
        # the recorder fed as test_gpu_trend.py fed it: the get blocks' layout, taken when the scan is over
        image = hand.scan(v[k], f[k], cmd[k], stepped[k])
        old["det"].scan(v[k], f[k], hand.lt, stepped[k], image=image)
        vals = {TR.IMAGE_VALUE: image[0].astype(np.float64), TR.IMAGE_FAULT: image[1].astype(np.float64),
                TR.FIELD_VALUE: v[k].astype(np.float64), TR.FIELD_FAULT: f[k].astype(np.float64),
                TR.CONTROL: old["ctl"].st.reshape(-1, N), TR.INJECT: old["inj"].st.reshape(-1, N),
                TR.ALARM: old["alm"].st.reshape(-1, N), TR.ALARM_WORD: old["alm"].words.astype(np.float64),
                TR.ACTUATOR: old["act"].st.reshape(-1, N), TR.DETECT: old["det"].st.reshape(-1, N), **command}
        old["trd"].scan(vals, hand.lt, stepped[k])
        hs.scan(v[k], f[k], cmd[k], stepped[k], tags=command)
        assert hs.values.keys() == vals.keys() and all(np.shape(x)[-1] == N for x in hs.values.values())
        after["stat"].append(old["det"].st[1, KR.KS_STAT].copy())
        after["output"].append(old["ctl"].st[0, CS_OUTPUT].copy())
        after["word"].append(old["alm"].words.astype(np.float64))
        after["x_image"].append(new["det"].st[0, KR.KS_X_PREV].copy())         # (HostScan's own detector)
        after["x_field"].append(new["det"].st[1, KR.KS_X_PREV].copy())
    return old, new, {k: np.array(x) for k, x in after.items()}


def test_all_six_programs_as_the_call_sites_wired_them(all_six):
    old, new, _ = all_six
    assert_all_equal(_state(old), _state(new), "all six")
    # the run was worth comparing: the command tamper and the trip acted, the acid loop held on the NaN reading
    assert old["inj"].st[1, 0].any() and old["alm"].rst[5].any() and old["ctl"].st[1, 6, 2] == 3
    assert old["trd"].st[0, TR.TS_N_SEEN].tolist() == [9, 10, 10, 10, 10, 9]


def _series(trd, slot, r):
    return trd.ring_x[slot, :int(trd.st[slot, TR.TS_N_RECORDED, r]), r]


@pytest.mark.parametrize("slot, what", [(0, "stat"), (1, "output"), (2, "word")])
def test_a_trend_slot_holds_this_scans_value(case, all_six, slot, what):
    """The recorder runs after the detector, the PI loops and the alarms: a sample is the value that program left at
    this scan, not the one it held when the scan began."""
    _, new, after = all_six
    for r in range(N):
        this = after[what][case["stepped"][:, r], r]
        assert np.array_equal(_series(new["trd"], slot, r), this, equal_nan=True), (what, r)
        assert (this[1:] != this[:-1]).any(), (what, r)          # the value moves from scan to scan: the scan before fails


def test_image_slots_see_the_spoof_and_field_slots_the_instrument(case, all_six):
    """The detector runs after the injection: its IMAGE slot on the spoofed chlorine_outlet holds the spoofed value as
    the last one it saw, the FIELD slot on the same sensor the instrument's own."""
    _, new, after = all_six
    v, stepped = case["v"], case["stepped"]
    for k in range(SCANS):
        took = stepped[k]
        assert took.sum() >= N - 1
        assert np.all(after["x_image"][k] == float(np.float32(SPOOF))), k              # (every reactor took scan 0)
        assert np.array_equal(after["x_field"][k][took], v[k, CL][took].astype(np.float64)), k
        assert np.array_equal(after["x_field"][k][~took], v[k - 1, CL][~took].astype(np.float64)), k
    assert np.all(v[:, CL] != np.float32(SPOOF))
    # and so does the recorder's reading tags: slot 3 the image, slot 4 the field value of every second scan seen
    for r in range(N):
        took = np.nonzero(stepped[:, r])[0]
        assert np.all(_series(new["trd"], 3, r) == float(np.float32(SPOOF))) and len(_series(new["trd"], 3, r)) == len(took)
        assert np.array_equal(_series(new["trd"], 4, r), v[took[::2], CL, r].astype(np.float64)), r


def test_tuner_before_the_pi_which_skips_the_loops_it_owns(wt):
    """``HostScan(N, ctl=, tun=)`` against the hand-written pair it stands for: ``TuneRef.scan``, then ``ControlRef.scan``
    with the loops the tuner owned as its skip mask.  Twelve reactors, forty scans; the chlorine_outlet reading is a square
    wave around the tuners' setpoint, so the relays cycle; reactor 3 reads a fault code and reactor 4 NaN for a few scans,
    reactors 5 and 0 each miss one; the experiments start at three different times, every second one commissions its PI
    loop, reactor 10 has no chlorine PI loop and reactor 11 no tuner."""
    n_r, scans = 12, 40
    rng = np.random.default_rng(23)
    r = np.arange(n_r)
    v = rng.uniform([[6.5], [6.5], [0.5], [0.5], [4.0], [10.0], [10.0]], [[8.0], [8.0], [3.0], [3.0], [8.0], [25.0], [25.0]],
                    (scans, 7, n_r)).astype(np.float32)
    v[:, CL] = (np.where((np.arange(scans) // 4) % 2 == 0, 1.25, 1.75)[:, None] + 0.05 * rng.random((scans, n_r))).astype(np.float32)
    f = np.zeros((scans, 7, n_r), dtype=np.int64)
    f[9:12, CL, 3] = 2
    v[14:17, CL, 4] = np.nan
    stepped = np.ones((scans, n_r), dtype=bool)
    stepped[13, 5] = stepped[21, 0] = False
    cblock = wt.control_block(n_r, wt.PILoop("chlorine_outlet", setpoint=1.5, kp=0.3, ki=1e-3, bias=0.2, enable=np.where(r == 10, 0, 1)),
                              wt.PILoop("pH_outlet", setpoint=7.0, kp=0.3, ki=1e-3, direction=-1, bias=0.1))
    tblock = wt.tune_block(n_r, wt.RelayTune("chlorine_outlet", 1.5, 0.25, 0.5, start=50.0 + 120.0 * (r % 3), settle=0, cycles=2,
                                             commission=r % 2, enable=np.where(r == 11, 0, 1)))
    pairs = []
    for _ in range(2):
        ctl = ControlRef(cblock, np.zeros(n_r))
        pairs.append((ctl, UR.TuneRef(tblock, ctl=ctl)))
    (ctl, tun), (hs_ctl, hs_tun) = pairs
    hs = HostScan(n_r, ctl=hs_ctl, tun=hs_tun)
    kept = np.zeros((2, n_r), dtype=bool)
    for k, _ in zip(range(scans), hs.calls(scans * INTERVAL, INTERVAL)):
        before = ctl.st.copy()
        tun.scan(v[k], f[k], hs.lt, stepped[k])
        ctl.scan(v[k], f[k], hs.lt, stepped[k], skip=tun.owned)
        hs.scan(v[k], f[k], stepped=stepped[k])
        # a loop whose experiment is still running after the scan was owned and not commissioned: its PI state stands
        running = tun.owned & (tun.st[:, UR.US_PHASE] == UR.RUNNING)
        for l in range(2):
            assert np.array_equal(ctl.st[l][:, running[l]], before[l][:, running[l]]), (k, l)
        kept |= running
        assert np.array_equal(ctl.t_prev[stepped[k]], hs.lt[stepped[k]])               # t_prev advances, owned or not
    state = lambda c, t: (c.st, c.t_prev, c.holding, c.p, t.st, t.owned, t.holding)
    assert_all_equal(state(ctl, tun), state(hs_ctl, hs_tun), "tuner + PI")
    assert hs.holding() is hs_ctl.holding and hs_tun.holding is hs_ctl.holding
    # the run was worth comparing
    phase, com = tun.st[0, UR.US_PHASE], tun.st[0, UR.US_COMMISSIONED] == 1
    assert kept[0, :10].all() and not kept[0, 11] and not kept[1].any()
    assert (phase[:11] == UR.DONE).all() and phase[11] == UR.WAITING and len(np.unique(tun.st[0, UR.US_T_BEGIN, :11])) == 3
    assert np.array_equal(com, (r % 2 == 1) & (r < 10)) and np.array_equal(ctl.p[0, 4, com], tun.st[0, UR.US_KP, com])
    assert tun.st[0, UR.US_N_HELD, 3] > 0 and tun.st[0, UR.US_N_HELD, 4] > 0
    scans_taken = stepped.sum(axis=0)
    assert np.array_equal(ctl.st[1, 5] + ctl.st[1, 6], scans_taken)                      # the acid PI ran at every scan taken
    assert np.all((ctl.st[0, 5] + ctl.st[0, 6])[:10] < scans_taken[:10]) and np.all((ctl.st[0, 5] + ctl.st[0, 6])[:10] > 0)
    assert ctl.st[0, 5, 11] + ctl.st[0, 6, 11] == scans_taken[11]                        # no tuner: the chlorine PI never skipped
    # a tuner without a PI: the words HostScan hands the master are the tuner's
    alone = UR.TuneRef(tblock)
    assert HostScan(n_r, tun=alone, emulated=True).holding() is alone.holding
