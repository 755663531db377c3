"""The per-reactor programs at the step-kernel instantiations the other program tests do not reach (csrc/wtphys.hip
``with_step_kernel``): wavefronts with idle lanes, an odd number of reactors per wavefront, a last wavefront-group that
holds one reactor, and reactors that do not step while their wavefront neighbours do.  With all eight programs on, the
device's program state is the restatements' bit for bit after every call; one fused call is the call-per-interval loop;
and programs that are off change nothing."""
import numpy as np
import pytest

import actuator_ref as AR
import alarm_ref as LR
import control_ref as CR
import detect_ref as KR
import disturb_ref as DR
import inject_ref as IR
import score_ref as SR
import trend_ref as TR
from program_helpers import (DT, MASTER, HostScan, acts, alarms, assert_all_equal, assert_equal_by_reactor, calls, everything,
                             full_waves, instantiation, plant, ragged_size, ref_acts, ref_alarms, wavefront_groups, words)
from test_gpu_actuator import _words
from test_gpu_detect import EVERYTHING, _closed, _four
from test_gpu_score import ROWS

ZONES = (2, 3, 5, 7, 12, 16, 17)           # one or two per instantiation without a program test, and the lower edge of <5,false>
OLD_ZONES = (4, 8, 20, 32)                 # the zone counts of the other bit-for-bit program tests
STEPS, STOP_AT = 120, 63                   # 1200 s; the mid-run stop falls between two calls of either scan interval
T_END = STEPS * DT
FROZEN = 1 | 32 | 64                       # WT_ST_T_RANGE, WT_ST_T_RANGE_POST, WT_ST_NONFINITE
LABEL = (300.0, 800.0)
SINE_AMPLITUDE, OU_SIGMA = 5.0, 0.3
BINS = 16
DT_PLACED = {16: 2.0, 17: 2.0}             # outer step of the adaptive-placement twins where 10 s gives the sort nothing to do


def test_zone_counts_reach_every_program_instantiation():
    carrying = {(1, True), (2, False), (2, True), (3, False), (3, True), (4, False), (4, True), (5, False)}
    new, old = {instantiation(n) for n in ZONES}, {instantiation(n) for n in OLD_ZONES}
    assert max(ZONES + OLD_ZONES) <= 32 and instantiation(33) == (6, False)      # the n > 32 kernel refuses programs
    assert new | old == carrying
    assert carrying - old <= new
    assert [instantiation(n) for n in (2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 32)] == [
        (1, True), (2, False), (2, True), (3, False), (3, False), (3, True), (4, False), (4, False), (4, True), (5, False),
        (5, False)]


def _roles(n):
    """Who does not step: three reactors with a non-finite pH from the start (first slot of group 0, a middle slot of
    group 1, last slot of group 2) and two stopped after STOP_AT steps (a middle slot of group 3, whose other reactors go
    on, and the lone reactor of the last group).  ``cls`` deals the reactors that step throughout into thirds: 0 gets
    parameters that make a realistic slot act, 1 parameters that keep it quiet, 2 anything in between."""
    R, N = ragged_size(n)
    never = np.array([0, R + R // 2, 2 * R + R - 1])
    stopped = np.array([3 * R + R // 2, N - 1])
    through = np.setdiff1d(np.arange(N), np.concatenate([never, stopped]))
    cls = np.arange(N) % 3
    cls[through] = np.arange(len(through)) % 3
    return R, N, never, stopped, through, cls


def _by_class(cls, rng, act, quiet, between):
    """Per-reactor values: uniform in the (lo, hi) pair of the reactor's class."""
    lo, hi = np.array([act, quiet, between]).T
    return rng.uniform(lo[cls], hi[cls])


def _window(cls, rng, shift=0):
    """Start and end of a per-reactor window: opens and closes inside the run (class 0), never opens (1), anywhere (2)."""
    c = (cls + shift) % 3
    start = _by_class(c, rng, (0.05 * T_END, 0.4 * T_END), (T_END + 100.0, 2 * T_END), (0.0, 2 * T_END))
    return start, start + rng.uniform(0.15, 0.4, len(cls)) * T_END


def _programs(wt, cols, bc, n, cls):
    """All eight programs.  Each scan program has one slot forced to act at every scan of every reactor that steps and
    realistic slots with per-reactor parameters around the reactor's own start."""
    N = len(cls)
    rng = np.random.default_rng(100 + n)
    r = np.arange(N)
    cl0, temp = np.asarray(cols["initial_chlorine"]), np.asarray(cols["temperature"])
    # PI: a chlorine loop whose setpoint is out of reach with a high gain (saturates), or close with a low one (does not)
    chlorine = wt.PILoop("chlorine_outlet", setpoint=cl0 + _by_class(cls, rng, (3.0, 4.0), (-0.2, 0.2), (-1.0, 1.0)),
                         kp=np.where(cls == 1, 0.02, 2.0), ki=np.where(cls == 1, 1e-6, 1e-4 + 2e-3 * rng.random(N)), bias=0.3)
    acid = wt.PILoop("pH_outlet", setpoint=6.8 + 0.6 * rng.random(N), kp=0.1 + 0.9 * rng.random(N), ki=1e-3, direction=-1, bias=0.1)
    # injections: the flow reading biased at every scan; a spoof of chlorine_outlet and two command tampers in windows
    s1, e1 = _window(cls, rng)
    s2, e2 = _window(cls, rng, 1)
    s3, e3 = _window(cls, rng, 2)
    injections = [wt.Injection("flow_main", "bias", a=0.5),
                  wt.Injection("chlorine_outlet", np.choose(r % 4, ["bias", "ramp", "freeze", "dropout"]), start=s1, end=e1,
                               a=rng.uniform(-0.5, 0.5, N), b=np.where(r % 4 == 1, rng.uniform(-1e-3, 1e-3, N), 0.0)),
                  wt.Injection("chlorine_flow_rate", "gain", start=s2, end=e2, a=rng.uniform(0.0, 2.0, N)),
                  wt.Injection(np.choose(r % 2, ["acid_flow_rate", "inlet_flow_rate"]), np.choose(r % 2, ["dropout", "bias"]),
                               start=s3, end=e3, a=rng.uniform(-1.0, 1.0, N))]
    # alarms: the flow trip that stands from the first scan; chlorine_outlet HIGH around the start; pH_outlet (warming
    # up: bad readings under both policies); a latched temperature limit
    alarms = [wt.Alarm("flow_main", "high", -1.0, source="field", on_bad="alarm", action="trip_chlorine",
                       trip_value=(bc[6] + 0.5) % 1.0),
              wt.Alarm("chlorine_outlet", "high", cl0 + _by_class(cls, rng, (-1.5, -1.0), (3.0, 4.0), (-0.3, 0.6)),
                       deadband=rng.uniform(0, 0.2, N), on_delay=rng.uniform(0, 100, N), latch=rng.random(N) < 0.5,
                       action="trip_acid", trip_value=rng.uniform(0, 2, N)),
              wt.Alarm("pH_outlet", "low", rng.uniform(6.8, 7.6, N), deadband=0.1, source="field",
                       on_bad=np.choose(r % 2, ["hold", "alarm"]), action="trip_acid", trip_value=rng.uniform(0, 2, N)),
              wt.Alarm("temp_outlet", "high", temp + rng.uniform(-0.5, 0.5, N), latch=True)]
    # actuators: a chlorine pump whose rate limit (1e-3 per 10 s) is far below the half unit between its start and the
    # trip value it is driven to; acid and inlet elements with lags, backlash, delays 0..8 and fault windows
    actuators = [wt.Actuator("chlorine", rate=1e-4)]
    for ch, lim, lo, shift in (("acid", 2.0, 0.0, 0), ("inlet", 20.0, 0.2, 1)):
        c = (cls + shift) % 3
        t_fault = _by_class(c, rng, (0.0, 0.5 * T_END), (0.0, 0.5 * T_END), (0.0, 1.5 * T_END))
        actuators.append(wt.Actuator(
            ch, tau=np.where(rng.random(N) < 0.2, 0.0, rng.uniform(1, 120, N)),
            rate=np.where(rng.random(N) < 0.3, np.inf, lim * 10.0 ** rng.uniform(-4.0, -1.7, N)),
            backlash=np.where(rng.random(N) < 0.5, 0.0, rng.uniform(0, 0.1 * lim, N)), delay=rng.integers(0, 9, N),
            fault=np.where(c == 1, 0, rng.integers(1, 3, N)), t_fault=t_fault,
            t_repair=t_fault + rng.uniform(0.1, 0.4, N) * T_END, fail_value=rng.uniform(lo, lim, N)))
    # detectors: the flow CUSUM that alarms at every scan; an EWMA of chlorine_outlet two units off its reference with
    # limits from far below to far above what the residual reaches; pH_outlet under both policies; the cross-check
    limit = 10.0 ** _by_class(cls, rng, (-2.0, -0.3), (2.3, 4.0), (-2.0, 4.0))
    detectors = [wt.Detector("flow_main", "cusum", 1.0, slack=0.0, ref_value=-1.0, source="field", on_bad="alarm"),
                 wt.Detector("chlorine_outlet", "ewma", limit, sigma=0.1, ref_value=cl0 + 2.0),
                 wt.Detector("pH_outlet", "cusum", 10.0 ** rng.uniform(0, 1, N), sigma=0.02, ref="track", tau=100.0, source="field",
                             on_bad=np.choose(r % 2, ["alarm", "hold"])),
                 wt.Detector("chlorine_outlet", "cusum", 10.0 ** rng.uniform(-0.3, 0.7, N), sigma=0.05, ref="chlorine_outlet",
                             ref_source="field")]
    # disturbances: the slots of test_gpu_disturb.py::test_matches_restatement (its tolerances hold for the SINE and
    # the OU slot), the STEP's window by class, the RAMP's offset in force from 30 s on in every reactor
    u = rng.random((3, N))
    s0, _ = _window(cls, rng)
    disturbances = [wt.Disturbance.step("inlet_temperature", 0.5 + 2.5 * u[0], s0, s0 + 300.0),
                    wt.Disturbance.ramp("chlorine_concentration", 1e-4, 30.0, 700.0, offset=0.02),
                    wt.Disturbance.sine("ambient_temperature", SINE_AMPLITUDE, 480.0 + 240.0 * u[1], phase=u[2]),
                    wt.Disturbance.ou("inlet_chlorine", OU_SIGMA, 90.0, 20.0, 900.0)]
    # scores: outlet chlorine against a band by class; pH of an interior zone; temperature MIN / MAX above 0 degC at every
    # step; mean chlorine in a window
    lo = cl0 + _by_class(cls, rng, (1.0, 2.0), (-6.0, -5.0), (-0.5, 0.5))
    scores = [wt.Score("chlorine", lo, lo + np.where(cls == 1, 12.0, 0.3)),
              wt.Score("pH", 6.8, 8.2, zone=r % (n - 1)),
              wt.Score("temperature", hi=0.0, reduce=np.choose(r % 2, ["min", "max"])),
              wt.Score("chlorine", lo=cl0 - 0.2, reduce="mean", t_start=100.0, t_end=1000.0)]
    fan = ([0.0, 6.0, 5.0, 0.0], [6.0, 9.0, 35.0, 5.0])
    # trends: a tag of every other scan program, an image value and a field fault code; slots 0, 1, 4, 5 and 7 record
    # every candidate (every 1, 2 or 3), slots 2, 3 and 6 changes only
    trends = [wt.Trend("control", ("chlorine", "output")), wt.Trend("inject", (0, "n_applied"), every=3),
              wt.Trend("alarm", (1, "time_active"), deadband=0.0), wt.Trend("alarm_word", deadband=0.0),
              wt.Trend("actuator", ("chlorine", "position")),
              wt.Trend("detect", r % 4 * 16 + KR.KS_STAT, every=np.choose(r % 2, [1, 2])),
              wt.Trend("image_value", "chlorine_outlet", deadband=0.0), wt.Trend("field_fault", "pH_outlet", every=3)]
    return dict(loops=(chlorine, acid), injections=injections, alarms=alarms, actuators=actuators, detectors=detectors,
                disturbances=disturbances, scores=scores, fan=fan, trends=trends)


def _set_all(wt, ens, p):
    ens.enable_control(*p["loops"])
    ens.set_injections(*p["injections"])
    ens.set_alarms(*p["alarms"])
    ens.set_actuators(*p["actuators"])
    ens.set_detectors(*p["detectors"], attack=LABEL)
    ens.set_disturbances(*p["disturbances"], seed=99, reactor_base=5, history=STEPS + 1)
    ens.set_scores(*p["scores"], curve=STEPS, bins=BINS, fan_range=p["fan"])
    ens.set_trends(*p["trends"], capacity=STEPS)           # a scan per step at the most: nothing is dropped


def _shares(flag, among):
    return float(np.mean(flag[among]))


@pytest.mark.gpu
@pytest.mark.parametrize("n", ZONES)
def test_everything_on_equals_the_restatements(gpu, wt, full_waves, n):
    """Shares and wall times observed on the MI355X are recorded in DESIGN.md section 7.12."""
    R, N, never, stopped, through, cls = _roles(n)
    cols, bc = wt.make_ensemble(N, seed=1200 + n)
    p = _programs(wt, cols, bc, n, cls)
    blocks = dict(ctl=wt.control_block(N, *p["loops"]), inj=wt.injection_block(N, *p["injections"]),
                  alm=wt.alarm_block(N, *p["alarms"]), act=wt.actuator_block(N, *p["actuators"]),
                  det=wt.detector_block(N, *p["detectors"]), dst=wt.disturbance_block(N, *p["disturbances"]),
                  scr=wt.score_block(N, *p["scores"]), trd=wt.trend_block(N, *p["trends"]))
    labels = np.array(LABEL)[:, None] * np.ones(N)
    dst_ref, times = None, None
    for interval in (1, 7):
        ens = plant(wt, cols, bc, n, history=STEPS)
        ens.set_placement(False)
        ens.set_schedule(0, interval)
        s = ens.state
        pH = s.pH.copy()
        pH[never, np.arange(3) % n] = [np.nan, np.inf, np.nan]
        ens.set_state(pH, s.chlorine, s.temperature)
        ens.record(every=1, capacity=STEPS)
        bc0 = ens.boundary()                     # the disturbances' base, the final elements' start
        _set_all(wt, ens, p)
        zero = np.zeros(N)
        ctl, inj, alm = CR.ControlRef(blocks["ctl"], zero), IR.InjectRef(blocks["inj"]), LR.AlarmRef(blocks["alm"], zero)
        act, det = AR.ActuatorRef(blocks["act"], bc0, zero), KR.DetectRef(blocks["det"], labels, zero)
        trd = TR.TrendRef(blocks["trd"], STEPS)
        hs = HostScan(N, ctl=ctl, inj=inj, alm=alm, act=act, det=det, trd=trd)          # no COMMAND slot: every tag is held
        rng = np.random.default_rng(10 * n + interval)
        t_before, done, scans = np.zeros(N), 0, np.zeros(N)
        for k, c in enumerate(hs.calls(STEPS, interval)):
            if done == STOP_AT:            # between two calls: one zone above 100 degC, the reactor raises and stops
                s = ens.state
                T = s.temperature.copy()
                T[stopped, [0, n - 1]] = [150.0, 101.0]
                ens.set_state(s.pH, s.chlorine, T)
            cmd = _words(rng, N)
            ens.write_holding(words(cmd))
            ens.step(DT, n_steps=c, download=False)
            done += c
            t_now = ens.state.time
            stepped = t_now != t_before           # the reactor's time advanced in this call
            t_before = t_now
            scans += stepped
            v, _, f = ens.sensor_readings()
            hs.scan(v, f, cmd, stepped)
            what = (n, interval, k)
            assert_equal_by_reactor((ctl.st,), (ens.control_state().block(),), what + ("control",), R)
            assert_equal_by_reactor((inj.st,), (ens.injection_state().block(),), what + ("injection",), R)
            assert_equal_by_reactor(ref_alarms(alm), alarms(ens), what + ("alarm",), R)
            assert_equal_by_reactor(ref_acts(act), acts(ens), what + ("actuator",), R)
            assert_equal_by_reactor((det.st, det.t_prev), ens.detector_state().block(), what + ("detector",), R)
            assert_equal_by_reactor((trd.st,), (ens.trend_state().block(),), what + ("trend",), R)
        assert done == STEPS
        # who stepped: the ensemble did what the roles say
        es = ens.state
        took = np.full(N, float(STEPS))
        took[never], took[stopped] = 0.0, float(STOP_AT)
        assert np.array_equal(es.time, took * DT), (n, interval)
        assert np.all(es.status[never] & 64) and np.all(es.status[stopped] & 1) and not (es.status[through] & FROZEN).any()
        assert np.array_equal(scans, -(-took // interval)), (n, interval)
        assert np.array_equal(ens.sensor_history()[3], took)
        d = ens.trend_data()
        held = trd.data()
        assert_equal_by_reactor(held, (d.time, d.value, d.count), (n, interval, "trend data"), R)
        # the disturbance and score programs against the recorded per-step times and true trajectory
        tr = ens.trajectory()
        assert len(tr) == STEPS
        if times is None:
            times = tr.time
            dst_ref = DR.DisturbRef(blocks["dst"], bc0, zero, seed=99, reactor_base=5, history=STEPS + 1)
            prev = zero
            for k in range(STEPS):
                dst_ref.evaluate(times[k], (times[k] != prev) & ((tr.status[k] & 32) == 0))
                prev = times[k]
        assert np.array_equal(tr.time, times), (n, interval)
        st = ens.disturbance_state()
        off, filled = ens.disturbance_history()
        got = ens.boundary()
        what = (n, interval, "disturbance")
        assert_equal_by_reactor((dst_ref.bc[[1, 5, 7, 9]], dst_ref.st[:, DR.DS_N_EVAL], dst_ref.st[:, DR.DS_N_DRAW], dst_ref.t_prev,
                                 dst_ref.st[:2, DR.DS_VALUE], dst_ref.hist[:, :2], dst_ref.n_filled(), dst_ref.base),
                                (got[[1, 5, 7, 9]], st.n_eval, st.n_draw, st.t_prev, st.value[:2], off[:, :2], filled, st.base), what, R)
        assert np.array_equal(got[3], dst_ref.bc[3]) and np.array_equal(got[7], dst_ref.bc[7]), what      # STEP and RAMP rows
        np.testing.assert_allclose(got[8], dst_ref.bc[8], rtol=0, atol=SINE_AMPLITUDE * 1e-13)     # SINE: 1e-13 of the amplitude
        np.testing.assert_allclose(got[2], dst_ref.bc[2], rtol=0, atol=1e-4 * OU_SIGMA)            # OU: 1e-4 sigma
        np.testing.assert_allclose(off[:, 2], dst_ref.hist[:, 2], rtol=0, atol=SINE_AMPLITUDE * 1e-13)
        np.testing.assert_allclose(off[:, 3], dst_ref.hist[:, 3], rtol=0, atol=1e-4 * OU_SIGMA)
        np.testing.assert_allclose(st.x[3], dst_ref.st[3, DR.DS_X], rtol=0, atol=1e-4 * OU_SIGMA)
        scr = SR.ScoreRef(blocks["scr"], zero, curve=STEPS, bins=BINS, fan_lo=p["fan"][0], fan_hi=p["fan"][1])
        scr.run(tr.pH, tr.chlorine, tr.temperature, tr.time, tr.status)
        sst, cv = ens.score_state(), ens.score_curve()
        assert_equal_by_reactor((scr.st, scr.t_prev), (np.stack([getattr(sst, k) for k in ROWS], axis=1), sst.t_prev),
                                (n, interval, "score"), R)
        assert len(cv.n_scored) == STEPS
        assert np.array_equal(np.stack([cv.n_scored, cv.n_low, cv.n_high], axis=2), scr.counts), (n, interval, "curve")
        assert np.array_equal(cv.fan, scr.fan), (n, interval, "fan")
        assert wavefront_groups(ens) == 6        # it ran as five full wavefront-groups and one that holds the last reactor
        ens.close()

        # ---- non-vacuity, on the restatements: the forced slots acted at every scan of every reactor that stepped,
        # the single-reactor group included; the realistic slots acted in a quarter of the reactors that stepped
        # throughout and stayed quiet in a quarter
        assert scans[N - 1] > 0 and np.all(scans[through] == scans.max())
        assert np.array_equal(ctl.st[:, CR.CS_N_EXEC] + ctl.st[:, CR.CS_N_HELD], np.stack([scans, scans]))
        assert np.array_equal(ctl.st[1, CR.CS_N_HELD], scans)                    # the pH probes warm up: the acid loop holds
        assert np.array_equal(inj.st[0, IR.IS_N_APPLIED], scans)
        assert np.array_equal(alm.st[0, LR.AS_N_ACT], (scans > 0).astype(float)) and np.array_equal(alm.st[0, LR.AS_ACTIVE], alm.st[0, LR.AS_N_ACT])
        assert np.array_equal(alm.rst[LR.AR_N_OVR_CHLORINE], np.maximum(scans - 1, 0))
        assert np.array_equal(act.st[1, AR.VS_N_EXEC], scans) and np.all(act.st[1, AR.VS_N_RATE] >= scans - 1)
        assert np.all(act.st[1, AR.VS_N_RATE][scans > 1] > 0)
        assert np.array_equal(det.st[0, KR.KS_N_EVAL], scans) and np.array_equal(det.st[0, KR.KS_N_ALARM], scans)
        assert np.array_equal(dst_ref.st[0, DR.DS_N_EVAL], took + 1) and np.array_equal((dst_ref.hist[:, 1] != 0).sum(axis=0), np.maximum(took - 2, 0))
        assert np.array_equal(scr.st[2, SR.S_N_EVAL], took) and np.array_equal(scr.st[2, SR.S_T_HIGH], took * DT)
        assert np.array_equal(alm.st[2, LR.AS_N_BAD], scans)                     # both on_bad policies ran on bad readings
        assert np.array_equal(det.st[2, KR.KS_N_BAD], scans)
        # every trend slot recorded at every reactor that was scanned, the lone one included: the first candidate always,
        # every candidate without a deadband; nothing was dropped, and the slots that record changes saw some
        every = blocks["trd"][:, TR.T_EVERY]
        assert np.array_equal(trd.st[:, TR.TS_N_SEEN], np.tile(scans, (8, 1))) and not trd.st[:, TR.TS_N_DROPPED].any()
        assert np.all(held[2][:, through] >= 1) and np.all(held[2][:, N - 1] >= 1) and not held[2][:, never].any()
        for slot in (0, 1, 4, 5, 7):
            assert np.array_equal(held[2][slot], -(-scans // every[slot])), (n, interval, slot)
        for slot in (2, 3, 6):
            assert (held[2][slot, through] > 1).any(), (n, interval, slot)
        assert np.isfinite(held[1][[0, 1, 2, 3, 4, 5, 7], 0][:, through]).all()     # state entries, the word and a fault code
        print("trend samples held per slot (min, max)", n, interval, [(int(c.min()), int(c.max())) for c in held[2][:, through]])
        chl = ctl.st[0]
        share = dict(
            pi=((chl[CR.CS_N_SAT] > 0), (chl[CR.CS_N_EXEC] > 0) & (chl[CR.CS_N_SAT] == 0)),
            injection=((inj.st[1, IR.IS_N_APPLIED] > 0), (inj.st[1, IR.IS_N_APPLIED] == 0)),
            tamper=((inj.st[2, IR.IS_N_APPLIED] > 0), (inj.st[2, IR.IS_N_APPLIED] == 0)),
            alarm=((alm.st[1, LR.AS_N_ACT] > 0), (alm.st[1, LR.AS_N_ACT] == 0)),
            actuator=((act.st[0, AR.VS_N_FAULT] > 0), (act.st[0, AR.VS_N_FAULT] == 0)),
            detector=((det.st[1, KR.KS_N_ALARM] > 0), (det.st[1, KR.KS_N_EVAL] > 0) & (det.st[1, KR.KS_N_ALARM] == 0)),
            disturbance=((dst_ref.hist[:, 0] != 0).any(axis=0), ~(dst_ref.hist[:, 0] != 0).any(axis=0)),
            score=((scr.st[0, SR.S_T_LOW] > 0), (scr.st[0, SR.S_N_EVAL] > 0) & (scr.st[0, SR.S_T_LOW] == 0) & (scr.st[0, SR.S_T_HIGH] == 0)))
        share = {k: (_shares(a, through), _shares(q, through)) for k, (a, q) in share.items()}
        print("shares (acted, quiet)", n, N, interval, {k: (round(a, 2), round(q, 2)) for k, (a, q) in share.items()})
        for k, (a, q) in share.items():
            assert a >= 0.25 and q >= 0.25, (n, interval, k, a, q)
        # windows opened and closed, delays drained, the curve saw a mixed ensemble
        last = inj.st[1, IR.IS_T_LAST][through]
        assert (last < T_END - interval * DT).any() and (alm.st[:, LR.AS_N_BAD] > 0).any()
        assert ((scr.counts[:, 0, 1] > 0) & (scr.counts[:, 0, 1] < scr.counts[:, 0, 0])).any()
        assert (scr.fan[STEPS - 1, 0, 1:-1] > 0).sum() >= 2


def _run_closed(wt, cols, bc, n, steps, *, chunk=7, streams=0, adaptive=False, per_call=None, dt=DT):
    """``dt``: the re-deal sorts the reactors by their mean RHS evaluations per outer step in eighths, 256 bins, so from
    32 evaluations per step on every reactor lands in the last bin and the stable sort deals the identity.  With 10 s
    steps that is what the re-deal gave at 16 and 17 zones; there the placement twins take 2 s steps, which move
    reactors (at 2 zones it is the 2 s steps that deal the identity)."""
    N = len(cols["initial_chlorine"])
    ens = _closed(wt, cols, bc, n, steps * dt)
    ens.set_placement(adaptive)
    ens.set_schedule(streams, chunk)
    ens.set_detectors(*_four(wt, N, steps * dt), attack=(0.2 * steps * dt, 0.6 * steps * dt))
    for c, _ in calls(steps, per_call or steps):
        ens.step(dt, n_steps=c, download=False)
    if adaptive:
        assert ens.schedule()["redeals"] >= 1 and not np.array_equal(ens.placement()[1], np.arange(N))
    out = everything(ens, programs=EVERYTHING) + ens.detector_state().block()
    assert wavefront_groups(ens) == 6
    ens.close()
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("n", ZONES)
def test_one_fused_call_equals_the_call_per_interval_loop(gpu, wt, full_waves, monkeypatch, n):
    """No host words between the calls: a scan in the middle of a work item, after which the reactor is reloaded, gives
    the bits of the call that ends with that scan."""
    R, N = ragged_size(n)
    steps = 60
    cols, bc = wt.make_ensemble(N, seed=1300 + n)
    fused = _run_closed(wt, cols, bc, n, steps)
    assert not (fused[5] & FROZEN).any()
    assert np.all(fused[-2][:, KR.KS_N_EVAL] == -(-steps // 7))           # every detector slot at every scan
    assert_all_equal(fused, _run_closed(wt, cols, bc, n, steps, per_call=7), (n, "a call per interval"))
    assert_all_equal(fused, _run_closed(wt, cols, bc, n, steps, streams=3), (n, "streams"))
    monkeypatch.setenv("WT_Q_TICKETS", "1")                            # the long-call split: one item per group and launch
    assert_all_equal(fused, _run_closed(wt, cols, bc, n, steps, chunk=7), (n, "tickets"))
    monkeypatch.delenv("WT_Q_TICKETS")
    # every call closes with a scan: five calls scan at other steps than one call, so they have their own twin
    dt = DT_PLACED.get(n, DT)
    five = _run_closed(wt, cols, bc, n, steps, per_call=steps // 5, dt=dt)
    assert_all_equal(five, _run_closed(wt, cols, bc, n, steps, per_call=steps // 5, dt=dt, adaptive=True), (n, "adaptive placement"))


@pytest.mark.gpu
@pytest.mark.parametrize("n", ZONES)
def test_programs_that_are_off_change_nothing(gpu, wt, full_waves, n):
    R, N = ragged_size(n)
    steps = 40
    cols, bc = wt.make_ensemble(N, seed=1400 + n)
    r = np.arange(N)
    outs = []
    for off in (False, True):
        ens = plant(wt, cols, bc, n)
        ens.set_placement(False)
        ens.set_schedule(0, 7)
        ens.write_commands(*MASTER)
        if off:
            ens.enable_control(wt.PILoop(r % 7, 1.0, kp=1.0, enable=0), wt.PILoop("pH_outlet", 7.0, kp=1.0, enable=0))
            ens.set_injections(*[wt.Injection(r % 10, "off", a=5.0)] * 4)
            ens.set_alarms(*[wt.Alarm(r % 7, "off", 5.0, action="trip_acid", trip_value=1.0)] * 4)
            ens.set_actuators()
            ens.set_detectors(*[wt.Detector(r % 7, "off", 1.0)] * 4)
            ens.set_disturbances(wt.Disturbance("inlet_pH"), wt.Disturbance(8, "off"), history=5)
            ens.set_scores(*[wt.Score("chlorine", 0.0, 1.0, kind="off")] * 4, curve=steps)
        ens.step(DT, n_steps=steps, download=False)
        outs.append(everything(ens, programs=()))
        if off:
            assert not ens.actuator_state().n_exec.any() and not ens.injection_state().n_applied.any()
            assert not ens.alarm_words().any() and not ens.score_state().n_eval.any() and not ens.detector_state().n_eval.any()
            assert np.all(ens.disturbance_state().n_eval == steps + 1)
        assert wavefront_groups(ens) == 6
        ens.close()
    assert not (outs[0][5] & FROZEN).any()
    assert_all_equal(outs[0], outs[1], (n, "all-OFF programs"))
