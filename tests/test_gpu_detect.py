"""Per-reactor anomaly detector programs at every PLC scan (include/wtphys.h ``wt_ensemble_detect_*``): the device's
detector state is the restatement in detect_ref.py bit for bit, the program changes nothing else, its answers depend on
the scan times only, and a replay study comes out the way the statistics say it must."""
import numpy as np
import pytest

from conftest import golden_json
from detect_ref import DetectRef
from inject_ref import InjectRef
from program_helpers import DT, K, MASTER, SCAN_PROGRAMS, HostScan, assert_all_equal, everything, pi_loops, plant, refused_as_checked

pytestmark = pytest.mark.gpu

CL, PH = 3, 1                      # chlorine_outlet, pH_outlet in the sensor suite's order
T0, T1 = 2000.0, 2600.0            # the attack window: after the pH probes' 1800 s warm-up, inside the 3000 s run
CAL0 = 1000.0                      # calibration window [CAL0, T0): the PI loops' start-up transient is not the residual
# attack magnitudes in units of the pilot's per-reactor sigma, and the per-reactor limits (a decade each)
BIAS_SIGMA, RAMP_SIGMA_PER_100S = 8.0, 3.0
EWMA_LIMITS, CUSUM_LIMITS, FLAT_LIMITS, CROSS_LIMITS = (1.0, 10.0), (4.0, 40.0), (30.0, 300.0), (1.0, 10.0)


def _spread(lo_hi, N, seed):
    """Per-reactor limits spread log-uniformly over ``lo_hi``, in an order unrelated to the attack groups."""
    return np.random.default_rng(seed).permutation(np.geomspace(lo_hi[0], lo_hi[1], N))


def _pilot(wt, cols, bc, n, interval, loops):
    """The plant under PI control without the programs: per-reactor mean and standard deviation of the field history of
    chlorine_outlet and pH_outlet over the calibration window before the attack."""
    ens = plant(wt, cols, bc, n, history=K)
    ens.set_schedule(0, interval)
    ens.enable_control(*loops)
    ens.step(DT, n_steps=K, download=False)
    vh, _, _, filled = ens.sensor_history()
    ens.close()
    assert np.all(filled == K)
    t = DT * np.arange(1, K + 1)
    w = vh[(t >= CAL0) & (t < T0)].astype(np.float64)
    few = np.isfinite(w).sum(axis=0) < 10                              # (the pH probes read from 1800 s on)
    w[:, few] = 0.0
    mu, sd = np.nanmean(w, axis=0), np.nanstd(w, axis=0)
    # an instrument that read fewer than ten values in the window (a fault, a long warm-up) gets the ensemble's medians
    for i in (CL, PH):
        assert few[i].mean() < 0.1, (i, few[i].mean())
        mu[i, few[i]], sd[i, few[i]] = np.median(mu[i, ~few[i]]), np.median(sd[i, ~few[i]])
    assert np.all(sd[[CL, PH]] > 0)
    return mu, sd


def _attacks(wt, N, sd):
    """BIAS, RAMP and FREEZE in disjoint quarters of the reactors, a DROPOUT window in half of the RAMP quarter, the last
    quarter clean.  Returns the injections and the group of every reactor (3: clean)."""
    g = np.arange(N) % 4
    mode = lambda on, name: np.where(on, name, "off")
    return [wt.Injection("chlorine_outlet", mode(g == 0, "bias"), start=T0, end=T1, a=BIAS_SIGMA * sd[CL]),
            wt.Injection("pH_outlet", mode(g == 1, "ramp"), start=T0, end=T1, b=RAMP_SIGMA_PER_100S * sd[PH] / 100.0),
            wt.Injection("chlorine_outlet", mode(g == 2, "freeze"), start=T0, end=T1),
            wt.Injection("chlorine_outlet", mode(np.arange(N) % 8 == 1, "dropout"), start=T0 + 100.0, end=T1)], g


def _detectors(wt, N, mu, sd, seed):
    """All three kinds, all three references, both sources, both bad-reading policies, per-reactor limits over a decade."""
    return [wt.Detector("chlorine_outlet", "ewma", _spread(EWMA_LIMITS, N, seed), sigma=sd[CL], ref_value=mu[CL], t_arm=CAL0),
            wt.Detector("chlorine_outlet", "cusum", _spread(CUSUM_LIMITS, N, seed + 1), sigma=sd[CL], slack=1.5, ref="track",
                        tau=100.0, t_arm=100.0, on_bad="alarm"),
            wt.Detector("chlorine_outlet", "flatline", _spread(FLAT_LIMITS, N, seed + 2)),
            wt.Detector("pH_outlet", "cusum", _spread(CROSS_LIMITS, N, seed + 3), sigma=sd[PH], source="field",
                        ref="pH_outlet", ref_source="image")]


def _restate(wt, ens, N, interval, iblock, dblock, labels):
    """The restatement fed the instruments' own history at the scan steps and InjectRef's tampered copy of it."""
    vh, _, fh, filled = ens.sensor_history()
    assert np.all(filled == K)
    ref = DetectRef(dblock, labels, np.zeros(N))
    hs = HostScan(N, inj=InjectRef(iblock), det=ref)
    k = -1
    for steps in hs.calls(K, interval):
        k += steps
        hs.scan(vh[k], fh[k])
    return ref


def study(wt, n, N, interval, seed=321):
    """One self-calibrated run: returns the open ensemble, the restatement, the attack groups and the label."""
    cols, bc = wt.make_ensemble(N, seed=seed)
    loops = pi_loops(wt, cols)
    mu, sd = _pilot(wt, cols, bc, n, interval, loops)
    injections, g = _attacks(wt, N, sd)
    iblock = wt.injection_block(N, *injections)
    start, end = wt.attack_window(iblock)
    detectors = _detectors(wt, N, mu, sd, seed=n)
    ens = plant(wt, cols, bc, n, history=K)
    ens.set_schedule(0, interval)
    ens.enable_control(*loops)
    ens.set_injections(*injections)
    ens.set_detectors(*detectors, attack=(start, end))
    ens.step(DT, n_steps=K, download=False)
    assert not ens.state.status.any()
    labels = np.stack([start, end])
    ref = _restate(wt, ens, N, interval, iblock, wt.detector_block(N, *detectors), labels)
    return ens, ref, g, labels


def shares(ref, g):
    """The non-vacuity figures of one run of the restatement."""
    st = ref.st
    attacked, clean = g != 3, g == 3
    fp = (st[:, 14] > 0).any(axis=0)
    return dict(detected=np.isfinite(st[:, 12]).any(axis=0)[attacked].mean(), clean_fp=fp[clean].mean(),
                clean_quiet=(~fp)[clean].mean(), alarm_scans=st[:, 9].sum(axis=1).tolist(), max_raise=st[:, 10].max(),
                bad_hold=st[[0, 2, 3], 8].sum(), bad_alarm=st[1, 8].sum())


@pytest.mark.parametrize("n, N", [(4, 2000), (8, 2000), (20, 1000), (32, 500)])
def test_device_equals_the_restatement(gpu, wt, n, N):
    """Shares observed on the MI355X are recorded in DESIGN.md section 7.11."""
    for interval in (1, 7, 50):
        ens, ref, g, labels = study(wt, n, N, interval)
        s = shares(ref, g)
        print(n, interval, s)
        assert np.array_equal(labels[0, g == 3], np.full((g == 3).sum(), np.inf)) and np.all(labels[0, g != 3] == T0)
        assert s["detected"] >= 0.25, (n, interval, s)
        assert s["clean_fp"] >= 0.05 and s["clean_quiet"] >= 0.25, (n, interval, s)
        assert all(a > 0 for a in s["alarm_scans"][:3]), (n, interval, s)          # every kind has alarm scans
        assert s["max_raise"] >= 2 and s["bad_hold"] > 0 and s["bad_alarm"] > 0, (n, interval, s)
        got = ens.detector_state()
        assert_all_equal((ref.st, ref.t_prev), got.block(), (n, interval, "detector state"))
        assert np.array_equal(got.label_start, labels[0]) and np.array_equal(got.label_end, labels[1])
        ens.close()


def _closed(wt, cols, bc, n, horizon):
    """Plant I/O with both PI loops, an injection, an alarm, an actuator, a disturbance and a score program."""
    ens = plant(wt, cols, bc, n)
    ens.write_commands(*MASTER)
    ens.enable_control(*pi_loops(wt, cols))
    ens.set_injections(wt.Injection("chlorine_outlet", "bias", start=0.2 * horizon, end=0.6 * horizon, a=0.8))
    ens.set_alarms(wt.Alarm("chlorine_outlet", "low", 1.0, deadband=0.1, source="field", action="trip_chlorine", trip_value=0.6))
    ens.set_actuators(wt.Actuator("chlorine", tau=40.0, rate=0.05), wt.Actuator("acid", delay=2))
    ens.set_disturbances(wt.Disturbance.ou("inlet_chlorine", 0.2, 300.0),
                         wt.Disturbance.step("chlorine_concentration", -30.0, 0.3 * horizon, 0.7 * horizon), seed=5)
    ens.set_scores(wt.Score("chlorine", 0.5, 3.0), wt.Score("pH", 6.5, 8.5, reduce="mean"), curve=8)
    return ens


EVERYTHING = SCAN_PROGRAMS + ("disturb", "score")           # all that _closed sets


def _four(wt, N, horizon):
    lim = np.geomspace(0.5, 5.0, N)
    return [wt.Detector("chlorine_outlet", "cusum", lim, sigma=0.05, ref="track", tau=100.0),
            wt.Detector("pH_outlet", "ewma", 0.5 * lim, sigma=0.02, ref_value=7.0, source="field", on_bad="alarm"),
            wt.Detector("chlorine_outlet", "flatline", 3 * DT, slack=0.01),
            wt.Detector("chlorine_outlet", "cusum", lim, sigma=0.05, ref="chlorine_outlet", ref_source="field")]


@pytest.mark.parametrize("n", [4, 8, 20, 32])
def test_changes_nothing(gpu, wt, n):
    N, steps = 96, 60
    cols, bc = wt.make_ensemble(N, seed=800 + n)
    outs = []
    for variant in ("none", "four", "off", "cleared"):
        ens = _closed(wt, cols, bc, n, steps * DT)
        ens.set_schedule(0, 7)
        if variant == "four":
            ens.set_detectors(*_four(wt, N, steps * DT), attack=(0.2 * steps * DT, 0.6 * steps * DT))
        elif variant == "off":
            ens.set_detectors(*[wt.Detector(np.arange(N) % 7, "off", 1.0)] * 4)
        elif variant == "cleared":
            ens.set_detectors(*_four(wt, N, steps * DT))
            ens.clear_detectors()
        ens.step(DT, n_steps=steps, download=False)
        outs.append(everything(ens, programs=EVERYTHING))
        if variant == "four":
            st = ens.detector_state()
            assert np.all(st.n_eval == 9) and st.n_alarm[3].sum() > 0 and st.n_tp.sum() > 0 and st.n_bad[1].sum() > 0
        elif variant == "off":
            st = ens.detector_state()
            assert not np.nan_to_num(st.block()[0]).any() and np.all(st.t_prev == steps * DT)
        ens.close()
    for v, o in zip(("four", "off", "cleared"), outs[1:]):
        assert_all_equal(outs[0], o, v)


def test_schedules_placement_and_calls(gpu, wt, monkeypatch):
    N, n, steps = 3000, 8, 200
    cols, bc = wt.make_ensemble(N, seed=2025)
    loops = pi_loops(wt, cols, seed=9)
    dets = _four(wt, N, steps * DT)

    def run(chunk, streams=0, fused=True, calls=1, tickets=False, adaptive=False):
        if tickets:
            monkeypatch.setenv("WT_Q_TICKETS", "1")
        ens = plant(wt, cols, bc, n)
        ens.set_placement(adaptive)
        ens.set_schedule(streams, chunk)
        ens.enable_control(*loops)
        ens.set_injections(wt.Injection("chlorine_outlet", "bias", start=500.0, end=1200.0, a=0.3))
        ens.set_detectors(*dets, attack=(500.0, 1200.0))
        for _ in range(calls):
            ens.step(DT, n_steps=steps // calls, fused=fused, download=False)
        if adaptive:
            assert ens.schedule()["redeals"] >= 1 and not np.array_equal(ens.placement()[1], np.arange(N))
        out = ens.detector_state().block()
        ens.close()
        monkeypatch.delenv("WT_Q_TICKETS", raising=False)
        return out

    base = {c: run(c) for c in (1, 7, 50)}
    assert base[1][0][:, 7].sum() > base[7][0][:, 7].sum() > base[50][0][:, 7].sum() > 0   # other scan times, other answers
    assert base[1][0][:, 9].sum() > 0 and not np.array_equal(base[1][0][:, 4], base[7][0][:, 4], equal_nan=True)
    for v in (dict(streams=3), dict(fused=False), dict(calls=steps), dict(tickets=True), dict(adaptive=True, calls=5)):
        assert_all_equal(base[1], run(1, **v), v)
    assert_all_equal(base[7], run(7, streams=3), "streams, chunk 7")
    assert_all_equal(base[7], run(7, tickets=True), "tickets, chunk 7")


def test_replay_study(gpu, wt):
    """Directions only: a replay of chlorine_outlet under PI dosing is seen by the flat-line check on the image and by the
    image-against-field cross-check, not by the flat-line check on the instrument's own reading; lower CUSUM limits
    detect at least as often as higher ones."""
    N, n, interval = 2000, 8, 5
    cols, bc = wt.make_ensemble(N, seed=77)
    loops = pi_loops(wt, cols)
    mu, sd = _pilot(wt, cols, bc, n, interval, loops)
    attacked = np.arange(N) % 2 == 0
    replay = wt.Injection("chlorine_outlet", np.where(attacked, "freeze", "off"), start=T0, end=T1)
    label = wt.attack_window(wt.injection_block(N, replay))
    flat = 100.0
    limits = _spread((2.0, 200.0), N, 5)
    ens = plant(wt, cols, bc, n)
    ens.set_schedule(0, interval)
    ens.enable_control(*loops)
    ens.set_injections(replay)
    ens.set_detectors(wt.Detector("chlorine_outlet", "flatline", flat), wt.Detector("chlorine_outlet", "flatline", flat, source="field"),
                      wt.Detector("chlorine_outlet", "cusum", 5.0, sigma=sd[CL], ref="chlorine_outlet", ref_source="field"),
                      wt.Detector("chlorine_outlet", "cusum", limits, sigma=sd[CL], ref="chlorine_outlet", ref_source="field"),
                      attack=label)
    ens.step(DT, n_steps=K, download=False)
    st = ens.detector_state()
    ens.close()
    tpr, fpr, delay = st.rates()
    found = np.isfinite(st.t_detect)
    in_time = found[0] & (delay[0] <= flat + 2 * interval * DT)
    assert in_time[attacked].mean() >= 0.9, in_time[attacked].mean()
    assert (st.n_tp[1] == 0)[attacked].mean() >= 0.9                          # the instrument itself keeps moving
    # the cross-check's residual is exactly zero without an attack, so it never alarms in a clean reactor; how far the true
    # chlorine moves away from the replayed value within the window depends on the plant, so "detects" takes the floor the
    # bit-exactness test uses for a detection share that means something: a quarter of the attacked reactors
    print("replay: flat-line in time", in_time[attacked].mean(), "cross-check", found[2][attacked].mean())
    assert found[2][attacked].mean() >= 0.25, found[2][attacked].mean()
    assert not found[2][~attacked].any() and not st.n_alarm[2][~attacked].any()
    assert np.isnan(delay[:, ~attacked]).all() and np.isnan(tpr[:, ~attacked]).all()
    order = np.argsort(limits[attacked])
    share = found[3][attacked][order]
    q = len(share) // 4
    assert share[:q].mean() >= share[-q:].mean(), (share[:q].mean(), share[-q:].mean())
    assert share[:q].mean() > 0


def test_errors_and_lifetime(gpu, wt):
    from importlib import import_module
    nat = import_module("ics-wt-physicsengine_amd.core._native")
    N, n = 256, 4
    cols, bc = wt.make_ensemble(N, seed=12)
    # z > 0 at every scan, or the reading is bad: an alarm either way
    flow = wt.Detector("flow_main", "cusum", 1.0, slack=0.0, ref_value=-1.0, source="field", on_bad="alarm")
    ens = wt.ReactorEnsemble(cols, n_zones=n)
    ens.set_boundary(bc)
    with pytest.raises(ValueError, match="plant I/O"):
        ens.set_detectors(flow)
    ens.enable_sensors(seed=4)
    with pytest.raises(ValueError, match="plant I/O"):
        ens.set_detectors(flow)
    ens.enable_plant_io()
    for call in (ens.detector_state, ens.reset_detectors):
        with pytest.raises(ValueError, match="no detector program"):
            call()
    assert nat.lib().wt_ensemble_detect_get(ens._h, None, None) == nat.WT_E_STATE
    assert nat.lib().wt_ensemble_detect_reset(ens._h) == nat.WT_E_STATE
    for big in (33, 40):                                         # the n > 32 kernel carries no detector section
        other = plant(wt, cols, bc, big)
        with pytest.raises(ValueError, match="up to 32 zones"):
            other.set_detectors(flow)
        with pytest.raises(ValueError, match="no detector program"):
            other.detector_state()
        other.close()
    with pytest.raises(ValueError, match="at most 4"):
        ens.set_detectors(*[flow] * 5)
    with pytest.raises(ValueError, match="sigma must be > 0"):
        ens.set_detectors(wt.Detector(3, "ewma", 1.0, sigma=0.0))
    good = wt.detector_block(N, flow, wt.Detector("pH_inlet", "ewma", 1.0, ref="pH_outlet"))
    never = np.full((2, N), np.inf)
    for slot, row, value in ((0, 0, 4.0), (0, 1, 7.0), (0, 2, 2.0), (0, 3, 3.0), (0, 4, np.nan), (0, 7, 0.0), (0, 8, -1.0),
                             (0, 9, 0.0), (0, 10, np.inf), (0, 11, 2.0), (1, 4, 7.0), (1, 5, 2.0), (1, 8, 1.5)):
        bad = good.copy()
        bad[slot, row, 17] = value
        assert nat.lib().wt_ensemble_detect_set(ens._h, nat.dptr(bad), nat.dptr(never)) == nat.WT_E_ARG, (slot, row, value)
        assert refused_as_checked(nat, nat.WT_PROG_DETECT, bad), (slot, row, value)
    for start, end, message in ((np.nan, 5.0, "must not be NaN"), (0.0, np.nan, "must not be NaN"), (5.0, 4.0, "label_end must be >= label_start"),
                                (np.inf, 0.0, "label_end must be >= label_start")):
        with pytest.raises(ValueError, match=message):
            ens.set_detectors(flow, attack=(np.where(np.arange(N) == 9, start, 0.0), np.where(np.arange(N) == 9, end, 1.0)))
    assert nat.lib().wt_ensemble_detect_set(ens._h, nat.dptr(good), None) == nat.WT_E_ARG
    with pytest.raises(ValueError, match="no detector program"):
        ens.detector_state()                                     # a refused program leaves none behind
    ens.set_schedule(0, 5)
    ens.write_commands(*MASTER)
    ens.step(DT, n_steps=10, download=False)
    ens.set_detectors(flow, attack=(-np.inf, 200.0))
    st = ens.detector_state()
    assert np.all(st.t_prev == 100.0) and not np.nan_to_num(st.block()[0]).any() and np.isnan(st.t_detect).all()
    assert np.isnan(st.baseline).all() and np.isnan(st.x_prev).all() and np.isnan(st.t_first).all()
    ens.step(DT, n_steps=30, download=False)                     # six scans, 150 ... 400 s; the flow reads > -1 at each
    st = ens.detector_state()
    assert np.all(st.n_eval[0] == 6) and np.all(st.n_alarm[0] == 6) and np.all(st.n_raise[0] == 1) and np.all(st.t_first[0] == 150.0)
    assert np.all(st.n_tp[0] == 1) and np.all(st.n_fp[0] == 5) and np.all(st.t_detect[0] == 150.0) and not st.n_eval[1:].any()
    assert np.all(st.rates()[0][0] == 1.0) and np.isnan(st.rates()[2]).all()     # no delay from a label that starts at -inf
    ens.reset_detectors()                                        # the state starts over at the current loop time, the label stays
    st = ens.detector_state()
    assert np.all(st.t_prev == 400.0) and not np.nan_to_num(st.block()[0]).any() and np.isnan(st.x_prev).all()
    ens.step(DT, n_steps=10, download=False)
    st = ens.detector_state()
    assert np.all(st.n_eval[0] == 2) and np.all(st.n_fp[0] == 2) and np.all(st.t_first[0] == 450.0) and np.all(st.label_end == 200.0)
    ens.set_detectors(wt.Detector("flow_main", "flatline", 1e6), flow)     # set twice replaces: new slots, fresh state, new label
    st = ens.detector_state()
    assert not st.n_eval.any() and np.all(st.t_prev == 500.0) and np.all(np.isinf(st.label_start))
    ens.step(DT, n_steps=5, download=False)
    st = ens.detector_state()
    assert np.all(st.n_eval[:2] == 1) and not st.n_alarm[0].any() and np.all(st.n_fp[1] == 1) and np.isnan(st.t_detect).all()
    ens.clear_detectors()
    with pytest.raises(ValueError, match="no detector program"):
        ens.detector_state()
    with pytest.raises(ValueError, match="no detector program"):
        ens.reset_detectors()
    ens.clear_detectors()                                        # no effect while none is set
    ens.step(DT, n_steps=5, download=False)
    ens.close()
    # a reactor frozen by WT_ST_T_RANGE is not read, so its detectors are not evaluated any more
    g = golden_json("g4_faults.json")["cold_run"]
    cfg = wt.ReactorConfiguration(**g["config"])
    b = wt.BoundaryConditions(**dict(zip(wt.params.BOUNDARY_FIELDS, g["bc"])))
    ens = wt.ReactorEnsemble([cfg, wt.ReactorConfiguration(n_zones=4)])
    ens.set_boundary([b, wt.BoundaryConditions()])
    ens.enable_sensors(seed=1)
    ens.enable_plant_io()
    ens.write_commands([b.acid_flow_rate, 0.0], [b.chlorine_flow_rate, 0.0], [b.inlet_flow_rate, 1.0])
    ens.set_schedule(0, 1)
    ens.set_detectors(flow)
    Kc = 60
    es = ens.step(1.0, n_steps=Kc)
    st = ens.detector_state()
    assert es.status[0] & 1 and es.time[0] < Kc and es.time[1] == Kc
    assert st.t_prev[0] == es.time[0] and st.n_eval[0, 0] == es.time[0] and st.t_prev[1] == Kc and st.n_eval[0, 1] == Kc
    ens.close()
