"""Per-reactor score programs after every outer step (include/wtphys.h ``wt_ensemble_score_*``): the device equals the
restatement in score_ref.py on the recorded trajectory bit for bit, a scored run computes the bits of an unscored one,
the results do not depend on the schedule, the placement or the sharding, the score sees what a spoofed image hides,
and the lifetime and error rules hold."""
import ctypes as C

import numpy as np
import pytest

import score_ref as SR
from program_helpers import DT, MASTER, SCAN_PROGRAMS, assert_all_equal, everything, pi_loops, plant, plant_state, refused_as_checked
from score_ref import ScoreRef

pytestmark = pytest.mark.gpu

INF = np.inf
FROZEN = 1 | 32 | 64          # WT_ST_T_RANGE, WT_ST_T_RANGE_POST, WT_ST_NONFINITE: the reactor stopped stepping
ROWS = ("n_eval", "time", "integral", "t_low", "t_high", "area_low", "area_high", "v_min", "v_max", "last", "out", "n_exc",
        "t_first_out", "run", "run_max")

# The open-loop study of test_equals_the_restatement: make_ensemble(128, seed=4242), 300 steps of 10 s, the chlorine
# stock (50 g/L) dropping by 45 for 600 <= t < 1000 and rising by 60 for 1600 <= t < 2000.  The numbers below come from
# the CPU oracle (wt_oracle.ensemble_step, the boundary's row 7 moved by hand) on that ensemble for n = 4, 8, 20, 32:
# the outlet chlorine's 30th / 70th percentile at step 150 was 1.59..1.67 / 2.60..2.73, its overall minimum 0.43..0.47
# and maximum 5.20..5.46.  With these bands the oracle run has 35..41 % of the reactors below at some time, 48..55 %
# above, 3..5 reactors with two or more excursions and a mixed ensemble at every step.
SEED, N_STUDY, K_STUDY = 4242, 128, 300
PULSES = ((-45.0, 600.0, 1000.0), (60.0, 1600.0, 2000.0))
CL_LO, CL_HI = 1.65, 2.70
FAN_LO, FAN_HI = 0.42, 5.47
BINS = 16


def _open(wt, cols, bc, n):
    ens = wt.ReactorEnsemble(cols, n_zones=n)
    ens.set_boundary(bc)
    return ens


def _four(wt):
    """Outlet chlorine ZONE, pH MEAN, temperature MAX, chlorine MIN with a window; their fan ranges."""
    return ((wt.Score("chlorine", CL_LO, CL_HI), wt.Score("pH", 6.5, 8.5, reduce="mean"),
             wt.Score("temperature", hi=25.0, reduce="max"), wt.Score("chlorine", lo=1.0, reduce="min", t_start=500.0, t_end=2500.0)),
            ([FAN_LO, 2.0, 9.0, 0.4], [FAN_HI, 9.0, 31.0, 5.5]))


def _pulses(wt):
    return [wt.Disturbance.step("chlorine_concentration", a, t0, t1) for a, t0, t1 in PULSES]


def _scores(ens):
    st, c = ens.score_state(), ens.score_curve()
    return tuple(getattr(st, k) for k in ROWS) + (st.t_prev, c.n_scored, c.n_low, c.n_high) + (() if c.fan is None else (c.fan,))


def _against(ref, ens, what):
    st, c = ens.score_state(), ens.score_curve()
    for i, k in enumerate(ROWS):
        assert np.array_equal(getattr(st, k), ref.st[:, i], equal_nan=True), (what, k)
    assert np.array_equal(st.t_prev, ref.t_prev), what
    K = len(c.n_scored)
    assert K == min(ref.j, ref.cap) and not ref.counts[K:].any()
    assert np.array_equal(np.stack([c.n_scored, c.n_low, c.n_high], axis=2), ref.counts[:K]), what
    if ref.fan is not None:
        assert np.array_equal(c.fan, ref.fan[:K]), what


@pytest.mark.parametrize("n", [4, 8, 20, 32])
def test_equals_the_restatement(gpu, wt, n):
    N, K = N_STUDY, K_STUDY
    cols, bc = wt.make_ensemble(N, seed=SEED)
    scores, (flo, fhi) = _four(wt)
    ens = _open(wt, cols, bc, n)
    ens.record(every=1, capacity=K)
    ens.set_disturbances(*_pulses(wt))
    ens.set_scores(*scores, curve=K, bins=BINS, fan_range=(flo, fhi))
    ens.step(DT, n_steps=K, download=False)
    tr = ens.trajectory()
    assert len(tr) == K and not (tr.status & FROZEN).any()
    ref = ScoreRef(wt.score_block(N, *scores), np.zeros(N), curve=K, bins=BINS, fan_lo=flo, fan_hi=fhi)
    ref.run(tr.pH, tr.chlorine, tr.temperature, tr.time, tr.status)
    # non-vacuity, on the restatement of the recorded trajectory (the reference side)
    cl = ref.st[0]
    assert (cl[SR.S_T_LOW] > 0).mean() >= 0.10 and (cl[SR.S_T_HIGH] > 0).mean() >= 0.10
    assert (cl[SR.S_N_EXC] >= 2).any()
    assert ((ref.counts[:, 0, 1] > 0) & (ref.counts[:, 0, 1] < ref.counts[:, 0, 0])).any()
    assert (ref.fan[K - 1, 0, 1:-1] > 0).sum() >= 3
    assert np.all(ref.st[3, SR.S_N_EVAL] == 200) and (ref.st[1:, SR.S_N_EVAL] > 0).all()
    _against(ref, ens, n)
    # quantile bands straight from the fan: ordered, inside the fan's range
    q = ens.score_curve().quantiles([0.1, 0.5, 0.9])[:, :, 0]
    assert np.all(q[0] <= q[1]) and np.all(q[1] <= q[2]) and q.min() >= FAN_LO and q.max() <= FAN_HI
    ens.close()


def _closed(wt, cols, bc, n, N, horizon):
    """Plant I/O with both PI loops, an injection, an alarm, an actuator and a disturbance program."""
    ens = plant(wt, cols, bc, n)
    ens.write_commands(*MASTER)
    chlorine, acid = pi_loops(wt, cols)
    ens.enable_control(chlorine, acid)
    ens.set_injections(wt.Injection("chlorine_outlet", "bias", start=0.2 * horizon, end=0.6 * horizon, a=0.8))
    ens.set_alarms(wt.Alarm("chlorine_outlet", "low", 1.0, deadband=0.1, source="field", action="trip_chlorine", trip_value=0.6))
    ens.set_actuators(wt.Actuator("chlorine", tau=40.0, rate=0.05), wt.Actuator("acid", delay=2))
    ens.set_disturbances(wt.Disturbance.ou("inlet_chlorine", 0.2, 300.0), wt.Disturbance.step("chlorine_concentration", -30.0, 0.3 * horizon, 0.7 * horizon),
                         seed=5)
    return ens


@pytest.mark.parametrize("n", [4, 8, 20, 32])
def test_changes_nothing(gpu, wt, n):
    N, K = 96, 60
    cols, bc = wt.make_ensemble(N, seed=700 + n)
    scores, fan = _four(wt)
    outs = []
    for scored in (False, True):
        ens = _closed(wt, cols, bc, n, N, K * DT)
        ens.set_schedule(0, 7)
        if scored:
            ens.set_scores(*scores, curve=K, bins=32, fan_range=fan)
        ens.step(DT, n_steps=K, download=False)
        outs.append(everything(ens, programs=SCAN_PROGRAMS + ("disturb",)))
        if scored:
            assert np.all(ens.score_state().n_eval[0] == K) and np.all(ens.score_curve().n_scored[:, 0] == N)
        ens.close()
    assert_all_equal(outs[0], outs[1], "score program")


def test_schedule_invariance(gpu, wt, monkeypatch):
    N, n, K = 160, 8, 70
    cols, bc = wt.make_ensemble(N, seed=61)
    scores, fan = _four(wt)
    scores = scores[:3] + (wt.Score("chlorine", lo=1.0, reduce="min", t_start=100.0, t_end=600.0),)

    def run(v):
        if v.get("tickets"):
            monkeypatch.setenv("WT_Q_TICKETS", "1")
        ens = _closed(wt, cols, bc, n, N, K * DT)
        ens.set_placement(v.get("adaptive", False))
        ens.set_schedule(v.get("streams", 0), v["chunk"])
        ens.set_scores(*scores, curve=K, bins=BINS, fan_range=fan)
        calls = v.get("calls", 1)
        for _ in range(calls):
            ens.step(DT, n_steps=K // calls, fused=v.get("fused", True), download=False)
        out = plant_state(ens) + _scores(ens)
        ens.close()
        monkeypatch.delenv("WT_Q_TICKETS", raising=False)
        return out

    ref = {c: run(dict(chunk=c)) for c in (1, 7, 50)}
    assert not (ref[7][5] & FROZEN).any() and ref[7][-4].sum() == 3 * K * N + 50 * N      # three open slots and a 500 s window
    # every call closes with a scan, and fused=False scans every step: those runs are the scan-every-step run
    for v, want in ((dict(streams=3, chunk=7), 7), (dict(chunk=7, tickets=True), 7), (dict(chunk=1, adaptive=True, calls=5), 1),
                    (dict(chunk=7, calls=K), 1), (dict(chunk=50, fused=False), 1)):
        assert_all_equal(ref[want], run(v), v)


def test_sharding_counts_add(gpu, wt):
    """Open loop (no per-reactor random streams to re-key): the curve of 2M reactors is the sum of its halves'."""
    M, n, K = 48, 4, 40
    cols, bc = wt.make_ensemble(2 * M, seed=SEED)
    bcb = wt.boundary_block(bc, 2 * M)
    scores, fan = _four(wt)
    scores = scores[:3] + (wt.Score("chlorine", lo=1.0, reduce="min", t_start=100.0, t_end=300.0),)

    def run(c, b):
        ens = _open(wt, c, b, n)
        ens.set_scores(*scores, curve=K, bins=BINS, fan_range=fan)
        ens.step(DT, n_steps=K, download=False)
        out = _scores(ens)
        ens.close()
        return out

    whole = run(cols, bc)
    parts = [run({k: np.asarray(v)[sl] for k, v in cols.items()}, bcb[:, sl]) for sl in (slice(0, M), slice(M, 2 * M))]
    for i in range(len(ROWS) + 1):
        assert np.array_equal(whole[i], np.concatenate([parts[0][i], parts[1][i]], axis=-1), equal_nan=True), i
    for i in range(len(ROWS) + 1, len(whole)):
        assert np.array_equal(whole[i], parts[0][i] + parts[1][i]), i
    assert 0 < whole[-3][:, 0].sum() < whole[-4][:, 0].sum()         # some, not all, below the band


def test_ground_truth_against_the_image(gpu, wt):
    """A spoof adds 1.5 mg/L to the chlorine_outlet reading of a PI loop that doses towards initial + 1 mg/L: the loop
    stops dosing and the true outlet chlorine sinks.  One limit (initial + 0.6 mg/L) for the score on the true state, an
    IMAGE alarm and a FIELD alarm: the score's time below grows, the instrument's own reading trips, the operator's
    image stays quiet.  Directions only: the chlorine analysers read well off the truth by the end of the run."""
    N, n, K = 64, 4, 300
    cols, bc = wt.make_ensemble(N, seed=45)
    init = np.asarray(cols["initial_chlorine"], dtype=np.float64)
    limit = init + 0.6
    res = []
    for spoofed in (False, True):
        ens = plant(wt, cols, bc, n)
        ens.set_schedule(0, 1)
        ens.write_commands(*MASTER)
        ens.enable_control(chlorine=wt.PILoop("chlorine_outlet", setpoint=init + 1.0, kp=2.0, ki=1e-3))
        if spoofed:
            ens.set_injections(wt.Injection("chlorine_outlet", "bias", start=500.0, a=1.5))
        ens.set_alarms(wt.Alarm("chlorine_outlet", "low", limit, source="image"),
                       wt.Alarm("chlorine_outlet", "low", limit, source="field"))
        ens.set_scores(wt.Score("chlorine", lo=limit))
        ens.step(DT, n_steps=K, download=False)
        res.append((ens.score_state(), ens.alarm_state()))
        ens.close()
    (s0, a0), (s1, a1) = res
    print("t_low", s0.t_low[0].sum(), s1.t_low[0].sum(), "area_low", s0.area_low[0].sum(), s1.area_low[0].sum(),
          "image active", a0.time_active[0].sum(), a1.time_active[0].sum(), "field active", a0.time_active[1].sum(), a1.time_active[1].sum())
    assert s1.t_low[0].sum() > s0.t_low[0].sum() and s1.area_low[0].sum() > s0.area_low[0].sum()
    assert np.all(s1.t_low[0] >= s0.t_low[0])
    assert a1.time_active[1].sum() > a0.time_active[1].sum() and a1.n_act[1].sum() > a0.n_act[1].sum()     # the FIELD alarm trips
    assert a1.time_active[0].sum() <= a0.time_active[0].sum() and a1.n_act[0].sum() <= a0.n_act[0].sum()   # the IMAGE alarm does not
    # at the end of the run: water in violation, the instrument in alarm, the image quiet
    assert ((s1.out[0] == 1) & (a1.active[1] == 1) & (a1.active[0] == 0)).any()


def test_errors_and_lifetime(gpu, wt):
    nat = gpu
    L = nat.lib()
    for nz in (33, 40):
        cols, bc = wt.make_ensemble(4, seed=1)
        ens = _open(wt, cols, bc, nz)
        with pytest.raises(ValueError, match="up to 32 zones"):
            ens.set_scores(wt.Score("pH"))
        ens.close()
    # before set_state, through the C ABI (the ensemble sets the state at creation); neither boundary nor sensors needed
    cols, bc = wt.make_ensemble(4, seed=2)
    ens = wt.ReactorEnsemble(cols, n_zones=4)
    h = C.c_void_p()
    nat.check(L.wt_ensemble_create(4, 4, 0, nat.dptr(np.ascontiguousarray(ens.constants)), C.byref(h)))
    blk = np.ascontiguousarray(wt.score_block(4, wt.Score("pH")))
    assert L.wt_ensemble_score_set(h, nat.dptr(blk), 0, 0, None, None) == nat.WT_E_STATE
    assert L.wt_ensemble_score_get(h, None, None) == nat.WT_E_STATE
    assert L.wt_ensemble_score_curve(h, None, None, None) == nat.WT_E_STATE
    assert L.wt_ensemble_score_reset(h) == nat.WT_E_STATE and L.wt_ensemble_score_clear(h) == nat.WT_OK
    L.wt_ensemble_destroy(h)
    ens.set_scores(wt.Score("pH"))           # no boundary yet
    ens.close()

    N, n, K = 32, 4, 12
    cols, bc = wt.make_ensemble(N, seed=3)
    ens = _open(wt, cols, bc, n)
    with pytest.raises(ValueError, match="no score program"):
        ens.score_state()
    # a refused block gives wt_program_check's message; zone >= n is the set call's own check
    bad = np.ascontiguousarray(wt.score_block(N, wt.Score("pH")))
    bad[0, 2] = 7.0
    with pytest.raises(ValueError, match="reduce must be"):
        ens._program_call(L.wt_ensemble_score_set, nat.dptr(bad), 0, 0, None, None)
    assert refused_as_checked(nat, nat.WT_PROG_SCORE, bad)
    for zone in (n, 31):
        with pytest.raises(ValueError, match="below the ensemble's zone count"):
            ens.set_scores(wt.Score("pH", zone=zone))
    ens.set_scores(wt.Score("pH", zone=n - 1), wt.Score("pH"))
    for kw, msg in ((dict(curve=-1), "curve_capacity"), (dict(curve=4, bins=33, fan_range=(0, 1)), "bins must be"),
                    (dict(curve=4, bins=4, fan_range=(1.0, 1.0)), "fan_lo < fan_hi"), (dict(curve=4, bins=4, fan_range=(0.0, INF)), "fan_lo < fan_hi")):
        with pytest.raises(ValueError, match=msg):
            ens.set_scores(wt.Score("pH"), **kw)
    # the refused calls left the program in place; zone n-1 and zone -1 are the same zone
    ens.step(DT, n_steps=3, download=False)
    st = ens.score_state()
    assert np.array_equal(st.last[0], st.last[1]) and np.array_equal(st.last[0], ens.state.pH[:, -1]) and np.all(st.n_eval[:2] == 3)
    # C = 0 and B = 0 allocate nothing; the per-reactor rows work
    c = ens.score_curve()
    assert c.n_scored.shape == (0, 4) and c.fan is None and c.edges is None
    # set twice replaces the program: new parameters, fresh accumulators, a fresh curve
    ens.set_scores(wt.Score("temperature", hi=0.0, reduce="max"), curve=5, bins=4, fan_range=(0.0, 40.0))
    st = ens.score_state()
    assert not st.n_eval.any() and np.all(np.isnan(st.v_min)) and np.all(np.isnan(st.last)) and np.all(np.isnan(st.t_first_out))
    assert np.array_equal(st.t_prev, ens.state.time) and np.all(st.t_prev == 3 * DT) and len(ens.score_curve().n_scored) == 0
    ens.step(DT, n_steps=3, download=False)
    ens.step(DT, n_steps=K - 3, download=False)
    st, c = ens.score_state(), ens.score_curve()
    assert np.all(st.n_eval[0] == K) and np.all(st.t_high[0] == K * DT) and np.all(st.t_first_out[0] == 4 * DT) and not st.n_eval[1:].any()
    # the curve stops at its capacity
    assert c.n_scored.shape == (5, 4) and np.all(c.n_scored[:, 0] == N) and np.all(c.n_high[:, 0] == N) and not c.n_low.any()
    assert c.fan.shape == (5, 4, 6) and np.all(c.fan[:, 0].sum(axis=1) == N) and not c.fan[:, 1:].any() and c.edges.shape == (4, 5)
    # entries beyond n_steps are 0 (the raw buffers)
    ens.reset_scores()
    ens.step(DT, n_steps=2, download=False)
    counts, fan, k = np.full((5, 4, 3), -1, dtype=np.int32), np.full((5, 4, 6), -1, dtype=np.int32), C.c_int(-1)
    i32p = C.POINTER(C.c_int32)
    nat.check(L.wt_ensemble_score_curve(ens._h, counts.ctypes.data_as(i32p), fan.ctypes.data_as(i32p), C.byref(k)))
    assert k.value == 2 and np.all(counts[:2, 0, 0] == N) and not counts[2:].any() and not fan[2:].any()
    # reset restored the set-time values and restarted j; the parameters stayed
    st = ens.score_state()
    assert np.all(st.n_eval[0] == 2) and np.all(st.time[0] == 2 * DT) and np.all(st.t_first_out[0] == (K + 3 + 1) * DT)
    ens.reset_scores()
    st = ens.score_state()
    assert not st.n_eval.any() and np.all(np.isnan(st.v_max)) and np.array_equal(st.t_prev, ens.state.time) and len(ens.score_curve().n_scored) == 0
    # clear frees the buffers; the calls then give WT_E_STATE
    ens.clear_scores()
    for call in (ens.score_state, ens.score_curve, ens.reset_scores):
        with pytest.raises(ValueError, match="no score program"):
            call()
    ens.clear_scores()
    ens.step(DT, n_steps=2, download=False)
    ens.close()


def test_frozen_reactors_stop_accumulating(gpu, wt):
    from conftest import golden_json
    g = golden_json("g4_faults.json")["cold_run"]
    cfg = wt.ReactorConfiguration(**g["config"])
    b = wt.BoundaryConditions(**dict(zip(wt.params.BOUNDARY_FIELDS, g["bc"])))
    ens = wt.ReactorEnsemble([cfg, wt.ReactorConfiguration(n_zones=4)])
    ens.set_boundary([b, wt.BoundaryConditions()])
    Kc = 60
    ens.set_scores(wt.Score("temperature", lo=-INF, hi=INF, reduce="min"), curve=Kc)
    es = ens.step(1.0, n_steps=Kc)
    st, c = ens.score_state(), ens.score_curve()
    assert es.status[0] & 1 and es.time[0] < Kc and es.time[1] == Kc
    assert st.t_prev.tolist() == [es.time[0], Kc] and st.n_eval[0].tolist() == [es.time[0], Kc]
    assert st.time[0].tolist() == [es.time[0], Kc]
    k0 = int(es.time[0])
    assert np.all(c.n_scored[:k0, 0] == 2) and np.all(c.n_scored[k0:, 0] == 1)
    ens.close()
    # a non-finite state: the reactor never steps
    N, n = 8, 4
    cols, bc = wt.make_ensemble(N, seed=6)
    ens = _open(wt, cols, bc, n)
    pH = np.full((N, n), 7.0); pH[3, 1] = np.nan
    ens.set_state(pH, 1.0, 20.0, 0.0)
    ens.set_scores(wt.Score("pH", reduce="mean"), curve=4)
    ens.step(DT, n_steps=4, download=False)
    st = ens.score_state()
    assert st.n_eval[0, 3] == 0 and np.isnan(st.last[0, 3]) and np.all(np.delete(st.n_eval[0], 3) == 4)
    assert np.all(ens.score_curve().n_scored[:, 0] == N - 1)
    ens.close()
