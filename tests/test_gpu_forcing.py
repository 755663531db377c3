"""Per-step boundary schedules and trajectory recording in fused calls (ReactorEnsemble.step(boundary_schedule=...),
ReactorEnsemble.record / .trajectory): one scheduled call gives the bits of the host loop set_boundary(S[k]) +
step(dt, 1) under every launch schedule, follows the reference's forced runs (g13) and the oracle at full size; the
records are the per-step snapshots, indexed by reactor."""
import numpy as np
import pytest

from conftest import cfg_columns, golden_json, golden_npz, relerr

pytestmark = pytest.mark.gpu

TOL = 1e-6


def _outputs(ens, es):
    return (es.pH, es.chlorine, es.temperature, es.H_concentration, es.density, es.chlorine_decay_rate, es.time,
            es.flow_rate, es.status, ens.solver_stats(), ens.boundary())


def _loop(wt, cols, n, S, dt=1.0, setup=None):
    """The host loop a scheduled call replaces: set_boundary(row k), one step, a snapshot."""
    ens = wt.ReactorEnsemble(cols, n_zones=n)
    if setup:
        setup(ens)
    snaps = []
    for k in range(S.shape[0]):
        ens.set_boundary(S[k])
        snaps.append(ens.step(dt, n_steps=1))
    return ens, snaps


def _assert_equal(ref, got, what):
    for i, (a, b) in enumerate(zip(ref, got)):
        assert np.array_equal(a, b, equal_nan=True), (what, i)


@pytest.mark.parametrize("n", [4, 8, 20])
def test_scheduled_call_equals_the_host_loop(gpu, wt, monkeypatch, n):
    N, K = 3000, 24
    cols, bc = wt.make_ensemble(N, seed=4242)
    S = wt.make_boundary_schedule(bc, K, seed=17)
    ens, snaps = _loop(wt, cols, n, S)
    ref = _outputs(ens, snaps[-1])
    ens.close()
    variants = [dict(streams=0, chunk=50), dict(streams=1, chunk=0), dict(streams=3, chunk=7), dict(streams=0, chunk=1),
                dict(streams=0, chunk=50, fused=False), dict(streams=0, chunk=5, tickets=True)]
    for v in variants:
        if v.get("tickets"):
            monkeypatch.setenv("WT_Q_TICKETS", "1")            # the long-call split: one item per group and launch
        ens = wt.ReactorEnsemble(cols, n_zones=n)
        ens.set_schedule(v["streams"], v["chunk"])
        if v.get("tickets"):
            assert ens.item_steps(K) < K
        es = ens.step(1.0, n_steps=K, boundary_schedule=S, fused=v.get("fused", True))
        _assert_equal(ref, _outputs(ens, es), v)
        assert np.array_equal(ens.boundary(), S[-1])
        ens.close()
        monkeypatch.delenv("WT_Q_TICKETS", raising=False)


@pytest.mark.parametrize("n", [4, 8, 20])
def test_forced_single_reactor_vs_reference(gpu, wt, n):
    """The reference's forced runs (tools/gen_golden_forcing.py): one scheduled call of a one-reactor ensemble,
    recorded every step, follows the reference's trajectory; the per-step loop takes scipy's decisions on every step."""
    g = golden_npz(f"g13_forced_n{n}.npz")
    cols = cfg_columns(g["cfg"], g["cfg_fields"])
    S = np.ascontiguousarray(g["schedule"][:, :, None])
    K, dt = S.shape[0], float(g["dt"])
    traj, stats = g["traj"], g["stats"]
    ens = wt.ReactorEnsemble(cols, n_zones=n)
    ens.record(every=1, capacity=K)
    ens.step(dt, n_steps=K, boundary_schedule=S)
    tr = ens.trajectory()
    assert len(tr) == K and not tr.status.any()
    got = np.stack([tr.pH[:, 0], tr.chlorine[:, 0], tr.temperature[:, 0]], axis=1)     # (K, 3, n)
    assert np.max(np.abs(got - traj[1:]) / np.abs(traj[1:])) < 1e-7
    assert np.all(np.abs(tr.time[:, 0] - g["time"]) < 1e-9) and np.array_equal(tr.flow_rate[:, 0], g["flow"])
    ens.close()
    ens = wt.ReactorEnsemble(cols, n_zones=n)
    for k in range(K):
        ens.set_boundary(S[k])
        es = ens.step(dt, n_steps=1)
        assert tuple(ens.solver_stats()[0][:4]) == tuple(stats[k][:4]), f"step {k}"
        assert np.array_equal(es.pH[0], tr.pH[k, 0]) and np.array_equal(es.temperature[0], tr.temperature[k, 0])
        assert relerr(np.stack([es.H_concentration[0], es.density[0], es.chlorine_decay_rate[0]]), g["derived"][k]) < TOL
    ens.close()


@pytest.mark.parametrize("n,N", [(8, 10000), (20, 10000)])
def test_full_size_scheduled_vs_oracle(gpu, wt, oracle, n, N):
    """8 steps under a schedule that changes every step, against oracle.ensemble_step applied row by row, with the
    tolerances of test_full_size_ensemble_vs_oracle."""
    cols, bc = wt.make_ensemble(N)
    K = 8
    S = wt.make_boundary_schedule(bc, K, seed=8)
    ens = wt.ReactorEnsemble(cols, n_zones=n)
    st0 = ens.state
    es = ens.step(1.0, n_steps=K, boundary_schedule=S)
    pH, Cl, T, t = st0.pH, st0.chlorine, st0.temperature, st0.time
    ost = np.zeros(N, dtype=np.int64)
    for k in range(K):
        pH, Cl, T, t, s = oracle.ensemble_step(n, ens.constants, S[k], 1.0, 1, pH, Cl, T, t, nthreads=16)
        ost |= s
    assert np.array_equal(es.status != 0, ost != 0)
    ok = ost == 0
    err = np.stack([np.abs(es.pH - pH) / np.abs(pH), np.abs(es.chlorine - Cl) / np.abs(Cl),
                    np.abs(es.temperature - T) / np.abs(T)])[:, ok]
    assert np.mean(err < TOL) > 1 - 1e-5
    assert err.max() < 1e-5
    assert np.mean(err < 1e-9) > 0.999
    assert np.allclose(es.time[ok], K * 1.0)
    assert np.array_equal(es.flow_rate[ok], (S[-1, 0] + S[-1, 4] + S[-1, 6])[ok])
    ens.close()


def _snapshot(es):
    return (es.pH, es.chlorine, es.temperature, es.time, es.flow_rate, es.status)


def _record(tr, i):
    return (tr.pH[i], tr.chlorine[i], tr.temperature[i], tr.time[i], tr.flow_rate[i], tr.status[i])


@pytest.mark.parametrize("n,N", [(8, 1000), (40, 200)])
def test_records_equal_the_per_step_snapshots(gpu, wt, n, N):
    """every = 1 and 3 over two calls (a scheduled one, then a plain one), a capacity that fills up, and a restart.
    n = 40 covers the kernel that records at launch boundaries (one outer step per launch)."""
    cols, bc = wt.make_ensemble(N, seed=31)
    S = wt.make_boundary_schedule(bc, 7, seed=2)
    S_all = np.concatenate([S, np.repeat(S[-1:], 5 + 4, axis=0)])      # the plain calls keep the last row
    ens, snaps = _loop(wt, cols, n, S_all)
    ens.close()
    for every, cap in ((1, 100), (3, 100), (1, 4), (2, 3)):
        ens = wt.ReactorEnsemble(cols, n_zones=n)
        ens.record(every=every, capacity=cap)
        ens.step(1.0, n_steps=7, boundary_schedule=S)
        ens.step(1.0, n_steps=5)
        tr = ens.trajectory()
        want = [k for k in range(12) if (k + 1) % every == 0][:cap]
        assert len(tr) == len(want) == min(cap, 12 // every), (every, cap)
        for i, k in enumerate(want):
            _assert_equal(_snapshot(snaps[k]), _record(tr, i), (every, cap, k))
        # recording again restarts the count (and drops the old records)
        ens.record(every=2, capacity=cap)
        assert len(ens.trajectory()) == 0
        ens.step(1.0, n_steps=4)
        tr = ens.trajectory()
        assert len(tr) == min(2, cap)
        for i in range(len(tr)):
            _assert_equal(_snapshot(snaps[12 + 2 * i + 1]), _record(tr, i), ("restart", every, cap, i))
        ens.record(capacity=0)                                  # off: the buffers are gone
        with pytest.raises(gpu.WtError):
            ens.trajectory()
        ens.close()


def test_records_of_a_frozen_reactor(gpu, wt):
    """The cold-run reactor of test_cold_run_freezes_like_reference raises at a known step: from there on its records
    hold the frozen state and time with the T_RANGE flag, while its neighbour keeps stepping."""
    g = golden_json("g4_faults.json")["cold_run"]
    cfg = wt.ReactorConfiguration(**g["config"])
    b = wt.BoundaryConditions(**dict(zip(wt.params.BOUNDARY_FIELDS, g["bc"])))
    k0 = g["raise_step_index"]
    K = 60
    ens = wt.ReactorEnsemble([cfg, wt.ReactorConfiguration(n_zones=4)])
    S = np.repeat(wt.boundary_block([b, wt.BoundaryConditions()], 2)[None], K, axis=0)
    ens.record(every=1, capacity=K)
    es = ens.step(1.0, n_steps=K, boundary_schedule=S)
    tr = ens.trajectory()
    assert len(tr) == K
    assert np.array_equal(tr.time[:, 1], np.arange(1, K + 1)) and not tr.status[:, 1].any()
    assert np.array_equal(tr.time[:k0, 0], np.arange(1, k0 + 1)) and not (tr.status[:k0, 0] & 1).any()
    assert np.all(tr.time[k0:, 0] == k0) and np.all(tr.status[k0:, 0] & 1)
    for f in (tr.pH, tr.chlorine, tr.temperature):
        assert np.all(f[k0:, 0] == f[k0 - 1, 0])
    assert np.array_equal(tr.temperature[-1], es.temperature) and np.array_equal(tr.status[-1], es.status)
    ens.close()


def test_records_are_indexed_by_reactor_after_a_redeal(gpu, wt):
    """Adaptive placement re-deals the wavefront slots after WT_PLACE_MIN_STEPS steps of cost history; the records
    come back by reactor index, equal to those of the fixed placement."""
    N, n = 3000, 8
    cols, bc = wt.make_ensemble(N, seed=2024)
    S = wt.make_boundary_schedule(bc, 10, seed=4)
    def run(adaptive):
        ens = wt.ReactorEnsemble(cols, n_zones=n); ens.set_boundary(bc)
        ens.set_placement(adaptive)
        ens.step(1.0, n_steps=40)
        ens.record(every=1, capacity=10)
        ens.step(1.0, n_steps=10, boundary_schedule=S)
        tr = ens.trajectory()
        info, perm = ens.schedule(), ens.placement()[1]
        ens.close()
        return tr, info, perm
    ref, _, perm0 = run(False)
    got, info, perm1 = run(True)
    assert np.array_equal(perm0, np.arange(N))
    assert info["redeals"] >= 1 and not np.array_equal(perm1, np.arange(N))
    assert len(got) == len(ref) == 10
    for i in range(10):
        _assert_equal(_record(ref, i), _record(got, i), i)


def test_schedule_with_the_sensor_suite(gpu, wt):
    """Sensors on under a schedule: the history equals that of the host loop bit for bit, and the sensors -- the flow
    meter above all -- read what the sensor oracle reads when it is fed the scheduled flows and the per-step states."""
    import sensor_oracle as SO
    N, n, K = 500, 8, 24
    cols, bc = wt.make_ensemble(N, seed=12)
    S = wt.make_boundary_schedule(bc, K, seed=6)
    ens, snaps = _loop(wt, cols, n, S, setup=lambda e: e.enable_sensors(seed=9, history=K))
    ref = ens.sensor_history()
    ens.close()
    ens = wt.ReactorEnsemble(cols, n_zones=n)
    ens.enable_sensors(seed=9, history=K)
    ens.step(1.0, n_steps=K, boundary_schedule=S)
    got = ens.sensor_history()
    _assert_equal(ref, got, "sensor history")
    assert np.all(got[3] == K)
    flow = S[:, 0] + S[:, 4] + S[:, 6]                       # (K, N) total flow of each step
    f32 = lambda x: float(np.float32(x))                      # the device taps are fp32
    for r in range(4):
        assert np.array_equal([es.flow_rate[r] for es in snaps], flow[:, r])
        suite = SO.SensorSuite(cols["flow_rate"][r], cols["initial_chlorine"][r], cols["temperature"][r], 0.0, 9, r)
        ov = np.empty((K, 7)); os_ = np.empty((K, 7), dtype=np.uint8)
        for k, es in enumerate(snaps):
            v, st, _ = suite.read_all({0: f32(es.pH[r, 0]), -1: f32(es.pH[r, -1])},
                                      {0: f32(es.chlorine[r, 0]), -1: f32(es.chlorine[r, -1])},
                                      {0: f32(es.temperature[r, 0]), -1: f32(es.temperature[r, -1])},
                                      f32(flow[k, r]), float(es.time[r]))
            ov[k], os_[k] = v, st
        hv = got[0][:, :, r]
        assert np.array_equal(np.isnan(hv), np.isnan(ov))
        ok = ~np.isnan(ov)
        assert ok[:, 4].sum() >= K - 11                       # the flow meter reads after its 10 s warm-up
        assert np.max(np.abs(hv[ok] - ov[ok]) / (1.0 + np.abs(ov[ok]))) < 2e-5
        assert np.array_equal(got[1][:, :, r], os_)
    ens.close()


def test_schedule_and_record_argument_errors(gpu, wt):
    N, n = 4, 8
    cols, bc = wt.make_ensemble(N)
    S = wt.make_boundary_schedule(bc, 3, seed=1)
    ens = wt.ReactorEnsemble(cols, n_zones=n)
    with pytest.raises(ValueError, match="shape"):
        ens.step(1.0, n_steps=3, boundary_schedule=S[:, :, :2])
    with pytest.raises(ValueError, match="rows for n_steps"):
        ens.step(1.0, n_steps=2, boundary_schedule=S)
    with pytest.raises(ValueError, match="not both"):
        ens.step(1.0, bc, n_steps=3, boundary_schedule=S)
    with pytest.raises(ValueError):
        ens.record(every=0, capacity=4)
    with pytest.raises(ValueError):
        ens.record(every=1, capacity=-1)
    with pytest.raises(gpu.WtError):
        ens.trajectory()                                       # recording was never switched on
    t0 = ens.state.time.copy()
    ens.step(1.0, n_steps=3, boundary_schedule=S)
    assert np.array_equal(ens.state.time, t0 + 3) and np.array_equal(ens.boundary(), S[-1])
    ens.enable_sensors(seed=1); ens.enable_plant_io()
    with pytest.raises(ValueError, match="plant I/O"):
        ens.step(1.0, n_steps=3, boundary_schedule=S)
    assert np.array_equal(ens.state.time, t0 + 3)             # refused before anything ran
    ens.close()
