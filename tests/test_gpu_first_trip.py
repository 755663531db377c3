"""The first Newton iteration of a fresh solver runs in the trip that probes the step size: the
probe's epilogue starts the first attempt with f(y0) as the three stage values, and the Jacobian, the factorisation
and Newton iteration 1 follow in that same trip.  Checked here: reactors that start an outer step a trip apart in one
wavefront, every step-kernel instantiation against the CPU oracle with solver counters, the re-attempt after a failed
first attempt, and the attempt count of a first attempt that never passes the guard at the loop top."""
import numpy as np
import pytest

from conftest import cfg_columns, golden_json, golden_npz
from program_helpers import both_packings, packing  # noqa: F401  (a fixture: every multi-reactor test runs spread and packed)

pytestmark = pytest.mark.gpu

ST_STEP_LIMIT = 128
CLAMP_CASES = ("clamp_cl", "clamp_ph_hi", "clamp_ph_lo")


def _oracle_stats(oracle, n, par, bc, dt, y, t):
    """One outer step of one reactor on the CPU: (y, t, status, [nfev, njev, nlu, nsteps, nrej])."""
    y, t, _, status, st = oracle.step(n, par, bc, dt, y, t, want_stats=True)
    return y, t, status, np.array([st.nfev, st.njev, st.nlu, st.nsteps, st.nrej], dtype=np.int32)


def _result(ens, es):
    return (es.pH, es.chlorine, es.temperature, es.time, es.status, es.H_concentration, es.density,
            es.chlorine_decay_rate, ens.solver_stats())


def _mixed_group(wt, n, R):
    """R reactors of n zones: the three clamp cases of g11 (their parameters, boundary and pre-step state, the two
    out-of-range inlet-side zones kept, the others at the fixture's in-range value) in slots 1, 3 and R - 2, ordinary
    reactors of make_ensemble elsewhere."""
    g = golden_npz("g11_branches.npz")
    cols, bc = wt.make_ensemble(R, seed=97)
    defaults = wt.ReactorConfiguration()
    full = {}
    for k in cfg_columns(g["clamp_cl__cfg"], g["cfg_fields"]):
        v = cols.get(k, np.asarray([getattr(defaults, k)]))
        full[k] = np.broadcast_to(v, (R,)).copy()
    bc = np.array(bc, dtype=np.float64, copy=True)
    pH = np.repeat(full["initial_pH"][:, None], n, 1)
    Cl = np.repeat(full["initial_chlorine"][:, None], n, 1)
    T = np.repeat(full["temperature"][:, None], n, 1)
    for slot, name in zip((1, 3, R - 2), CLAMP_CASES):
        c = cfg_columns(g[f"{name}__cfg"], g["cfg_fields"])
        for k in full:
            full[k][slot] = c[k][0]
        bc[:, slot] = g[f"{name}__bc"]
        pre = g[f"{name}__pre"][0]                     # (3, 4): zones 0 and 1 carry the out-of-range values
        for arr, row in ((pH, pre[0]), (Cl, pre[1]), (T, pre[2])):
            arr[slot, :] = row[3]
            arr[slot, :2] = row[:2]
    return full, np.ascontiguousarray(bc), pH, Cl, T


@pytest.mark.parametrize("limit", [0, 2])
@both_packings("n,R", [(8, 8), (5, 12)])
def test_mixed_starts_in_one_wavefront(gpu, wt, packing, n, R, limit):
    """Packed, one wavefront-group (spread, R wavefronts of one reactor each: the same comparison without neighbours,
    kept as it was) whose reactors start their outer steps a trip apart: a reactor that was clamped (the g11
    clamp cases clamp on the first step they take, status asserted) has no carried f(y0) on the step after and passes
    through PH_OUTER_BEGIN, so its probe -- and with it the joined first Newton iteration -- comes one trip after its
    neighbours'.  With an attempt limit of 2 the same happens after every outer step a reactor fails, which for the
    ordinary reactors is most steps.  12 steps in one call; every reactor equals, bit for bit, the same reactor
    stepped in an ensemble of its own."""
    steps = 12
    cols, bc, pH, Cl, T = _mixed_group(wt, n, R)
    ens = wt.ReactorEnsemble(cols, n_zones=n)
    assert ens.n_reactors == R and R == 64 // n
    ens.set_boundary(bc)
    ens.set_state(pH, Cl, T, np.zeros(R))
    ens.set_step_limit(limit)
    packing.place(ens)
    got = _result(ens, ens.step(1.0, n_steps=steps))
    packing.check(ens)
    ens.close()
    clamp_bits = {1: 8, 3: 4, R - 2: 4}               # ST_CLAMP_CL, ST_CLAMP_PH
    for slot, bit in clamp_bits.items():
        assert got[4][slot] & bit, (slot, got[4][slot])
    if limit:
        assert np.count_nonzero(got[4] & ST_STEP_LIMIT) >= 2          # some reactors did fail steps, not all need to
    else:
        assert not np.any(got[4] & ST_STEP_LIMIT)
    for r in range(R):
        one = wt.ReactorEnsemble({k: v[r:r + 1] for k, v in cols.items()}, n_zones=n)
        one.set_boundary(np.ascontiguousarray(bc[:, r:r + 1]))
        one.set_state(pH[r:r + 1], Cl[r:r + 1], T[r:r + 1], np.zeros(1))
        one.set_step_limit(limit)
        alone = _result(one, one.step(1.0, n_steps=steps))
        one.close()
        for a, b in zip(got, alone):
            assert np.array_equal(a[r:r + 1], b, equal_nan=True), (r, a[r], b[0])


_ORACLE = {}                # zone count -> the oracle's state after 6 steps and its counters of every step


@both_packings("n", [2, 4, 5, 8, 12, 16, 20, 40])
def test_every_instantiation_vs_oracle_with_counters(gpu, wt, oracle, packing, n):
    """Two wavefront-groups' worth of reactors and one more at every instantiation of the step kernel -- packed, two
    full wavefronts and a partial one; spread, a wavefront per reactor -- 6 steps: state against the
    oracle's ensemble_step within the bounds of test_full_size_ensemble_vs_oracle (1e-6 on all but 1e-5 of the samples,
    1e-5 on every one), solver counters of every outer step exactly (nfev and the attempt count of the joined trip).
    The counters come from the oracle's single-reactor step chained over the same states (computed once per zone
    count, for both packings); the GPU's per step from a second ensemble stepped one call at a time, which must leave
    the bits of the one-call run."""
    N, steps = 2 * (64 // n) + 1, 6
    cols, bc = wt.make_ensemble(N)
    ens = packing.place(wt.ReactorEnsemble(cols, n_zones=n))
    ens.set_boundary(bc)
    s0 = ens.state
    es = ens.step(1.0, n_steps=steps)
    last = ens.solver_stats()
    if n not in _ORACLE:
        out = tuple(oracle.ensemble_step(n, ens.constants, bc, 1.0, steps, s0.pH, s0.chlorine, s0.temperature, s0.time,
                                         nthreads=4))
        # the oracle's counters, step by step
        ref = np.zeros((steps, N, 5), dtype=np.int32)
        for r in range(N):
            y, tt = np.concatenate([s0.pH[r], s0.chlorine[r], s0.temperature[r]]), float(s0.time[r])
            for k in range(steps):
                y, tt, status, ref[k, r] = _oracle_stats(oracle, n, ens.constants[:, r], bc[:, r], 1.0, y, tt)
                assert status == 0
        for a in out + (ref,):
            a.setflags(write=False)
        _ORACLE[n] = out + (ref,)
    pH, Cl, T, t, ost, ref = _ORACLE[n]
    assert not es.status.any() and not ost.any()
    err = np.stack([np.abs(es.pH - pH) / np.abs(pH), np.abs(es.chlorine - Cl) / np.abs(Cl),
                    np.abs(es.temperature - T) / np.abs(T)])
    print(f"n={n}: max rel err vs oracle {err.max():.3e}")
    assert np.mean(err < 1e-6) > 1 - 1e-5
    assert err.max() < 1e-5
    assert np.array_equal(es.time, t)
    ens.set_state(s0.pH, s0.chlorine, s0.temperature, s0.time)
    for k in range(steps):
        es1 = ens.step(1.0, n_steps=1)
        assert np.array_equal(ens.solver_stats(), ref[k]), (n, k)
    assert np.array_equal(last, ref[steps - 1])
    for a, b in ((es.pH, es1.pH), (es.chlorine, es1.chlorine), (es.temperature, es1.temperature), (es.time, es1.time)):
        assert np.array_equal(a, b)
    packing.check(ens)
    ens.close()


@pytest.mark.parametrize("name", ["clamp_ph_lo", "host_edit"])
def test_first_attempt_failures_keep_the_fixture_counters(gpu, wt, oracle, name):
    """g11 fixtures with a failing first attempt: every outer step from the reference's own pre-step state, scipy's
    counters per step.  Which steps fail their first attempt is found on the CPU (the oracle under an attempt limit of
    one accepts nothing in such a step); a re-attempt without dense output still has to evaluate its stage points, or
    nfev would fall short of the fixture's."""
    from test_oracle_golden import branch_case
    c = branch_case(wt, name)
    n, K = c["n"], c["pre"].shape[0]
    first_fails = []
    oracle.set_step_limit(1)
    try:
        for k in range(K):
            _, _, _, st = _oracle_stats(oracle, n, c["par"], c["bc"], c["dt"], c["pre"][k].reshape(-1), float(c["pre_time"][k]))
            if st[3] == 0:
                first_fails.append(k)
    finally:
        oracle.set_step_limit(0)
    if name == "host_edit":
        assert first_fails, "the fixture no longer has a step whose first attempt fails"
    ens = wt.ReactorEnsemble(c["cols"], n_zones=n)
    ens.set_boundary(np.ascontiguousarray(c["bc"][:, None]))
    for k in range(K):
        ens.set_state(c["pre"][k][0][None], c["pre"][k][1][None], c["pre"][k][2][None], c["pre_time"][k:k + 1])
        ens.clear_status()
        es = ens.step(c["dt"], n_steps=1)
        got = np.stack([es.pH[0], es.chlorine[0], es.temperature[0]])
        post = c["traj"][k + 1]
        tol = 1e-7 if (name == "clamp_ph_lo" and k == 0) else 1e-9     # the bounds of test_branch_fixtures_vs_reference
        assert np.all(np.abs(got - post) <= tol * np.abs(post) + 1e-300), (name, k)
        assert tuple(ens.solver_stats()[0][:4]) == tuple(c["stats"][k][:4]), (name, k, k in first_fails)
        assert es.time[0] == c["time"][k]
    ens.close()


@both_packings("limit", [1, 2])
def test_step_limit_counts_the_joined_first_attempt(gpu, wt, oracle, packing, limit):
    """16 reactors of 4 zones (packed, one full wavefront, where a flagged reactor waits beside neighbours still at
    work; spread, sixteen wavefronts), 3 outer steps, one call each so that every step's counters and flags can be read.  A
    reactor whose outer step needs more attempts than the limit (the oracle's nsteps + nrej of that step, unlimited,
    from the state the GPU step starts from) ends it flagged STEP_LIMIT with exactly `limit` attempts made; the others
    are not flagged and keep the oracle's counters.  The first attempt is started by the probe's epilogue and never
    sees the guard at the loop top, so this is where a miscount would show."""
    n, N = 4, 16
    cols, bc = wt.make_ensemble(N)
    ens = packing.place(wt.ReactorEnsemble(cols, n_zones=n))
    ens.set_boundary(bc)
    ens.set_step_limit(limit)
    flagged_total = 0
    for k in range(3):
        s = ens.state
        need = np.zeros((N, 5), dtype=np.int32)
        for r in range(N):
            y = np.concatenate([s.pH[r], s.chlorine[r], s.temperature[r]])
            _, _, status, need[r] = _oracle_stats(oracle, n, ens.constants[:, r], bc[:, r], 1.0, y, float(s.time[r]))
            assert status == 0
        ens.clear_status()
        es = ens.step(1.0, n_steps=1)
        stats = ens.solver_stats()
        flagged = (es.status & ST_STEP_LIMIT) != 0
        over = (need[:, 3] + need[:, 4]) > limit
        assert np.array_equal(flagged, over), (k, need[:, 3] + need[:, 4], es.status)
        assert np.all(stats[flagged, 3] + stats[flagged, 4] == limit), (k, stats[flagged])
        assert np.array_equal(stats[~flagged], need[~flagged]), k
        assert np.all(es.status[~flagged] == 0)
        flagged_total += int(flagged.sum())
    assert flagged_total > 0
    packing.check(ens)
    ens.close()
