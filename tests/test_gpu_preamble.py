"""The fresh solver's preamble ahead of the trip loop: the first half of select_initial_step, the
probe f(y0 + h0 f0) and the probe's epilogue run once per outer step behind f(y0), the lanes enter the loop in PH_NEWTON
with their stage values preset, and the loop's single-point site serves PH_ERR_REFINE and PH_FNEW alone.  None of it may
move a bit or a counter.  Every test runs at every instantiation of the step kernel, on three wavefront-groups' worth of
synthetic reactors less a few, once spread and once packed (the ``packing`` fixture).  Packed (WT_FULL_WAVES, identity
placement, group count asserted) these are two full wavefronts and a partly filled one, so absent segments sit beside
live ones and lanes in different phases share a wavefront; spread, the library deals an ensemble this small one reactor
to a wavefront on an MI355X and no reactor has a neighbour."""
import numpy as np
import pytest

from program_helpers import both_packings, packing  # noqa: F401  (a fixture: every multi-reactor test runs spread and packed)
from test_gpu_pending_f import ST_T_RANGE, _assert_same, _fields, _rare_group

pytestmark = pytest.mark.gpu

NS = [2, 4, 5, 8, 12, 16, 20, 40]
K = 12


def _population(n):
    """Three wavefront-groups' worth of reactors, the last group partly filled (a group holds 64 // n reactors)."""
    R = 64 // n
    return 3 * R - max(1, R // 3) if R > 1 else 3


def _run(wt, n, cols, bc, how, steps=K, state=None, identity=False, dt=1.0, packing=None):
    """`packing`: the fixture's, for a run that is to have it (asserted after the last step); None for a reactor run
    alone."""
    ens = wt.ReactorEnsemble(cols, n_zones=n)
    if packing is not None:
        packing.place(ens)
    ens.set_boundary(bc)
    if state is not None:
        ens.set_state(*state)
    if identity:
        ens.set_placement(False)
    if how == "one-step calls":
        for _ in range(steps):
            ens.step(dt, n_steps=1, download=False)
    else:
        if how == "stream":
            ens.set_schedule(1, 5)
        ens.step(dt, n_steps=steps, download=False)
    f = _fields(ens)
    if packing is not None:
        packing.check(ens)
    ens.close()
    return f


# ---------------------------------------------------------------- 1. the schedule moves no bit
@both_packings("n", NS)
def test_results_do_not_depend_on_the_schedule(gpu, wt, packing, n):
    """12 one-step calls (every step begins with f(y0) from memory), one 12-step call (f carried where a step ended in
    PH_FNEW, evaluated ahead of the loop elsewhere) and the stream schedule with launches of 5 steps: state with the
    derived arrays, status and the per-reactor solver counters, bit for bit."""
    N = _population(n)
    cols, bc = wt.make_ensemble(N)
    got = {how: _run(wt, n, cols, bc, how, packing=packing) for how in ("one call", "one-step calls", "stream")}
    assert not got["one call"]["status"].any() and np.all(got["one call"]["time"] == K)
    _assert_same(got["one call"], got["one-step calls"], "one call / one-step calls")
    _assert_same(got["one call"], got["stream"], "one call / stream schedule")


# ---------------------------------------------------------------- 2. and 3. counters against the oracle; carried f
_ORACLE = {}


def _oracle_counters(wt, oracle, n, start=0, dt=1.0):
    """(K, N, 5) nfev, njev, nlu, nsteps, nrej of K outer steps on the CPU, the oracle's single-reactor step chained over
    its own states, for reactors start ... start + N of the synthetic population; computed once per zone count and
    window, shared by the tests below and left unchanged."""
    if (n, start, dt) not in _ORACLE:
        N = _population(n)
        cols, bc = wt.make_ensemble(N, start=start)
        ens = wt.ReactorEnsemble(cols, n_zones=n)
        ens.set_boundary(bc)
        par, s0 = ens.constants, ens.state
        ens.close()
        ref = np.zeros((K, N, 5), dtype=np.int32)
        for r in range(N):
            y, t = np.concatenate([s0.pH[r], s0.chlorine[r], s0.temperature[r]]), float(s0.time[r])
            for k in range(K):
                y, t, _, status, st = oracle.step(n, par[:, r], bc[:, r], dt, y, t, want_stats=True)
                assert status == 0
                ref[k, r] = (st.nfev, st.njev, st.nlu, st.nsteps, st.nrej)
        ref.setflags(write=False)
        _ORACLE[n, start, dt] = ref
    return _ORACLE[n, start, dt]


@both_packings("n", NS)
def test_counters_of_every_step_of_an_item_vs_oracle(gpu, wt, oracle, packing, n):
    """A call stores the counters of its last outer step, so step k of a 12-step item is read from an item of k steps
    from the same start.  nfev is where a miscount of the preamble would show: f(y0) (evaluated or carried), the probe
    and the three stage values that the first Newton iteration takes from f(y0) are counted ahead of the loop."""
    N = _population(n)
    cols, bc = wt.make_ensemble(N)
    ref = _oracle_counters(wt, oracle, n)
    ens = packing.place(wt.ReactorEnsemble(cols, n_zones=n))
    ens.set_boundary(bc)
    s0 = ens.state
    for k in range(1, K + 1):
        ens.set_state(s0.pH, s0.chlorine, s0.temperature, s0.time)
        es = ens.step(1.0, n_steps=k)
        assert not es.status.any()
        got = ens.solver_stats()
        assert np.array_equal(got, ref[k - 1]), (n, k, np.argwhere(got != ref[k - 1])[:4].tolist())
    packing.check(ens)
    ens.close()


@both_packings("n", NS)
def test_lanes_that_carry_f_beside_lanes_that_do_not(gpu, wt, oracle, packing, n):
    """A reactor whose outer step takes a second Jacobian (njev > 1 in the oracle's counters) went through PH_FNEW, and
    where the refresh came with the step's last accept it carries f into the next outer step while its neighbours
    evaluate theirs ahead of the loop.  Such steps are found on the CPU: the synthetic population is scanned window by
    window (three wavefront-groups' worth each, 11 steps, at most 1024 reactors) until a window holds one; about 7 % of
    the reactor-steps at n = 8 do.  Identity placement; the window in one 12-step call has the oracle's counters and
    equals, bit for bit, each such reactor run alone.  Where the scan finds none (n = 2: two zones do not refresh at
    dt = 1 s), window 0 is stepped with dt = 10, 30 or 100 s instead, the first that holds one.  (The counters cannot
    tell a refresh at a step's last accept, which carries f, from one at an earlier accept, which does not: the count
    printed is of refreshes, an upper bound of the carries.  The bitwise comparison holds either way.)"""
    N = _population(n)
    candidates = [(1.0, start) for start in range(0, 1024 - N + 1, N)] + [(10.0, 0), (30.0, 0), (100.0, 0)]
    for dt, start in candidates:
        ref = _oracle_counters(wt, oracle, n, start, dt)
        carry = np.argwhere(ref[:K - 1, :, 1] > 1)        # (step, reactor): a refresh in a step that another step follows
        lanes = np.unique(carry[:, 1])
        if len(lanes):
            break
    print(f"n={n}: dt {dt}, window at {start}: {len(carry)} outer steps with a Jacobian refresh, in {len(lanes)} of {N} reactors")
    assert len(lanes) >= 1
    cols, bc = wt.make_ensemble(N, start=start)
    got = _run(wt, n, cols, bc, "one call", identity=True, dt=dt, packing=packing)
    assert not got["status"].any()
    assert np.array_equal(got["stats"], ref[K - 1])
    for r in lanes[:8]:
        alone = _run(wt, n, {k: v[r:r + 1] for k, v in cols.items()}, np.ascontiguousarray(bc[:, r:r + 1]), "one call", dt=dt)
        for k in got:
            assert np.array_equal(got[k][r:r + 1], alone[k], equal_nan=True), (r, k, got[k][r], alone[k][0])


# ---------------------------------------------------------------- 4. raises in the preamble
_COLD_T = {}


def _cold_T_for_a_probe_raise_in_step_3(wt, oracle, n, N):
    """The start temperature of the cold reactor (all zones) from which the CPU oracle takes two outer steps and raises in
    the third at the probe point: y0 of step 3 is in range, so its f(y0) is fine, and the coldest zone -- cooling at
    about 0.015 K/s -- is closer to the range's end than h0 |f0|, so y0 + h0 f0 is the first point outside.  Bisection
    on the start temperature: too cold where one of the first two steps raises, too warm where step 3 gets as far as an
    attempt; found where step 3 raises with nfev = 2 (f(y0), the probe), no Jacobian and no step."""
    if n not in _COLD_T:
        cols, bc, pH, Cl, T, slots = _rare_group(wt, n, N, cold_T=1.0)
        s = slots["cold_run"]
        ens = wt.ReactorEnsemble(cols, n_zones=n)
        par = ens.constants[:, s].copy()
        ens.close()

        def verdict(c):
            y, t = np.concatenate([pH[s], Cl[s], np.full(n, c)]), 0.0
            for _ in range(2):
                y, t, _, status, st = oracle.step(n, par, bc[:, s], 1.0, y, t, want_stats=True)
                if status:
                    return -1
            if np.min(y[2 * n:]) < 0.0:
                return -1
            _, _, _, status, st = oracle.step(n, par, bc[:, s], 1.0, y, t, want_stats=True)
            if status & ST_T_RANGE and (st.nfev, st.njev, st.nsteps) == (2, 0, 0):
                return 0
            return 1

        lo, hi, found = 0.0, 1.0, None
        for _ in range(200):
            c = 0.5 * (lo + hi)
            v = verdict(c)
            if v == 0:
                found = c
                break
            if v < 0:
                lo = c
            else:
                hi = c
        assert found is not None, (n, lo, hi)
        _COLD_T[n] = found
    return _COLD_T[n]


@pytest.mark.parametrize("where", ["f(y0)", "probe", "probe in step 3", "inside the item"])
@both_packings("n", NS)
def test_raises_in_the_preamble(gpu, wt, oracle, packing, n, where):
    """g4's cold run (a reactor that loses heat) beside the g11 clamp cases and ordinary reactors, a 6-step item against
    one-step calls: status bits, the frozen state, the temperature the message names and the untouched neighbours, bit
    for bit.  `f(y0)`: a zone below 0 degC when the item begins, so the evaluation ahead of the loop raises (stage 1)
    and the state stays.  `probe`: every zone at 1e-10 degC, inside the range, and f0 < 0 there, so y0 + h0 f0 is the
    first point outside it: the lane ends before any attempt, with nfev = 2.  `inside the item`: the reactor starts
    0.02 K above the range's end and leaves it in a later step of the item (which one is read from the one-step
    calls and must be neither the first nor the last).  `probe in step 3`: the start temperature comes from the CPU oracle
    (bisection, see the helper) so that after two steps the coldest zone is in range by less than h0 |f0|: step 3 of the
    item evaluates f(y0) ahead of the loop beside lanes that carry theirs, its probe point is the first outside the
    range, and the lane ends with the counters of a step that attempted nothing (nfev = 2: f(y0) and the probe), the
    state of step 2 and time = 2.  An f(y0) raise in a later step of an item cannot happen: y0 of step k + 1 is y_new of
    step k, and the accept's range test (or PH_FNEW's evaluation) raises on it first -- the `inside the item` case."""
    N = min(64, max(3 * (64 // n) - 1, 8))
    if where == "probe in step 3":
        cold_T = _cold_T_for_a_probe_raise_in_step_3(wt, oracle, n, N)
    else:
        cold_T = {"f(y0)": -0.01, "probe": 1e-10, "inside the item": 0.02}[where]
    cols, bc, pH, Cl, T, slots = _rare_group(wt, n, N, cold_T=cold_T)
    s = slots["cold_run"]
    state = (pH, Cl, T, np.zeros(N))
    steps = 6
    one = _run(wt, n, cols, bc, "one call", steps=steps, state=state, packing=packing)
    # one-step calls, reading which call raised and what it named (later calls leave a frozen reactor alone)
    ens = packing.place(wt.ReactorEnsemble(cols, n_zones=n))
    ens.set_boundary(bc)
    ens.set_state(*state)
    raised_at, named, stats_at = None, None, None
    for k in range(steps):
        ens.step(1.0, n_steps=1, download=False)
        if raised_at is None and ens.status()[s] & ST_T_RANGE:
            raised_at, named, stats_at = k, ens.bad_temperature()[s], ens.solver_stats()[s].copy()
    ref = _fields(ens)
    packing.check(ens)
    ens.close()
    assert raised_at is not None
    ref["bad_T"][s] = named
    assert one["status"][s] & ST_T_RANGE and one["time"][s] == raised_at
    if where == "inside the item":
        assert 1 <= raised_at <= steps - 2, raised_at
    elif where == "probe in step 3":
        assert raised_at == 2 and one["time"][s] == 2
        assert -1e-3 < one["bad_T"][s] < 0.0 and np.all(one["temperature"][s] >= 0.0)
        assert tuple(one["stats"][s]) == (2, 0, 0, 0, 0), one["stats"][s]      # f(y0), the probe, and no attempt
    else:
        assert raised_at == 0
        assert np.array_equal(one["temperature"][s], T[s]) and np.array_equal(one["pH"][s], pH[s])   # the state stayed
    if where == "f(y0)":
        assert one["bad_T"][s] == cold_T
    if where == "probe":
        assert -1e-3 < one["bad_T"][s] < 0.0
    ordinary = np.setdiff1d(np.arange(N), list(slots.values()))
    assert not one["status"][ordinary].any() and np.all(one["time"][ordinary] == steps)
    # (the counters of the step that raised are stored only by a call in which the reactor also took a step)
    live = np.arange(N) != s
    assert np.array_equal(one["stats"][live], ref["stats"][live])
    del one["stats"], ref["stats"]
    _assert_same(one, ref, "one call / one-step calls")


# ---------------------------------------------------------------- 5. a boundary reload after every step
@both_packings("n", NS)
def test_boundary_reload_after_every_step(gpu, wt, packing, n):
    """Plant I/O with a scan per step over 8 steps: every scan reloads the boundary, so no step carries f and every
    preamble begins with its own f(y0).  One call against one-step calls, bit for bit, readings and image included."""
    N, steps = _population(n), 8
    cols, bc = wt.make_ensemble(N)
    got = {}
    for how in ("one call", "one-step calls"):
        ens = packing.place(wt.ReactorEnsemble(cols, n_zones=n))
        ens.set_boundary(bc)
        ens.enable_sensors(seed=11)
        ens.enable_plant_io()
        ens.write_commands(0.4, 0.2, 5.5)
        if how == "one call":
            ens.set_schedule(0, 1)
            ens.step(1.0, n_steps=steps, download=False)
        else:
            for _ in range(steps):
                ens.step(1.0, n_steps=1, download=False)
        f = _fields(ens)
        f.update({f"reading{i}": a for i, a in enumerate(ens.sensor_readings())})
        f.update({f"image{i}": a for i, a in enumerate(ens.input_image())})
        got[how] = f
        packing.check(ens)
        ens.close()
    assert np.all(got["one call"]["time"] == steps)
    _assert_same(got["one call"], got["one-step calls"], "one call / one-step calls")


# ---------------------------------------------------------------- 6. the rare phases' single-point site
def test_rejections_and_refinements_keep_the_fixture_counters(gpu, wt):
    """The g11 `clamp_ph_lo` case from the reference's own pre-step state: 80 internal steps through pH 0..2 with
    rejected steps and second error estimates (PH_ERR_REFINE) and Jacobian refreshes (PH_FNEW), both through the loop's
    remaining single-point site.  Counters are scipy's, the state within the bound of test_branch_fixtures_vs_reference,
    as test_first_attempt_failures_keep_the_fixture_counters holds them."""
    from test_oracle_golden import branch_case
    c = branch_case(wt, "clamp_ph_lo")
    n, steps = c["n"], c["pre"].shape[0]
    ens = wt.ReactorEnsemble(c["cols"], n_zones=n)
    ens.set_boundary(np.ascontiguousarray(c["bc"][:, None]))
    for k in range(steps):
        ens.set_state(c["pre"][k][0][None], c["pre"][k][1][None], c["pre"][k][2][None], c["pre_time"][k:k + 1])
        ens.clear_status()
        es = ens.step(c["dt"], n_steps=1)
        got = np.stack([es.pH[0], es.chlorine[0], es.temperature[0]])
        post = c["traj"][k + 1]
        tol = 1e-7 if k == 0 else 1e-9
        assert np.all(np.abs(got - post) <= tol * np.abs(post) + 1e-300), k
        st = ens.solver_stats()[0]
        assert tuple(st[:4]) == tuple(c["stats"][k][:4]), (k, st, c["stats"][k])
        if k == 0:
            assert st[4] > 0, "the fixture's first step no longer rejects a step"     # (the fixture records no nrej)
    ens.close()
