"""Where a pending f is evaluated: an outer step ends in the trip that accepts its last internal
step, the next one evaluates f(y0) ahead of its first trip, the pending f(y_new) of a non-final step is the fourth point
of the next stage block, and the derived state is formed once per item.  None of it may move a bit or a counter, at any
item length and at any instantiation of the step kernel.  Checked here: one call against one-step calls and a chunked
stream schedule, the counters of every step of an item against the CPU oracle, clamps and a raise inside an item
(g11 / g4 fixtures), a boundary reload after every step, and reactors that lag their wavefront.

Every test runs twice (the ``packing`` fixture).  Spread is the library's own dealing of an ensemble this small, one
reactor per wavefront on an MI355X: nobody has a neighbour, and what the docstrings say about wavefronts with ordinary
reactors in them holds for the packed run alone, where WT_FULL_WAVES puts 64 // n reactors into every wavefront under
the identity placement and the group count is asserted."""
import numpy as np
import pytest

from conftest import cfg_columns, golden_json, golden_npz
from program_helpers import both_packings, packing  # noqa: F401  (a fixture: every test runs spread and packed)

pytestmark = pytest.mark.gpu

NS = [2, 4, 5, 8, 16, 20, 40]                          # one zone count per instantiation of the step kernel
ST_T_RANGE, ST_CLAMP_PH, ST_CLAMP_CL, ST_T_RANGE_POST, ST_STEP_LIMIT = 1, 4, 8, 32, 128
CLAMP_CASES = {"clamp_cl": ST_CLAMP_CL, "clamp_ph_hi": ST_CLAMP_PH, "clamp_ph_lo": ST_CLAMP_PH}
STATE_FIELDS = ("pH", "chlorine", "temperature", "time", "flow_rate", "H_concentration", "density",
                "chlorine_decay_rate", "status")


def _fields(ens):
    """Everything a call leaves behind: the nine arrays of the state, the last step's counters, the named temperature
    (defined only where a range bit is set)."""
    s = ens.state
    bad = np.where(s.status & (ST_T_RANGE | ST_T_RANGE_POST), ens.bad_temperature(), 0.0)
    return {**{k: getattr(s, k) for k in STATE_FIELDS}, "stats": ens.solver_stats(), "bad_T": bad}


def _assert_same(a, b, what):
    for k in a:
        assert np.array_equal(a[k], b[k], equal_nan=True), (what, k, np.argwhere(a[k] != b[k])[:4].tolist())


def _group_size(n, floor=8):
    """Reactors of a test: two wavefront-groups' worth, at least `floor` (a packed group holds 64 // n reactors), at
    most 64."""
    return min(64, max(2 * (64 // n), floor))


# ---------------------------------------------------------------- item length
@both_packings("n", NS)
def test_item_length_changes_no_bit(gpu, wt, packing, n):
    """The same ensemble advanced by one call of 9 steps (one item: f pending from step to step in registers, derived
    state formed once), by nine calls of one step (every step begins with f(y0) from memory, derived state stored every
    step) and by a stream schedule with launches of 2 steps: state with the derived arrays, flow and time, status and
    the last step's counters, bit for bit."""
    N, K = min(64, 2 * (64 // n) + 1), 9
    cols, bc = wt.make_ensemble(N)
    got = {}
    for how in ("one call", "one-step calls", "stream, chunk 2"):
        ens = packing.place(wt.ReactorEnsemble(cols, n_zones=n))
        ens.set_boundary(bc)
        if how == "stream, chunk 2":
            ens.set_schedule(1, 2)
        if how == "one-step calls":
            for _ in range(K):
                ens.step(1.0, n_steps=1, download=False)
        else:
            ens.step(1.0, n_steps=K, download=False)
        got[how] = _fields(ens)
        packing.check(ens)
        ens.close()
    assert not got["one call"]["status"].any()
    assert np.all(got["one call"]["time"] == K)
    _assert_same(got["one call"], got["one-step calls"], "one call / one-step calls")
    _assert_same(got["one call"], got["stream, chunk 2"], "one call / stream schedule")


# ---------------------------------------------------------------- counters of every step of an item
_ORACLE_COUNTERS = {}


def _oracle_counters(oracle, n, par, bc, s0, K):
    """(K, N, 4) nfev, njev, nlu, nsteps of K outer steps on the CPU, the oracle's single-reactor step chained over its
    own states from s0; computed once per zone count and shared by the test cases."""
    if n not in _ORACLE_COUNTERS:
        N = par.shape[1]
        ref = np.zeros((K, N, 4), dtype=np.int32)
        for r in range(N):
            y, t = np.concatenate([s0.pH[r], s0.chlorine[r], s0.temperature[r]]), float(s0.time[r])
            for k in range(K):
                y, t, _, status, st = oracle.step(n, par[:, r], bc[:, r], 1.0, y, t, want_stats=True)
                assert status == 0
                ref[k, r] = (st.nfev, st.njev, st.nlu, st.nsteps)
        ref.setflags(write=False)
        _ORACLE_COUNTERS[n] = ref
    return _ORACLE_COUNTERS[n]


@pytest.mark.parametrize("lengths", [(1, 3, 5, 7, 9), (2, 4, 6, 8)])
@both_packings("n", NS)
def test_counters_of_every_step_of_an_item_vs_oracle(gpu, wt, oracle, packing, n, lengths):
    """A call stores the counters of its last outer step, so step k of an item is read from an item of k + 1 steps: the
    items of 1 ... 9 steps from the same start (two test cases, odd and even lengths), each against the oracle's
    single-reactor step chained over its own states.  nfev is where a miscount would show: f(y_new) of an outer step's
    last internal step is counted at the accept although nothing evaluates it there, and f(y0) of the next outer step
    where it is evaluated.  The draw holds both classes of the bench ensemble, two and three internal steps of two
    Newton iterations (16 and 23 evaluations)."""
    N, K = min(64, 2 * (64 // n) + 1), 9
    cols, bc = wt.make_ensemble(N)
    ref = None
    for k in lengths:
        ens = packing.place(wt.ReactorEnsemble(cols, n_zones=n))
        ens.set_boundary(bc)
        if ref is None:
            ref = _oracle_counters(oracle, n, ens.constants, bc, ens.state, K)
            assert (ref[..., 0] == 16).any() and (ref[..., 0] == 23).any(), np.unique(ref[..., 0])
        es = ens.step(1.0, n_steps=k)
        assert not es.status.any()
        got = ens.solver_stats()[:, :4]
        packing.check(ens)
        ens.close()
        assert np.array_equal(got, ref[k - 1]), (n, k, np.argwhere(got != ref[k - 1])[:4].tolist())


# ---------------------------------------------------------------- the rare ends of a step inside an item
def _rare_group(wt, n, N, cold_T, where=None):
    """N reactors of n zones: the three clamp cases of g11 in slots 1, 3 and N - 2 (their parameters, boundary and
    pre-step state: the two out-of-range inlet-side zones kept, the others at the fixture's in-range value), the cold
    run of g4 in slot N - 4 with every zone at cold_T, ordinary reactors of make_ensemble elsewhere.  `where`: other
    reactor indices for the four, in that order."""
    where = (1, 3, N - 2, N - 4) if where is None else tuple(where)
    assert len(set(where)) == 4 and all(0 <= w < N for w in where), where
    g = golden_npz("g11_branches.npz")
    cold = golden_json("g4_faults.json")["cold_run"]
    cols, bc = wt.make_ensemble(N, seed=97)
    defaults = wt.ReactorConfiguration()
    full = {}
    for k in cfg_columns(g["clamp_cl__cfg"], g["cfg_fields"]):
        full[k] = np.broadcast_to(cols.get(k, np.asarray([getattr(defaults, k)])), (N,)).copy()
    bc = np.array(bc, dtype=np.float64, copy=True)
    pH = np.repeat(full["initial_pH"][:, None], n, 1)
    Cl = np.repeat(full["initial_chlorine"][:, None], n, 1)
    T = np.repeat(full["temperature"][:, None], n, 1)
    slots = dict(zip(CLAMP_CASES, where[:3]))
    for name, slot in slots.items():
        c = cfg_columns(g[f"{name}__cfg"], g["cfg_fields"])
        for k in full:
            full[k][slot] = c[k][0]
        bc[:, slot] = g[f"{name}__bc"]
        pre = g[f"{name}__pre"][0]                     # (3, 4): zones 0 and 1 carry the out-of-range values
        for arr, row in ((pH, pre[0]), (Cl, pre[1]), (T, pre[2])):
            arr[slot, :] = row[3]
            arr[slot, :min(2, n)] = row[:min(2, n)]
    c = slots["cold_run"] = where[3]
    for k in full:
        if k in cold["config"]:
            full[k][c] = cold["config"][k]
    bc[:, c] = cold["bc"]
    pH[c], Cl[c], T[c] = cold["config"]["initial_pH"], cold["config"]["initial_chlorine"], cold_T
    return full, np.ascontiguousarray(bc), pH, Cl, T, slots


@both_packings("n", NS)
def test_clamps_and_a_raise_inside_an_item(gpu, wt, packing, n):
    """Reactors that clamp on the first step of a 9-step item and one that cools below 0 degC in the middle of it, in
    wavefronts with ordinary reactors: state, status, the temperature the raise names and the derived arrays equal,
    bit for bit, those of the same ensemble advanced by one-step calls -- where the derived state is formed after every
    step, a clamped step's from its pre-clamp state, and a frozen reactor's stays that of its last live step.  The
    cooling reactor starts 0.05 K above the range's end and loses about 0.015 K a step (g4's run: 0.5 K in 34 steps);
    which step raises is read from the one-step calls and must lie inside the item, live steps before it and frozen
    ones after."""
    N, K = _group_size(n), 9
    cols, bc, pH, Cl, T, slots = _rare_group(wt, n, N, cold_T=0.05)
    runs = {}
    for how in ("one call", "one-step calls"):
        ens = packing.place(wt.ReactorEnsemble(cols, n_zones=n))
        ens.set_boundary(bc)
        ens.set_state(pH, Cl, T, np.zeros(N))
        if how == "one call":
            ens.step(1.0, n_steps=K, download=False)
        else:
            first_status = None
            raised_at = None
            for k in range(K):
                ens.step(1.0, n_steps=1, download=False)
                st = ens.status()
                if k == 0:
                    first_status = st
                if raised_at is None and st[slots["cold_run"]] & ST_T_RANGE:
                    raised_at = k
                    named = ens.bad_temperature()[slots["cold_run"]]   # (the call that raised names it; later calls do not)
        runs[how] = _fields(ens)
        if how == "one-step calls":
            runs[how]["bad_T"][slots["cold_run"]] = named
        packing.check(ens)
        ens.close()
    for name, bit in CLAMP_CASES.items():
        assert first_status[slots[name]] & bit, (name, first_status[slots[name]])
    assert raised_at is not None and 1 <= raised_at <= K - 2, raised_at
    one = runs["one call"]
    assert one["status"][slots["cold_run"]] & ST_T_RANGE and one["time"][slots["cold_run"]] == raised_at
    assert one["bad_T"][slots["cold_run"]] < 0
    ordinary = np.setdiff1d(np.arange(N), list(slots.values()))
    assert not one["status"][ordinary].any() and np.all(one["time"][ordinary] == K)
    # (the counters of the step that raised are stored only by a call in which the reactor also took a step: the live ones')
    live = np.arange(N) != slots["cold_run"]
    assert np.array_equal(one["stats"][live], runs["one-step calls"]["stats"][live])
    del one["stats"], runs["one-step calls"]["stats"]
    _assert_same(one, runs["one-step calls"], "one call / one-step calls")


def test_clamp_fixtures_keep_their_counters_inside_an_item(gpu, wt, packing):
    """The g11 clamp cases from the reference's own pre-step state, in a wavefront with ordinary reactors: the items of
    1, 2 and 3 steps end on the fixture's recorded steps 0, 1 and 2.  Counters and status bits are the fixture's, the
    state within the bounds of test_branch_fixtures_vs_reference, the derived arrays within ten times those (the bound
    test_branch_fixtures_oracle_vs_reference holds the oracle to) -- step 0's are those of the pre-clamp state."""
    from test_oracle_golden import branch_case
    n, N = 4, 16
    cols, bc, pH, Cl, T, slots = _rare_group(wt, n, N, cold_T=20.0)
    for k in (1, 2, 3):
        ens = packing.place(wt.ReactorEnsemble(cols, n_zones=n))
        ens.set_boundary(bc)
        ens.set_state(pH, Cl, T, np.zeros(N))
        es = ens.step(1.0, n_steps=k)
        stats = ens.solver_stats()
        packing.check(ens)
        ens.close()
        for name, bit in CLAMP_CASES.items():
            c, s = branch_case(wt, name), slots[name]
            assert np.array_equal(c["pre"][0], np.stack([pH[s], Cl[s], T[s]]))
            assert es.status[s] == bit, (name, k, es.status[s])
            assert tuple(stats[s][:4]) == tuple(c["stats"][k - 1][:4]), (name, k, stats[s], c["stats"][k - 1])
            tol = 1e-7 if name == "clamp_ph_lo" else 1e-9     # (step 0 of clamp_ph_lo: 80 internal steps through pH 0..2)
            got = np.stack([es.pH[s], es.chlorine[s], es.temperature[s]])
            post = c["traj"][k]
            assert np.all(np.abs(got - post) <= tol * np.abs(post) + 1e-300), (name, k)
            der = np.stack([es.H_concentration[s], es.density[s], es.chlorine_decay_rate[s]])
            ref = c["derived"][k - 1]
            assert np.all(np.abs(der - ref) <= 10 * tol * np.abs(ref) + 1e-300), (name, k)
            assert es.time[s] == c["time"][k - 1]


def test_cold_run_raises_inside_an_item_like_the_reference(gpu, wt, packing):
    """g4's cold run from its initial state in a wavefront with ordinary reactors, four items of 9 steps: the reference
    raises in step 34, the eighth step of the fourth item, out of f(y_new) of an accepted step -- the raise at the
    accept where that step ends the outer step.  Status, time, the state before the raise and the named temperature
    within the bounds of test_cold_run_freezes_like_reference; the derived arrays stay those of step 33."""
    g = golden_json("g4_faults.json")["cold_run"]
    n, N = 4, 16
    cols, bc, pH, Cl, T, slots = _rare_group(wt, n, N, cold_T=g["config"]["temperature"])
    s = slots["cold_run"]
    ens = packing.place(wt.ReactorEnsemble(cols, n_zones=n))
    ens.set_boundary(bc)
    ens.set_state(pH, Cl, T, np.zeros(N))
    for _ in range(4):
        es = ens.step(1.0, n_steps=9)
    bad_T = ens.bad_temperature()[s]
    packing.check(ens)
    ens.close()
    assert g["raise_step_index"] == 34
    assert es.status[s] == ST_T_RANGE and es.time[s] == g["time_before_raise"]
    got = np.stack([es.pH[s], es.chlorine[s], es.temperature[s]])
    ref = np.array(g["state_before_raise"])
    assert np.max(np.abs(got - ref) / np.abs(ref)) < 1e-9
    assert abs(bad_T - float(g["message"].split()[1].split("°")[0])) < 1e-8
    # the derived arrays of the last live step: formed when the item ended, from the state that stayed (a few ulp of
    # the device's 10^x against numpy's)
    assert np.allclose(es.H_concentration[s], 10.0 ** -es.pH[s], rtol=1e-13, atol=0)
    ordinary = np.setdiff1d(np.arange(N), list(slots.values()))
    assert not es.status[ordinary].any() and np.all(es.time[ordinary] == 36)


# ---------------------------------------------------------------- a boundary reload after every step
@both_packings("n", NS)
def test_boundary_reload_every_step(gpu, wt, packing, n):
    """Plant I/O with a PLC scan after every outer step, 24 reactors, 8 steps: every scan reloads the boundary, so no f
    is ever carried and every step begins with its own f(y0).  One call with a scan per step against one-step calls
    (a scan per launch): state with the derived arrays, status, counters, sensor readings and register image, bit for
    bit."""
    N, K = 24, 8
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
            ens.step(1.0, n_steps=K, download=False)
        else:
            for _ in range(K):
                ens.step(1.0, n_steps=1, download=False)
        f = _fields(ens)
        f.update({f"reading{i}": a for i, a in enumerate(ens.sensor_readings())})
        f.update({f"image{i}": a for i, a in enumerate(ens.input_image())})
        f["boundary"] = ens.boundary()
        got[how] = f
        packing.check(ens)
        ens.close()
    assert np.all(got["one call"]["time"] == K)
    assert np.allclose(got["one call"]["boundary"][[4, 6, 0]], np.array([[0.4], [0.2], [5.5]]))   # the command path ran
    _assert_same(got["one call"], got["one-step calls"], "one call / one-step calls")


# ---------------------------------------------------------------- reactors that lag their wavefront
@both_packings("n", NS)
def test_lagging_reactors_in_one_wavefront(gpu, wt, packing, n):
    """Packed, one wavefront-group (spread, 64 // n wavefronts of one reactor, where nothing meets anything) under an
    attempt limit of 2: a reactor that needs a third internal step fails its outer
    step and begins the next a trip behind its neighbours, so pending points meet other reactors' stage points, and
    evaluations ahead of the first trip meet reactors that carry their f.  9 steps in one call; every reactor equals,
    bit for bit, the same reactor stepped in an ensemble of its own."""
    R, K = 64 // n, 9
    cols, bc = wt.make_ensemble(R, seed=97)
    ens = packing.place(wt.ReactorEnsemble(cols, n_zones=n))
    assert ens.n_reactors == R
    ens.set_boundary(bc)
    ens.set_step_limit(2)
    ens.step(1.0, n_steps=K, download=False)
    got = _fields(ens)
    packing.check(ens)
    ens.close()
    flagged = (got["status"] & ST_STEP_LIMIT) != 0
    if R >= 8:
        assert flagged.any() and not flagged.all(), got["status"]
    for r in range(R):
        one = wt.ReactorEnsemble({k: v[r:r + 1] for k, v in cols.items()}, n_zones=n)
        one.set_boundary(np.ascontiguousarray(bc[:, r:r + 1]))
        one.set_step_limit(2)
        one.step(1.0, n_steps=K, download=False)
        alone = _fields(one)
        one.close()
        for k in got:
            assert np.array_equal(got[k][r:r + 1], alone[k], equal_nan=True), (r, k, got[k][r], alone[k][0])
