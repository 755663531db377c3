"""Packed equals spread, bit for bit.  The library spreads an ensemble smaller than the card's
wavefront slots over more wavefronts than it needs -- one reactor each up to 4 x CUs reactors -- and packs 64 // n
reactors into every wavefront of a large one (`units_per_wavefront`, csrc/wtphys.hip: "Results do not depend on it").
So the same small population run both ways is an exact reference for the step kernel's mixed-wavefront paths, free of
solver chaos: the ballot dispatch of the trip loop, `all_held` in num_jac, the ballot retry of num_jac_species, the
wave-uniform solves of wt_pcr.hpp and the masked out-of-segment reads of the LDS exchange row.  The spread run is what
the other solver tests tie to the oracle and the reference.

Every case: N = 5 (64 // n) + 1 reactors (five full wavefront-groups and one that holds a single reactor), identity
placement, both group counts asserted through wt_ensemble_wave_diag, and everything a call leaves behind compared:
state, derived arrays, flow, time, status, the last step's counters and the named bad temperature."""
import numpy as np
import pytest

from program_helpers import assert_equal_by_reactor, assert_packing, instantiation, ragged_size, set_packing
from test_gpu_parity import _random_edge_ensemble
from test_gpu_pending_f import (CLAMP_CASES, ST_STEP_LIMIT, ST_T_RANGE, _fields, _rare_group)

PACKED_NS = (2, 3, 4, 5, 7, 8, 12, 16, 17, 20, 31, 32)     # every instantiation with n <= 32, both row modes, R = 32 ... 2
ST_NONFINITE = 64
K = 12


def test_zone_counts_reach_every_packing_instantiation():
    """The zone counts of this module reach every instantiation of the step kernel that can hold two reactors in a
    wavefront, in both row modes, and every level's largest and smallest number of reactors per wavefront."""
    sharing = {(1, True), (2, False), (2, True), (3, False), (3, True), (4, False), (4, True), (5, False)}
    assert {instantiation(n) for n in range(2, 33)} == sharing and instantiation(33) == (6, False)
    assert {instantiation(n) for n in PACKED_NS} == sharing
    assert all(64 // n >= 2 for n in PACKED_NS) and 64 // 33 == 1
    per_wave = [64 // n for n in PACKED_NS]
    assert per_wave == sorted(per_wave, reverse=True) and per_wave[0] == 32 and per_wave[-1] == 2
    assert {n for n in PACKED_NS if instantiation(n)[1]} == {2, 4, 8, 16}                 # every row-mode zone count
    assert {instantiation(n)[0] for n in PACKED_NS if 64 % n} == {2, 3, 4, 5}             # idle lanes behind the last segment
    assert ragged_size(2) == (32, 161) and ragged_size(32) == (2, 11)


def _both(wt, monkeypatch, n, cols, bc, *, steps=K, dt=1.0, state=None, limit=0, how="one call"):
    """The population run packed and spread (in that order): `_fields` of each."""
    out = {}
    for packing in ("packed", "spread"):
        set_packing(monkeypatch, packing)
        ens = wt.ReactorEnsemble(cols, n_zones=n)
        ens.set_placement(False)
        ens.set_boundary(bc)
        if state is not None:
            ens.set_state(*state)
        if limit:
            ens.set_step_limit(limit)
        if how == "stream":
            ens.set_schedule(1, 5)
        elif how == "tickets":
            ens.set_schedule(0, 5)
        ens.step(dt, n_steps=steps, download=False)
        out[packing] = _fields(ens)
        assert_packing(ens, packing)
        ens.close()
    return out["packed"], out["spread"]


def _assert_packed_equals_spread(packed, spread, what, n):
    assert list(packed) == list(spread)
    assert_equal_by_reactor([np.moveaxis(np.asarray(v), 0, -1) for v in spread.values()],
                            [np.moveaxis(np.asarray(v), 0, -1) for v in packed.values()], (what, list(packed)), 64 // n)


# ---------------------------------------------------------------- (a) benign
_ORACLE = {}


def _oracle_last_step(wt, oracle, n, N):
    """(N, 5) nfev, njev, nlu, nsteps, nrej of outer step K on the CPU: the oracle's single-reactor step chained over its
    own states; computed once per zone count."""
    if n not in _ORACLE:
        cols, bc = wt.make_ensemble(N)
        ens = wt.ReactorEnsemble(cols, n_zones=n)
        par, s0 = ens.constants, ens.state
        ens.close()
        ref = np.zeros((N, 5), dtype=np.int32)
        for r in range(N):
            y, t = np.concatenate([s0.pH[r], s0.chlorine[r], s0.temperature[r]]), float(s0.time[r])
            for k in range(K):
                y, t, _, status, st = oracle.step(n, par[:, r], bc[:, r], 1.0, y, t, want_stats=True)
                assert status == 0
            ref[r] = (st.nfev, st.njev, st.nlu, st.nsteps, st.nrej)
        ref.setflags(write=False)
        _ORACLE[n] = ref
    return _ORACLE[n]


@pytest.mark.gpu
@pytest.mark.parametrize("how", ["one call", "stream", "tickets"])
@pytest.mark.parametrize("n", PACKED_NS)
def test_benign_population(gpu, wt, oracle, monkeypatch, n, how):
    """make_ensemble, 12 steps of 1 s in one call: as one launch, as a stream schedule with launches of 5 steps, and
    through the work queue with its ticket budget turned down (WT_Q_TICKETS=1: one item per group and launch).  The
    counters of the last step are the oracle's, so both runs did the solve the CPU does; within at least one packed
    group two reactors' counters differ, so neighbours really went different ways."""
    R, N = ragged_size(n)
    cols, bc = wt.make_ensemble(N)
    if how == "tickets":
        monkeypatch.setenv("WT_Q_TICKETS", "1")
    packed, spread = _both(wt, monkeypatch, n, cols, bc, how=how)
    assert not spread["status"].any() and np.all(spread["time"] == K)
    ref = _oracle_last_step(wt, oracle, n, N)
    assert np.array_equal(spread["stats"], ref), np.argwhere(spread["stats"] != ref)[:4].tolist()
    groups = ref[:5 * R].reshape(5, R, 5)
    assert np.any(groups != groups[:, :1]), "every packed group holds reactors with one set of counters"
    _assert_packed_equals_spread(packed, spread, (n, how), n)


# ---------------------------------------------------------------- (b) rare ends
def _rare_population(wt, n):
    """`_rare_group` over five groups and a lone reactor: clamp_cl in the first slot of group 0, clamp_ph_hi in a middle
    slot of group 1, clamp_ph_lo in the last slot of group 2, the cold run (0.05 K above the range's end: it raises in
    the middle of the item) in a middle slot of group 3, and a reactor whose pH is NaN from the start in the last slot of
    group 4."""
    R, N = ragged_size(n)
    where = (0, R + R // 2, 3 * R - 1, 3 * R + R // 2)
    cols, bc, pH, Cl, T, slots = _rare_group(wt, n, N, cold_T=0.05, where=where)
    slots["nonfinite"] = 5 * R - 1
    pH[slots["nonfinite"]] = np.nan
    return N, cols, bc, (pH, Cl, T, np.zeros(N)), slots


@pytest.mark.gpu
@pytest.mark.parametrize("limit", [0, 2])
@pytest.mark.parametrize("n", PACKED_NS)
def test_rare_ends(gpu, wt, monkeypatch, n, limit):
    """Reactors that clamp on the first step of a 9-step item, one that cools below 0 degC inside it and one that never
    steps, each beside ordinary reactors, in different groups and slots.  With an attempt limit of 2 the ordinary
    reactors fail outer steps beside ones that do not (and the clamp cases, which need more attempts, fail theirs).
    Status bits as test_clamps_and_a_raise_inside_an_item and test_lagging_reactors_in_one_wavefront assert them."""
    steps = 9
    N, cols, bc, state, slots = _rare_population(wt, n)
    R = 64 // n
    packed, spread = _both(wt, monkeypatch, n, cols, bc, steps=steps, state=state, limit=limit)
    st, c = spread["status"], slots["cold_run"]
    for name, bit in CLAMP_CASES.items():
        assert st[slots[name]] & bit, (name, st[slots[name]])
    assert st[slots["nonfinite"]] == ST_NONFINITE and spread["time"][slots["nonfinite"]] == 0
    ordinary = np.setdiff1d(np.arange(N), list(slots.values()))
    flagged = (st[ordinary] & ST_STEP_LIMIT) != 0
    if limit:
        # (the bit stays once set: over nine steps of the larger zone counts every ordinary reactor fails one, so "not
        # all" is asked where test_lagging_reactors_in_one_wavefront asks it, at eight reactors per wavefront and more)
        assert flagged.any(), st[ordinary]
        assert R < 8 or not flagged.all(), st[ordinary]
    else:
        # (the raise inside the item: a live step before it and frozen ones after, as without a limit in that module)
        assert st[c] & ST_T_RANGE and 1 <= spread["time"][c] <= steps - 2 and spread["bad_T"][c] < 0, (st[c], spread["time"][c])
        assert not st[ordinary].any() and np.all(spread["time"][ordinary] == steps)
    _assert_packed_equals_spread(packed, spread, (n, "limit", limit), n)


# ---------------------------------------------------------------- (c) edges
@pytest.mark.gpu
@pytest.mark.parametrize("n,dt,steps", [(5, 0.1, 6), (8, 10.0, 4), (12, 30.0, 3), (20, 100.0, 2), (3, 1.0, 6)])
def test_edge_population(gpu, wt, monkeypatch, n, dt, steps):
    """_random_edge_ensemble under an attempt limit of 300: reactors on the branches of the RHS -- no inlet flow, no
    Richardson number, stratification off or at its switches, the 8 degC density branch -- whose solves differ widely
    from their neighbours' in steps, rejections and Jacobian refreshes.  Against the oracle these are chaotic
    (test_edge_configurations_vs_oracle); against themselves they are not, so only packed against spread.  (At these
    sizes no reactor of the draw ends with a status bit -- the count is printed; frozen and clamped neighbours are
    test_rare_ends' part.)"""
    R, N = ragged_size(n)
    cols, bc = _random_edge_ensemble(wt, N, seed=1000 * n + int(dt * 10))
    packed, spread = _both(wt, monkeypatch, n, cols, bc, steps=steps, dt=dt, limit=300)
    print(f"n={n}, dt={dt}: {np.count_nonzero(spread['status'])} of {N} reactors end with a status bit")
    _assert_packed_equals_spread(packed, spread, (n, dt), n)
