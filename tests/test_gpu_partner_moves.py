"""Data movement taken out of the step kernel's trip loop: the partner exchange of the top
cyclic-reduction level at n = 8 without the copy of its operand, and the stage points and values of a trip defined
afresh instead of carried round the loop.  Neither may move a bit or a counter.  At n = 8 a packed wavefront holds eight reactors, two to a 16-lane DPP row, so a lane that the exchange
left unwritten, or wrote from the wrong half of its row, would hold the value of ANOTHER reactor: the tests run packed
(WT_FULL_WAVES, identity placement: reactor r sits in slot r % 8 of wavefront-group r // 8, in the lower half of row
(r % 8) // 2 where r is even and in the upper half where it is odd) against spread, against reactors run alone and
against the CPU oracle's counters."""
import numpy as np
import pytest

from program_helpers import Packing, set_packing
from test_gpu_pending_f import CLAMP_CASES, ST_T_RANGE, _assert_same, _fields, _rare_group

pytestmark = pytest.mark.gpu

N8, K8 = 41, 12          # 5 R + 1 reactors at n = 8 (R = 8 to a wavefront): five full wavefronts and a lone reactor


def _advance(wt, monkeypatch, name, n, cols, bc, how, steps, state=None, dt=1.0):
    """The ensemble advanced by `steps` outer steps with packing `name` ("packed": full wavefronts and the identity
    placement; "spread": the library's own dealing), the packing asserted after the last step; None: a run whose packing
    does not matter (a reactor alone).  Returns what the run left (``_fields``) and, for one-step calls, the counters
    after every call (steps, N, 5)."""
    p = None if name is None else Packing(name)
    if p is not None:
        set_packing(monkeypatch, name)
    ens = wt.ReactorEnsemble(cols, n_zones=n)
    if p is not None:
        p.place(ens)
    ens.set_boundary(bc)
    if state is not None:
        ens.set_state(*state)
    per_step = []
    if how == "one-step calls":
        for _ in range(steps):
            ens.step(dt, n_steps=1, download=False)
            per_step.append(ens.solver_stats().copy())
    else:
        ens.step(dt, n_steps=steps, download=False)
    f = _fields(ens)
    if p is not None:
        p.check(ens)
    ens.close()
    return f, np.array(per_step)


def _alone(wt, monkeypatch, n, cols, bc, state, r, how, steps):
    """Reactor r of the ensemble run by itself."""
    return _advance(wt, monkeypatch, None, n, {k: v[r:r + 1] for k, v in cols.items()}, np.ascontiguousarray(bc[:, r:r + 1]),
                    how, steps, tuple(np.ascontiguousarray(a[r:r + 1]) for a in state))


def _oracle_counters(wt, oracle, n, cols, bc, steps):
    """(steps, N, 5) nfev, njev, nlu, nsteps, nrej on the CPU: the oracle's single-reactor step chained over its own
    states from the ensemble's initial state."""
    ens = wt.ReactorEnsemble(cols, n_zones=n)
    ens.set_boundary(bc)
    par, s0 = ens.constants, ens.state
    ens.close()
    N = par.shape[1]
    ref = np.zeros((steps, N, 5), dtype=np.int32)
    for r in range(N):
        y, t = np.concatenate([s0.pH[r], s0.chlorine[r], s0.temperature[r]]), float(s0.time[r])
        for k in range(steps):
            y, t, _, status, st = oracle.step(n, par[:, r], bc[:, r], 1.0, y, t, want_stats=True)
            assert status == 0
            ref[k, r] = (st.nfev, st.njev, st.nlu, st.nsteps, st.nrej)
    return ref


# ---------------------------------------------------------------- 1. packed against spread, n = 8
def test_packed_equals_spread_and_the_oracle_counts(gpu, wt, oracle, monkeypatch):
    """41 reactors of 8 zones over a 12-step call and over twelve one-step calls, packed and spread: every reactor's bits
    are the same in the four runs, the counters after every one-step call are the same packed and spread, and they are
    the CPU oracle's.  Packed, a 16-lane row holds two different reactors side by side, and spread a reactor has its
    wavefront to itself: a lane the partner exchange did not write, or a stage value taken from the trip before, would
    differ between the two."""
    cols, bc = wt.make_ensemble(N8)
    got, counters = {}, {}
    for name in ("packed", "spread"):
        for how in ("one call", "one-step calls"):
            got[name, how], counters[name, how] = _advance(wt, monkeypatch, name, 8, cols, bc, how, K8)
    first = got["packed", "one call"]
    assert not first["status"].any() and np.all(first["time"] == K8)
    for key, f in got.items():
        _assert_same(first, f, ("packed one call", key))
    assert counters["packed", "one-step calls"].shape == (K8, N8, 5)
    assert np.array_equal(counters["packed", "one-step calls"], counters["spread", "one-step calls"])
    ref = _oracle_counters(wt, oracle, 8, cols, bc, K8)
    bad = np.argwhere(counters["packed", "one-step calls"] != ref)
    assert not len(bad), bad[:4].tolist()


# ---------------------------------------------------------------- 2. an odd reactor in either half of a row
@pytest.mark.parametrize("half", ["upper", "lower"])
def test_neighbours_of_an_odd_reactor_keep_their_bits(gpu, wt, monkeypatch, half):
    """The same packed 12-step run with the three clamp cases of g11 and g4's cold run (0.02 K above the range's end: it
    raises on the temperature range a step or two into the item) in rows 0, 1, 2 and 3 of four different wavefronts, in
    the upper half of their rows and then in the lower: `clamp_ph_lo` goes through some eighty internal steps with
    rejections while its row neighbour waits in PH_DONE, and the cold run ends in the middle of a solve.  The other half
    of each such row holds an ordinary reactor, which must keep the bits it has when run alone; the whole run equals the
    spread one."""
    odd = 1 if half == "upper" else 0
    where = (0 + odd, 10 + odd, 20 + odd, 30 + odd)          # slots 0/1, 2/3, 4/5, 6/7 of groups 0, 1, 2, 3
    cols, bc, pH, Cl, T, slots = _rare_group(wt, 8, N8, cold_T=0.02, where=where)
    state = (pH, Cl, T, np.zeros(N8))
    packed, _ = _advance(wt, monkeypatch, "packed", 8, cols, bc, "one call", K8, state)
    for name, bit in CLAMP_CASES.items():
        assert packed["status"][slots[name]] & bit, (name, packed["status"][slots[name]])
    c = slots["cold_run"]
    assert packed["status"][c] & ST_T_RANGE and 1 <= packed["time"][c] <= K8 - 2 and packed["bad_T"][c] < 0
    ordinary = np.setdiff1d(np.arange(N8), list(slots.values()))
    assert not packed["status"][ordinary].any() and np.all(packed["time"][ordinary] == K8)
    for s in slots.values():
        r = s ^ 1                                            # the other half of the row
        assert r in ordinary
        alone, _ = _alone(wt, monkeypatch, 8, cols, bc, state, r, "one call", K8)
        for k in packed:
            assert np.array_equal(packed[k][r:r + 1], alone[k], equal_nan=True), (half, s, r, k, packed[k][r], alone[k][0])
    spread, _ = _advance(wt, monkeypatch, "spread", 8, cols, bc, "one call", K8, state)
    # (the counters of the step that raised are stored only by a call in which the reactor also took a step)
    live = np.arange(N8) != c
    assert np.array_equal(packed["stats"][live], spread["stats"][live])
    del packed["stats"], spread["stats"]
    _assert_same(packed, spread, "packed / spread")


# ---------------------------------------------------------------- 3. reject, refine and repeated accepts
@pytest.mark.parametrize("n", [8, 4])
def test_repeated_accepts_beside_benign_reactors(gpu, wt, oracle, monkeypatch, n):
    """g11's `clamp_ph_lo` (the rejection fixture: its first step takes some eighty internal steps through pH 0..2 with
    rejected steps, second error estimates and Jacobian refreshes) in the first wavefront of a packed ensemble among
    ordinary reactors, forty one-step calls.  After every call the counters of that reactor and of its row neighbour are
    the CPU oracle's for a step from the state the device had before the call -- through reject, refine and repeated
    accepts, the trips in which a lane takes none of the paths that assign its stage values -- and the state after the
    fortieth equals, bit for bit, a run of the reactor alone and a single 40-step call of the ensemble."""
    R, steps = 64 // n, 40
    N = 2 * R + 1
    cols, bc, pH, Cl, T, slots = _rare_group(wt, n, N, cold_T=20.0, where=(R + 1, R + 3, 2, N - 1))
    s = slots["clamp_ph_lo"]
    state = (pH, Cl, T, np.zeros(N))
    set_packing(monkeypatch, "packed")
    p = Packing("packed")
    ens = p.place(wt.ReactorEnsemble(cols, n_zones=n))
    ens.set_boundary(bc)
    ens.set_state(*state)
    par = ens.constants
    watched = (s, s ^ 1)
    rejected = 0
    for k in range(steps):
        pre = ens.state
        ens.step(1.0, n_steps=1, download=False)
        got = ens.solver_stats()
        for r in watched:
            y = np.concatenate([pre.pH[r], pre.chlorine[r], pre.temperature[r]])
            _, _, _, _, st = oracle.step(n, par[:, r], bc[:, r], 1.0, y, float(pre.time[r]), want_stats=True)
            ref = (st.nfev, st.njev, st.nlu, st.nsteps, st.nrej)
            assert tuple(got[r]) == ref, (n, k, r, got[r], ref)
        rejected += int(got[s][4])
    assert rejected > 0, "the fixture no longer rejects a step"
    chained = _fields(ens)
    p.check(ens)
    ens.close()
    assert chained["status"][s] & CLAMP_CASES["clamp_ph_lo"] and chained["time"][s] == steps
    alone, _ = _alone(wt, monkeypatch, n, cols, bc, state, s, "one-step calls", steps)
    for k in chained:
        assert np.array_equal(chained[k][s:s + 1], alone[k], equal_nan=True), (n, k, chained[k][s], alone[k][0])
    one, _ = _advance(wt, monkeypatch, "packed", n, cols, bc, "one call", steps, state)
    for k in chained:
        assert np.array_equal(chained[k][s], one[k][s], equal_nan=True), (n, k, chained[k][s], one[k][s])


# ---------------------------------------------------------------- 4. the other zone counts
@pytest.mark.parametrize("n", [16, 5])
def test_other_zone_counts_packed_equals_spread(gpu, wt, monkeypatch, n):
    """n = 16 (a row rotation for the top level's partner) and n = 5 (the exchange row): eleven reactors, ten steps,
    packed against spread, bit for bit with the counters."""
    cols, bc = wt.make_ensemble(11)
    packed, _ = _advance(wt, monkeypatch, "packed", n, cols, bc, "one call", 10)
    spread, _ = _advance(wt, monkeypatch, "spread", n, cols, bc, "one call", 10)
    assert not packed["status"].any() and np.all(packed["time"] == 10)
    _assert_same(packed, spread, "packed / spread")
