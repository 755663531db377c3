"""The train program (include/wtphys.h ``wt_ensemble_train_*``): reactors coupled into treatment trains inside the
step call.  The fused call gives the bits of the host loop of one-step calls that copies outlets into ``set_boundary``
(train_ref.py) at every kernel instantiation and wavefront packing, whatever the schedule and the placement, with the
rest of the plant around it; a train behaves like one; frozen stages stop feeding; refusals and lifetime; and one train
stepped tank by tank with the CPU oracle."""

import numpy as np
import pytest

from program_helpers import DT, MASTER, assert_all_equal, full_waves, pi_loops, plant, plant_state, wavefront_groups  # noqa: F401
from train_ref import host_fed_loop, params

pytestmark = pytest.mark.gpu

E_LENGTH = "length must be at least 2 and at most 64 / n_zones (the stages of a train share a wavefront)"
E_MULTIPLE = "n_reactors must be a multiple of length (an ensemble holds whole trains)"
E_CONFLICT = "a disturbance slot targets an inlet row (1, 2 or 3) that the train program feeds into that reactor"
E_NOT_SET = "no train program is set (wt_ensemble_train_set)"


def _open(wt, cols, bc, n):
    ens = wt.ReactorEnsemble(cols, n_zones=n)
    ens.set_boundary(bc)
    return ens


def _core(ens):
    es = ens.state
    return (es.pH, es.chlorine, es.temperature, es.time, es.flow_rate, es.status, ens.solver_stats(), ens.boundary())


def _trains(ens):
    st = ens.train_state()
    return st.n_fed, st.t_last


# ---- 1. fused equals host loop, bit for bit, where the layout can go wrong
@pytest.mark.parametrize("full", [True, False], ids=["full_waves", "spread"])
@pytest.mark.parametrize("n, L", [(4, 3), (5, 5), (8, 2), (8, 8), (20, 3), (20, 2), (32, 2)])
def test_fused_equals_host_loop(gpu, wt, monkeypatch, n, L, full):
    if full:
        monkeypatch.setenv("WT_FULL_WAVES", "1")
    R = L * ((64 // n) // L) if full else L       # spread: a small ensemble gets one train per wavefront
    N, K = 3 * R + L, 12                          # the last wavefront-group holds one train
    cols, bc = wt.make_ensemble(N, seed=40 + n + L)
    u = np.random.default_rng(n * L).random(N)
    link = (u > 0.15).astype(np.float64)          # a few unlinked stages
    rows = np.where(u > 0.7, 5, 7)                # and a few that take pH and temperature only
    a = _open(wt, cols, bc, n)
    a.set_trains(L, linked=link, rows=rows)
    st = a.train_state()
    assert (st.length, st.per_wavefront) == (L, R)
    a.step(DT, n_steps=K, download=False)
    b = _open(wt, cols, bc, n)
    ref = host_fed_loop(b, K, L, link, rows)
    assert_all_equal(_core(b), _core(a), (n, L, full))
    assert not a.status().any()
    assert_all_equal((ref.n_fed, ref.t_last), _trains(a), "n_fed, t_last")
    assert ref.n_fed.max() == K and not np.array_equal(a.boundary()[1:4], wt.boundary_block(bc, N)[1:4])
    assert wavefront_groups(a) == -(-N // R)
    a.close(); b.close()


# ---- 2. the schedule changes no bit
def test_schedule_and_placement_change_no_bit(gpu, wt, monkeypatch, full_waves):
    n, L, N, K = 8, 4, 100, 60                    # two trains per wavefront, the last group holds one
    cols, bc = wt.make_ensemble(N, seed=77)
    rows = np.where(np.arange(N) % 3 == 0, 2, 7)

    def run(v):
        if v.get("tickets"):
            monkeypatch.setenv("WT_Q_TICKETS", "1")
        ens = _open(wt, cols, bc, n)
        ens.set_placement(v.get("adaptive", False))
        ens.set_schedule(v.get("streams", 0), v.get("chunk", 50))
        ens.set_trains(L, rows=rows)
        for c in v.get("calls", (K,)):
            ens.step(DT, n_steps=c, fused=v.get("fused", True), download=False)
        out = _core(ens) + _trains(ens)
        info = (ens.schedule(), ens.placement()[1])
        ens.close()
        monkeypatch.delenv("WT_Q_TICKETS", raising=False)
        return out, info

    ref, _ = run({})
    assert not ref[5].any() and np.all(ref[8][np.arange(N) % L != 0] == K)
    for v in (dict(chunk=1), dict(chunk=7), dict(streams=3, chunk=7), dict(fused=False), dict(tickets=True, chunk=7),
              dict(calls=(1,) * K)):
        assert_all_equal(ref, run(v)[0], v)
    # adaptive placement: the second call re-deals (35 >= 33 steps of history) -- whole trains, in stage order
    got, (sched, perm) = run(dict(adaptive=True, calls=(35, K - 35)))
    assert_all_equal(ref, got, "adaptive")
    assert sched["redeals"] >= 1 and sorted(perm.tolist()) == list(range(N))
    assert np.all(perm[::L] % L == 0)
    for j in range(1, L):
        assert np.array_equal(perm[j::L], perm[::L] + j)
    assert not np.array_equal(perm, np.arange(N)), "the re-deal moved no train: the placement went untested"


# ---- 3. with the rest of the plant
def test_with_plant_io_control_and_disturbances(gpu, wt, full_waves):
    n, L, N, K = 8, 4, 36, 30
    cols, bc = wt.make_ensemble(N, seed=5)
    base = wt.boundary_block(bc, N)
    chlorine, acid = pi_loops(wt, cols)
    u = np.random.default_rng(9).random(N)
    link = (u > 0.3).astype(np.float64)
    rows = np.where(u > 0.65, 2, 7)                # chlorine only on some
    # rows the train does not feed: ambient, the chlorine stock, and the first stages' inlet temperature
    dist = (wt.Disturbance.ou("ambient_temperature", 1.5, 300.0), wt.Disturbance.ramp("chlorine_concentration", -1e-3, 50.0, 250.0),
            wt.Disturbance("inlet_temperature", np.where(np.arange(N) % L == 0, "step", "off"), t_start=100.0, a=2.0))

    def start():
        ens = plant(wt, cols, bc, n)
        ens.set_schedule(0, 1)                     # a scan after every outer step, as the one-step calls have it
        ens.write_commands(*MASTER)
        ens.enable_control(chlorine, acid)
        ens.set_disturbances(*dist, seed=3)
        return ens

    everything = lambda ens: plant_state(ens) + ens.input_image() + (ens.control_state().block(),) + (
        ens.disturbance_state().value, ens.disturbance_state().x, ens.disturbance_state().n_draw)
    a = start()
    a.set_trains(L, linked=link, rows=rows)
    a.step(DT, n_steps=K, download=False)
    b = start()
    ref = host_fed_loop(b, K, L, link, rows, base=base)
    assert_all_equal(everything(b), everything(a), "plant")
    assert_all_equal((ref.n_fed, ref.t_last), _trains(a), "n_fed, t_last")
    got, lk = a.boundary(), params(N, L, link)[0] == 1.0
    only_cl = lk & (rows == 2)
    assert only_cl.any() and np.array_equal(got[[1, 3]][:, only_cl], base[[1, 3]][:, only_cl])   # rows the mask leaves out
    assert not np.array_equal(got[2][only_cl], base[2][only_cl])
    unlinked = ~lk & (np.arange(N) % L != 0)
    assert unlinked.any() and np.array_equal(got[1:4][:, unlinked], base[1:4][:, unlinked])
    assert not np.array_equal(got[[4, 6]], base[[4, 6]])                                           # the PI loops did dose
    assert not np.array_equal(got[[7, 8]], base[[7, 8]]) and not a.status().any()
    a.close(); b.close()


# ---- 4. it does what a train does
def test_a_chlorine_step_travels_down_the_train(gpu, wt):
    n, L, K = 4, 3, 12
    cfgs = [wt.ReactorConfiguration(n_zones=n, initial_chlorine=1.0)] * L
    b0 = wt.BoundaryConditions(inlet_chlorine=1.0)
    runs = []
    for raised in (False, True):
        ens = wt.ReactorEnsemble(cfgs)
        ens.set_boundary([b0] * L)
        ens.set_trains(L)
        if raised:                                  # a new base: the first stage's inlet chlorine steps up
            ens.set_boundary([wt.BoundaryConditions(inlet_chlorine=5.0)] + [b0] * (L - 1))
        fed, out = [ens.boundary()[2].copy()], []
        for _ in range(K):
            es = ens.step(DT, n_steps=1)
            fed.append(ens.boundary()[2].copy()); out.append(es.chlorine[:, -1].copy())
        runs.append((np.array(fed), np.array(out)))
        ens.close()
    (fed0, out0), (fed1, out1) = runs
    assert fed1[0, 0] == 5.0 and np.array_equal(fed1[0, 1:], fed0[0, 1:])          # set_boundary fed the links again
    # stage 1's fed row rises one step later, stage 2's two steps later; until then their bits are the quiet run's
    assert fed1[1, 1] > fed0[1, 1] and fed1[1, 2] == fed0[1, 2] and fed1[2, 2] > fed0[2, 2]
    # the outlets rise in stage order: stage s cannot know before step s + 1 (until then its bits are the quiet run's),
    # and a stage further down answers later (its first steps' answer is below the solver's resolution)
    for s in range(L):
        assert np.array_equal(out1[:s, s], out0[:s, s]), s
    first = [int(np.argmax(out1[:, s] > out0[:, s])) for s in range(L)]
    assert first[0] == 0 and first[0] < first[1] < first[2] and np.all(out1[-1] > out0[-1]), first


def test_an_all_unlinked_program_gives_the_bits_of_no_program(gpu, wt, full_waves):
    n, L, N, K = 8, 4, 40, 20
    cols, bc = wt.make_ensemble(N, seed=12)
    a, b = _open(wt, cols, bc, n), _open(wt, cols, bc, n)
    a.set_trains(L, linked=False)
    a.step(DT, n_steps=K, download=False); b.step(DT, n_steps=K, download=False)
    assert_all_equal(_core(b), _core(a), "all-unlinked")
    assert not a.train_state().n_fed.any() and np.isnan(a.train_state().t_last).all()
    a.close(); b.close()


# ---- 5. frozen stages
def test_a_frozen_upstream_stops_feeding(gpu, wt):
    from conftest import golden_json
    g = golden_json("g4_faults.json")["cold_run"]
    cold = wt.ReactorConfiguration(**g["config"])
    cb = wt.BoundaryConditions(**dict(zip(wt.params.BOUNDARY_FIELDS, g["bc"])))
    warm, wb = wt.ReactorConfiguration(n_zones=cold.n_zones), wt.BoundaryConditions()
    cfgs, bcs, L, K = [cold, warm, warm, warm], [cb, wb, wb, wb], 2, 60
    rows = ("pH", "chlorine")                      # (the cold tank's temperature would freeze its downstream too)

    def start():
        ens = wt.ReactorEnsemble(cfgs)
        ens.set_boundary(bcs)
        return ens

    a = start()
    a.set_trains(L, rows=rows)
    es = a.step(1.0, n_steps=K)
    b = start()
    ref = host_fed_loop(b, K, L, rows=3, dt=1.0)
    # (the solver counters of a reactor whose step raised are those of the launch that last stepped it: the raising
    # solve's in the fused call, the step's before it in one-step calls -- with or without a program)
    ca, cb = _core(a), _core(b)
    assert_all_equal(cb[:6] + (cb[6][1:], cb[7]), ca[:6] + (ca[6][1:], ca[7]), "frozen upstream")
    assert es.status[0] & 1 and es.time[0] < K and not es.status[1:].any() and np.all(es.time[1:] == K)
    st = a.train_state()
    assert_all_equal((ref.n_fed, ref.t_last), (st.n_fed, st.t_last), "n_fed, t_last")
    assert st.n_fed.tolist() == [0, es.time[0], 0, K] and st.t_last[1] == es.time[0] and st.t_last[3] == K
    # the downstream holds the rows of the last feed: the frozen state's outlet zone
    assert a.boundary()[1:3, 1].tolist() == [es.pH[0, -1], es.chlorine[0, -1]]
    a.close(); b.close()


# ---- 6. errors and lifetime
def _refused(fn, *args):
    with pytest.raises(ValueError) as ei:
        fn(*args)
    return str(ei.value)


def test_refusals(gpu, wt):
    L_ = gpu.lib()
    n, N = 8, 16
    cols, bc = wt.make_ensemble(N, seed=3)
    ens = wt.ReactorEnsemble(cols, n_zones=n)
    assert _refused(ens.set_trains, 2) == "set_state and set_boundary must precede train_set"
    ens.set_boundary(bc)
    assert _refused(ens.train_state) == E_NOT_SET
    ens.clear_trains()                              # no effect while none is set
    # the handle's own checks (the builder would stop these before the call)
    for length, blk, msg in ((9, None, E_LENGTH), (1, None, E_LENGTH), (3, None, E_MULTIPLE),
                             (2, np.array([[1.0] + [0.0] * (N - 1), [7.0] * N]), "the first stage of a train has no upstream: its link must be 0"),
                             (2, np.array([[0.0, 2.0] + [0.0] * (N - 2), [7.0] * N]), "link must be 0 or 1"),
                             (2, np.array([[0.0] * N, [7.5] + [7.0] * (N - 1)]), "rows must be an integer in 0..7 (1 pH, 2 chlorine, 4 temperature)")):
        assert L_.wt_ensemble_train_set(ens._h, length, gpu.dptr(blk)) == gpu.WT_E_ARG and L_.wt_last_error().decode() == msg
    assert _refused(ens.set_trains, 9) == E_LENGTH and _refused(ens.set_trains, 3) == E_MULTIPLE
    assert _refused(ens.train_state) == E_NOT_SET
    # a boundary schedule
    ens.set_trains(4)
    sched = np.ascontiguousarray(np.broadcast_to(wt.boundary_block(bc, N), (2, 10, N)))
    assert L_.wt_ensemble_step_scheduled(ens._h, DT, 2, 1, gpu.dptr(sched)) == gpu.WT_E_STATE
    assert L_.wt_last_error() == b"a boundary schedule cannot be combined with a train program (the run itself sets the linked rows)"
    assert "train program" in _refused(lambda: ens.step(DT, n_steps=2, boundary_schedule=sched))
    # the disturbance conflict, train first: a slot on a fed row of a linked reactor
    assert _refused(ens.set_disturbances, wt.Disturbance.step("inlet_chlorine", 0.5)) == E_CONFLICT
    first = (np.arange(N) % 4 == 0)
    only_first = wt.Disturbance("inlet_chlorine", np.where(first, "step", "off"), a=0.5)
    ens.set_disturbances(only_first, wt.Disturbance.step("ambient_temperature", 1.0))   # first stages are fed nothing
    ens.clear_disturbances()
    ens.set_trains(4, rows="chlorine")
    ens.set_disturbances(wt.Disturbance.step("inlet_pH", 0.1), wt.Disturbance.step("inlet_temperature", 1.0))   # rows the mask leaves out
    assert _refused(ens.set_disturbances, wt.Disturbance.step("inlet_pH", 0.1), wt.Disturbance.step(2, 1.0)) == E_CONFLICT
    # ... and disturbance first (the pH / temperature program is still set)
    assert _refused(ens.set_trains, 4) == E_CONFLICT
    assert _refused(ens.set_trains, 4, True, ("pH",)) == E_CONFLICT
    assert ens.train_state().length == 4            # a refused set leaves the program that was set
    ens.set_trains(2, rows="chlorine")
    ens.clear_disturbances()
    ens.close()
    # 33 zones and more hold no train
    cols2, bc2 = wt.make_ensemble(2, seed=1)
    big = _open(wt, cols2, bc2, 40)
    assert L_.wt_ensemble_train_set(big._h, 2, None) == gpu.WT_E_ARG and L_.wt_last_error().decode() == E_LENGTH
    big.close()


def test_lifetime_and_shape(gpu, wt, full_waves):
    n, N = 8, 44
    cols, bc = wt.make_ensemble(N, seed=21)
    base = wt.boundary_block(bc, N)
    ens = _open(wt, cols, bc, n)
    groups = wavefront_groups(ens)                  # (this also switches the wave diagnostics on)
    assert groups == -(-N // 8)
    ens.set_trains(4)
    assert ens.train_state().per_wavefront == 8 and wavefront_groups(ens) == groups
    ens.step(DT, n_steps=3, download=False)
    assert np.all(ens.train_state().n_fed[np.arange(N) % 4 != 0] == 3)
    # set twice replaces: new length, new shape, counts from 0, the rows of stages no longer linked back at the base
    ens.set_trains(2, linked=np.arange(N) % 4 == 1)
    st = ens.train_state()
    assert (st.length, st.per_wavefront) == (2, 8) and not st.n_fed.any() and np.isnan(st.t_last).all()
    got, lk = ens.boundary(), np.arange(N) % 4 == 1
    assert np.array_equal(got[:, ~lk], base[:, ~lk]) and not np.array_equal(got[1:4, lk], base[1:4, lk])
    assert np.array_equal(got[1:4, lk], np.stack([getattr(ens.state, f)[np.nonzero(lk)[0] - 1, -1] for f in ("pH", "chlorine", "temperature")]))
    ens.close()


def test_clear_restores_rows_and_shape(gpu, wt, full_waves):
    n, N, K = 20, 16, 10                            # 3 reactors per wavefront; trains of 2 leave one lane group idle
    cols, bc = wt.make_ensemble(N, seed=21)
    base = wt.boundary_block(bc, N)
    ens, fresh = _open(wt, cols, bc, n), _open(wt, cols, bc, n)
    groups = wavefront_groups(ens)
    assert groups == 6
    ens.set_trains(2)
    assert ens.train_state().per_wavefront == 2 and wavefront_groups(ens) == 8
    ens.step(DT, n_steps=K, download=False)
    assert not np.array_equal(ens.boundary(), base)
    state = ens.state
    ens.clear_trains()
    assert np.array_equal(ens.boundary(), base)
    assert _refused(ens.train_state) == E_NOT_SET and wavefront_groups(ens) == groups
    # the cleared handle steps like one that never had a program (from the same state)
    fresh.set_state(state.pH, state.chlorine, state.temperature, state.time)
    ens.step(DT, n_steps=K, download=False); fresh.step(DT, n_steps=K, download=False)
    assert_all_equal(_core(fresh), _core(ens), "after clear")
    ens.close(); fresh.close()
    # destroying the handle with a program set
    ens = _open(wt, cols, bc, n)
    ens.set_trains(2)
    ens.step(DT, n_steps=2, download=False)
    ens.close()


# ---- 7. against the oracle, tank by tank
@pytest.mark.parametrize("n", [4, 8])
def test_one_train_against_the_oracle(gpu, wt, oracle, n):
    L, K = 3, 40
    cols, bc = wt.make_ensemble(L, seed=8 + n)
    ens = _open(wt, cols, bc, n)
    s0 = ens.state
    ens.set_trains(L)
    es = ens.step(DT, n_steps=K)
    par, blk = ens.constants, wt.boundary_block(bc, L)
    y = [np.concatenate([s0.pH[r], s0.chlorine[r], s0.temperature[r]]) for r in range(L)]
    t, stats = [0.0] * L, [None] * L

    def feed():
        for r in range(1, L):
            blk[1:4, r] = y[r - 1][[n - 1, 2 * n - 1, 3 * n - 1]]

    feed()
    for _ in range(K):
        for r in range(L):
            y[r], t[r], _, status, stats[r] = oracle.step(n, par[:, r], blk[:, r], DT, y[r], t[r], want_stats=True)
            assert status == 0
        feed()
    from conftest import relerr
    want = np.array(y).reshape(L, 3, n)
    assert not es.status.any() and np.array_equal(es.time, t)
    assert relerr(es.pH, want[:, 0]) < 1e-7 and relerr(es.chlorine, want[:, 1]) < 1e-7 and relerr(es.temperature, want[:, 2]) < 1e-7
    assert relerr(ens.boundary()[1:4, 1:], blk[1:4, 1:]) < 1e-7
    got = ens.solver_stats()
    assert [tuple(got[r][:4]) for r in range(L)] == [(s.nfev, s.njev, s.nlu, s.nsteps) for s in stats]
    ens.close()
