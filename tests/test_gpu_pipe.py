"""The pipe program (include/wtphys.h ``wt_ensemble_pipe_*``): dead time between the stages of a treatment train inside
the step call.  The fused call gives the bits of the host loop of one-step calls with a FIFO per link (pipe_ref.py) at
every kernel instantiation and wavefront packing, whatever the schedule and the placement, with the rest of the plant
around it; delay 0 is the train program alone; a step travels down the train D steps late; a frozen upstream stalls its
line; refusals and lifetime; and one train stepped tank by tank with the CPU oracle and the same FIFO."""
from collections import deque

import numpy as np
import pytest

from pipe_ref import PipeRef, host_piped_loop
from program_helpers import DT, MASTER, assert_all_equal, full_waves, pi_loops, plant, plant_state  # noqa: F401
from train_ref import host_fed_loop, params

pytestmark = pytest.mark.gpu

E_DELAY = "delay must be a whole number in 0..4095 (outer steps)"
E_UNLINKED = "a stage that is not linked has no pipe: its delay must be 0"
E_NO_TRAIN = "no train program is set (wt_ensemble_train_set)"
E_NO_PIPE = "no pipe program is set (wt_ensemble_pipe_set)"


def _open(wt, cols, bc, n):
    ens = wt.ReactorEnsemble(cols, n_zones=n)
    ens.set_boundary(bc)
    return ens


def _core(ens):
    es = ens.state
    return (es.pH, es.chlorine, es.temperature, es.time, es.flow_rate, es.status, ens.solver_stats(), ens.boundary())


def _pipes(ens):
    """In the order of ``PipeRef.state``."""
    ts, ps = ens.train_state(), ens.pipe_state()
    return ts.n_fed, ts.t_last, ps.n_sent, ps.t_sent, ens.pipe_lines()


def _delays(N, L, K, link=None):
    """Per link, in turn, from {1, 0, K + 3, 2, 5, 3}: three links already give a line that delivers real samples, an
    undelayed link next to it and a line that never finishes emptying its initial fill (K + 3 > K)."""
    linked = np.nonzero(params(N, L, link)[0] == 1.0)[0]
    delay = np.zeros(N, dtype=np.int64)
    delay[linked] = np.array([1, 0, K + 3, 2, 5, 3])[np.arange(len(linked)) % 6]
    return delay


def _refused(fn, *args):
    with pytest.raises(ValueError) as ei:
        fn(*args)
    return str(ei.value)


# ---- 1. fused equals host loop, bit for bit, where the layout can go wrong
@pytest.mark.parametrize("full", [True, False], ids=["full_waves", "spread"])
@pytest.mark.parametrize("n, L", [(4, 3), (5, 5), (8, 2), (8, 8), (20, 3), (32, 2)])
def test_fused_equals_host_loop(gpu, wt, monkeypatch, n, L, full):
    if full:
        monkeypatch.setenv("WT_FULL_WAVES", "1")
    R = L * ((64 // n) // L) if full else L       # spread: a small ensemble gets one train per wavefront
    N, K = 3 * R + L, 12                          # the last wavefront-group holds one train
    cols, bc = wt.make_ensemble(N, seed=40 + n + L)
    u = np.random.default_rng(n * L).random(N)
    link = (u > 0.15).astype(np.float64)          # a few unlinked stages
    rows = np.where(u > 0.7, 5, 7)                # and a few that take pH and temperature only
    delay = _delays(N, L, K, link)
    a = _open(wt, cols, bc, n)
    a.set_trains(L, linked=link, rows=rows)
    a.set_pipes(delay)
    assert a.train_state().per_wavefront == R
    a.step(DT, n_steps=K, download=False)
    b = _open(wt, cols, bc, n)
    ref = host_piped_loop(b, K, L, delay, link, rows)
    assert_all_equal(_core(b), _core(a), (n, L, full))
    assert not a.status().any()
    assert_all_equal(ref.state(), _pipes(a), "n_fed, t_last, n_sent, t_sent, lines")
    ps = a.pipe_state()
    assert np.array_equal(ps.delay, ref.delay) and ps.slots == ref.delay.max() + 1
    # the case is one: an undelayed link, a line that delivered real samples, one that only gave its initial fill
    assert ((ref.delay == 0) & (ref.link == 1.0)).any() and ref.n_sent.max() == K and np.isfinite(ref.t_sent).any()
    assert (ref.delay == K + 3).any() and np.isnan(ref.t_sent[ref.delay == K + 3]).all()
    a.close(); b.close()


# ---- 2. delay 0 is the train program alone
def test_delay_zero_gives_the_bits_of_the_train_program(gpu, wt, full_waves):
    n, L, N, K = 8, 4, 40, 20
    cols, bc = wt.make_ensemble(N, seed=12)
    rows = np.where(np.arange(N) % 3 == 0, 2, 7)
    got = []
    for v in ("trains", "zero", "cleared"):
        ens = _open(wt, cols, bc, n)
        ens.set_trains(L, rows=rows)
        if v == "zero":
            ens.set_pipes(0)
        if v == "cleared":
            ens.set_pipes(4)
            ens.clear_pipes()
            assert _refused(ens.pipe_state) == E_NO_PIPE
        ens.step(DT, n_steps=K, download=False)
        ts = ens.train_state()
        got.append(_core(ens) + (ts.n_fed, ts.t_last))
        if v == "zero":
            ps = ens.pipe_state()
            assert not ps.n_sent.any() and np.isnan(ps.t_sent).all() and ps.slots == 1 and ens.pipe_lines().shape == (0, 4, N)
        ens.close()
    assert_all_equal(got[0], got[1], "delay 0")
    assert_all_equal(got[0], got[2], "set, then cleared")
    assert np.all(got[0][8][np.arange(N) % L != 0] == K)


# ---- 3. the schedule changes no bit
def test_schedule_and_placement_change_no_bit(gpu, wt, monkeypatch, full_waves):
    n, L, N, K = 8, 4, 100, 60                    # two trains per wavefront, the last group holds one
    cols, bc = wt.make_ensemble(N, seed=77)
    rows = np.where(np.arange(N) % 3 == 0, 2, 7)
    delay = _delays(N, L, K)

    def run(v):
        if v.get("tickets"):
            monkeypatch.setenv("WT_Q_TICKETS", "1")
        ens = _open(wt, cols, bc, n)
        ens.set_placement(v.get("adaptive", False))
        ens.set_schedule(v.get("streams", 0), v.get("chunk", 50))
        ens.set_trains(L, rows=rows)
        ens.set_pipes(delay)
        for c in v.get("calls", (K,)):
            ens.step(DT, n_steps=c, fused=v.get("fused", True), download=False)
        out = _core(ens) + _pipes(ens)
        info = (ens.schedule(), ens.placement()[1])
        ens.close()
        monkeypatch.delenv("WT_Q_TICKETS", raising=False)
        return out, info

    ref, _ = run({})
    linked = np.arange(N) % L != 0
    assert not ref[5].any() and np.all(ref[8][linked] == K) and np.array_equal(ref[10], np.where(linked & (delay > 0), K, 0))
    for v in (dict(chunk=1), dict(chunk=7), dict(streams=3, chunk=7), dict(fused=False), dict(tickets=True, chunk=7),
              dict(calls=(1,) * K)):
        assert_all_equal(ref, run(v)[0], v)
    # adaptive placement: the second call re-deals (35 >= 33 steps of history) -- whole trains, in stage order
    got, (sched, perm) = run(dict(adaptive=True, calls=(35, K - 35)))
    assert_all_equal(ref, got, "adaptive")
    assert sched["redeals"] >= 1 and sorted(perm.tolist()) == list(range(N))
    assert not np.array_equal(perm, np.arange(N)), "the re-deal moved no train: the placement went untested"


# ---- 4. with the rest of the plant
def test_with_plant_io_control_and_disturbances(gpu, wt, full_waves):
    n, L, N, K = 8, 4, 36, 30
    cols, bc = wt.make_ensemble(N, seed=5)
    base = wt.boundary_block(bc, N)
    chlorine, acid = pi_loops(wt, cols)
    u = np.random.default_rng(9).random(N)
    link = (u > 0.3).astype(np.float64)
    rows = np.where(u > 0.65, 2, 7)                # chlorine only on some
    delay = _delays(N, L, K, link)
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
    a.set_pipes(delay)
    a.step(DT, n_steps=K, download=False)
    b = start()
    ref = host_piped_loop(b, K, L, delay, link, rows, base=base)
    assert_all_equal(everything(b), everything(a), "plant")
    assert_all_equal(ref.state(), _pipes(a), "n_fed, t_last, n_sent, t_sent, lines")
    got = a.boundary()
    assert not np.array_equal(got[[4, 6]], base[[4, 6]]) and not np.array_equal(got[[7, 8]], base[[7, 8]])   # PI and disturbances ran
    assert np.isfinite(ref.t_sent).any() and not a.status().any()
    a.close(); b.close()


# ---- 5. a step arrives D steps late
def test_a_chlorine_step_arrives_a_dead_time_late(gpu, wt):
    n, L, K, D1, D2 = 4, 3, 12, 2, 3
    cfgs = [wt.ReactorConfiguration(n_zones=n, initial_chlorine=1.0)] * L
    b0 = wt.BoundaryConditions(inlet_chlorine=1.0)

    def run(raised, piped):
        ens = wt.ReactorEnsemble(cfgs)
        ens.set_boundary([b0] * L)
        ens.set_trains(L)
        if piped:
            ens.set_pipes([0, D1, D2])
        if raised:                                  # a new base: the first stage's inlet chlorine steps up
            ens.set_boundary([wt.BoundaryConditions(inlet_chlorine=5.0)] + [b0] * (L - 1))
        fed, times, sent = [ens.boundary()[2].copy()], [ens.state.time.copy()], []
        for _ in range(K):
            es = ens.step(DT, n_steps=1)
            fed.append(ens.boundary()[2].copy()); times.append(es.time.copy())
            if piped:
                sent.append(ens.pipe_state().t_sent.copy())
        ens.close()
        return np.array(fed), np.array(times), np.array(sent)

    def first_departure(fed1, fed0, s):
        differs = fed1[:, s] != fed0[:, s]
        assert differs.any(), s
        return int(np.argmax(differs))

    plain0, plain1 = run(False, False)[0], run(True, False)[0]
    (fed0, _, _), (fed1, times, sent) = run(False, True), run(True, True)
    assert fed1[0, 0] == 5.0 and np.array_equal(fed1[0, 1:], fed0[0, 1:])
    at = [first_departure(plain1, plain0, s) for s in (1, 2)]
    assert at == [1, 2]
    # stage 1's fed row departs D1 steps later than without pipes, stage 2's D1 + D2 later; until then the quiet bits
    assert [first_departure(fed1, fed0, s) for s in (1, 2)] == [at[0] + D1, at[1] + D1 + D2]
    assert fed1[at[0] + D1, 1] > fed0[at[0] + D1, 1] and fed1[at[1] + D1 + D2, 2] > fed0[at[1] + D1 + D2, 2]
    # what arrives is what left: the fed row after feed k is the undelayed run's row of D feeds before
    assert np.array_equal(fed1[1 + D1:, 1], plain1[1:K + 1 - D1, 1])
    # t_sent: the upstream's time D feeds ago once D + 1 feeds have passed, NaN while the initial fill comes out
    for s, D in ((1, D1), (2, D2)):
        assert np.isnan(sent[:D, s]).all()
        assert np.array_equal(sent[D:, s], times[1:K + 1 - D, s - 1])
    assert np.isnan(sent[:, 0]).all()


# ---- 6. a frozen upstream stalls its line
def test_a_frozen_upstream_stalls_its_line(gpu, wt):
    from conftest import golden_json
    g = golden_json("g4_faults.json")["cold_run"]
    cold = wt.ReactorConfiguration(**g["config"])
    cb = wt.BoundaryConditions(**dict(zip(wt.params.BOUNDARY_FIELDS, g["bc"])))
    warm, wb = wt.ReactorConfiguration(n_zones=cold.n_zones), wt.BoundaryConditions()
    cfgs, bcs, L, K, more = [cold, warm, warm, warm], [cb, wb, wb, wb], 2, 60, 5
    rows = ("pH", "chlorine")                      # (the cold tank's temperature would freeze its downstream too)
    delay = [0, 3, 0, 2]

    def start():
        ens = wt.ReactorEnsemble(cfgs)
        ens.set_boundary(bcs)
        return ens

    a = start()
    a.set_trains(L, rows=rows)
    a.set_pipes(delay)
    es = a.step(1.0, n_steps=K)
    assert es.status[0] & 1 and es.time[0] < K and not es.status[1:].any() and np.all(es.time[1:] == K)
    at_k = _pipes(a) + (a.boundary()[1:4, 1].copy(),)
    frozen_at = es.time[0]                          # (dt = 1: the steps the cold tank took)
    assert at_k[2].tolist() == [0, frozen_at, 0, K] and at_k[0].tolist() == [0, frozen_at, 0, K]
    assert at_k[3][1] == frozen_at - 3 and at_k[3][3] == K - 2
    es = a.step(1.0, n_steps=more)
    # the line of link 1 stalled: nothing sent, nothing popped, the downstream holds its rows and goes on stepping
    now = _pipes(a)
    assert now[2][1] == frozen_at and now[3][1] == frozen_at - 3 and np.array_equal(now[4][:, :, 1], at_k[4][:, :, 1], equal_nan=True)
    assert np.array_equal(a.boundary()[1:4, 1], at_k[5]) and es.time[1] == K + more and es.time[0] == frozen_at
    assert now[2][3] == K + more and now[3][3] == K + more - 2
    b = start()
    ref = host_piped_loop(b, K + more, L, delay, rows=3, dt=1.0)
    # (the solver counters of a reactor whose step raised are those of the launch that last stepped it: the raising
    # solve's in the fused call, the step's before it in one-step calls -- with or without a program)
    ca, cb_ = _core(a), _core(b)
    assert_all_equal(cb_[:6] + (cb_[6][1:], cb_[7]), ca[:6] + (ca[6][1:], ca[7]), "frozen upstream")
    assert_all_equal(ref.state(), now, "n_fed, t_last, n_sent, t_sent, lines")
    a.close(); b.close()


# ---- 7. errors and lifetime
def test_refusals(gpu, wt):
    L_ = gpu.lib()
    n, N = 8, 16
    cols, bc = wt.make_ensemble(N, seed=3)
    ens = _open(wt, cols, bc, n)
    assert _refused(ens.set_pipes, 2) == E_NO_TRAIN and _refused(ens.pipe_state) == E_NO_PIPE
    assert L_.wt_ensemble_pipe_set(ens._h, gpu.dptr(np.zeros(N))) == gpu.WT_E_STATE and L_.wt_last_error().decode() == E_NO_TRAIN
    ens.clear_pipes()                               # no effect while none is set
    ens.set_trains(4, linked=np.arange(N) != 5)
    assert _refused(ens.pipe_state) == E_NO_PIPE and _refused(ens.pipe_lines) == E_NO_PIPE
    # the handle's own checks (the builder would stop these before the call), in the order of wt_pipe_check
    d = lambda r, v: np.where(np.arange(N) == r, v, 0.0)
    for delay, msg in ((d(1, 4096.0), E_DELAY), (d(1, -1.0), E_DELAY), (d(1, 0.5), E_DELAY), (d(2, np.nan), E_DELAY),
                       (d(0, 1.0), E_UNLINKED), (d(4, 3.0), E_UNLINKED), (d(5, 3.0), E_UNLINKED),
                       (d(5, 3.0) + d(6, 5000.0), E_UNLINKED), (d(5, 5000.0), E_DELAY)):
        assert L_.wt_ensemble_pipe_set(ens._h, gpu.dptr(delay)) == gpu.WT_E_ARG and L_.wt_last_error().decode() == msg
    assert L_.wt_ensemble_pipe_set(ens._h, None) == gpu.WT_E_ARG
    assert _refused(ens.set_pipes, 4096) == E_DELAY and _refused(ens.pipe_state) == E_NO_PIPE   # a refused set sets nothing
    ens.set_pipes(3)                                # the builder zeroes first stages and the unlinked reactor 5
    assert ens.pipe_state().delay.tolist() == [0 if r % 4 == 0 or r == 5 else 3 for r in range(N)]
    assert _refused(ens.set_pipes, -1) == E_DELAY and ens.pipe_state().slots == 4   # ... and leaves the program that was set
    ens.close()


def test_lifetime(gpu, wt, full_waves):
    n, L, N, K = 8, 4, 44, 6
    cols, bc = wt.make_ensemble(N, seed=21)
    base = wt.boundary_block(bc, N)
    linked = np.arange(N) % L != 0
    outlet = lambda es: np.stack([es.pH[:, -1], es.chlorine[:, -1], es.temperature[:, -1]])
    ens = _open(wt, cols, bc, n)
    s0 = ens.state
    ens.set_trains(L)
    delay = np.where(np.arange(N) % L == 2, 0, 2)
    ens.set_pipes(delay)
    ens.step(DT, n_steps=K, download=False)
    ps = ens.pipe_state()
    piped = linked & (delay > 0)
    assert np.array_equal(ps.n_sent, np.where(piped, K, 0)) and ps.slots == 3 and ens.pipe_lines().shape == (2, 4, N)
    # set twice replaces: new delays, new lines full of the upstream's outlet as it is now, the state from the start
    ens.set_pipes(5)
    ps, es = ens.pipe_state(), ens.state
    ref = PipeRef(N, L, 5)
    ref.fill(es)
    assert ps.slots == 6 and not ps.n_sent.any() and np.isnan(ps.t_sent).all() and np.array_equal(ps.delay, ref.delay)
    assert np.array_equal(ens.pipe_lines(), ref.lines(), equal_nan=True)
    assert np.array_equal(ens.boundary()[1:4, 1:][:, linked[1:]], outlet(es)[:, :-1][:, linked[1:]])   # every link delivered again
    assert ens.train_state().n_fed[1] == K          # the train program's own state is not restarted
    # set_boundary re-delivers: a line's last delivered sample where D >= 1, the upstream's state where D = 0
    ens.set_pipes(delay)
    ens.step(DT, n_steps=K, download=False)
    before, es = ens.boundary(), ens.state
    ens.set_boundary(base + 1.0)
    got = ens.boundary()
    assert np.array_equal(got[1:4, piped], before[1:4, piped]) and np.array_equal(got[:, ~linked], base[:, ~linked] + 1.0)
    undelayed = linked & (delay == 0)
    assert np.array_equal(got[1:4, undelayed], outlet(es)[:, np.nonzero(undelayed)[0] - 1])
    assert not np.array_equal(got[1:4, piped], outlet(es)[:, np.nonzero(piped)[0] - 1])        # the delayed rows lag the state
    assert np.array_equal(got[[0, 4, 5, 6, 7, 8, 9]], base[[0, 4, 5, 6, 7, 8, 9]] + 1.0)
    # set_state: a new state is a new plant -- the lines full of it, the pipe state from the start, every link delivered
    ens.set_state(s0.pH, s0.chlorine, s0.temperature, s0.time)
    ref = PipeRef(N, L, delay)
    ref.fill(s0)
    ps = ens.pipe_state()
    assert not ps.n_sent.any() and np.isnan(ps.t_sent).all() and np.array_equal(ens.pipe_lines(), ref.lines(), equal_nan=True)
    assert np.array_equal(ens.boundary()[1:4, linked], outlet(s0)[:, np.nonzero(linked)[0] - 1])
    # train_set over a program clears the pipes, and so does train_clear
    ens.set_trains(2)
    assert _refused(ens.pipe_state) == E_NO_PIPE
    ens.set_pipes(1)
    assert ens.pipe_state().delay.tolist() == [0, 1] * (N // 2)
    ens.clear_trains()
    assert _refused(ens.pipe_state) == E_NO_PIPE and _refused(ens.set_pipes, 1) == E_NO_TRAIN
    assert np.array_equal(ens.boundary(), base + 1.0)
    ens.close()
    # destroying the handle with a program set
    ens = _open(wt, cols, bc, n)
    ens.set_trains(L)
    ens.set_pipes(delay)
    ens.step(DT, n_steps=2, download=False)
    ens.close()


def test_pipes_set_after_some_steps_of_a_train_program(gpu, wt, full_waves):
    n, L, N, K0, K = 8, 4, 20, 5, 9
    cols, bc = wt.make_ensemble(N, seed=31)
    rows = np.where(np.arange(N) % 5 == 1, 3, 7)
    delay = _delays(N, L, K)
    a = _open(wt, cols, bc, n)
    a.set_trains(L, rows=rows)
    a.step(DT, n_steps=K0, download=False)
    a.set_pipes(delay)                              # fill and deliver from the state in memory
    a.step(DT, n_steps=K, download=False)
    b = _open(wt, cols, bc, n)
    head = host_fed_loop(b, K0, L, rows=rows)
    ref = host_piped_loop(b, K, L, delay, rows=rows)   # the host loop started at that point
    assert_all_equal(_core(b), _core(a), "set after steps")
    got = _pipes(a)
    assert_all_equal((head.n_fed + ref.train.n_fed, ref.train.t_last) + ref.state()[2:], got, "n_fed, t_last, n_sent, t_sent, lines")
    assert np.nanmin(got[3]) > K0 * DT - 1e-9 and np.isfinite(got[3]).any()   # no sample older than the set call
    a.close(); b.close()


# ---- 8. against the oracle, tank by tank, with the same FIFO
@pytest.mark.parametrize("n", [4, 8])
def test_one_train_against_the_oracle(gpu, wt, oracle, n):
    L, K, D = 3, 40, (0, 2, 3)
    cols, bc = wt.make_ensemble(L, seed=8 + n)
    ens = _open(wt, cols, bc, n)
    s0 = ens.state
    ens.set_trains(L)
    ens.set_pipes(D)
    es = ens.step(DT, n_steps=K)
    par, blk = ens.constants, wt.boundary_block(bc, L)
    y = [np.concatenate([s0.pH[r], s0.chlorine[r], s0.temperature[r]]) for r in range(L)]
    t, stats = [0.0] * L, [None] * L
    out = lambda r: y[r][[n - 1, 2 * n - 1, 3 * n - 1]]
    line = [deque([out(r - 1).copy()] * D[r]) for r in range(L)]
    for r in range(1, L):
        blk[1:4, r] = out(r - 1)
    for _ in range(K):
        for r in range(L):
            y[r], t[r], _, status, stats[r] = oracle.step(n, par[:, r], blk[:, r], DT, y[r], t[r], want_stats=True)
            assert status == 0
        for r in range(1, L):
            line[r].append(out(r - 1).copy())
            blk[1:4, r] = line[r].popleft()
    from conftest import relerr
    want = np.array(y).reshape(L, 3, n)
    assert not es.status.any() and np.array_equal(es.time, t)
    assert relerr(es.pH, want[:, 0]) < 1e-7 and relerr(es.chlorine, want[:, 1]) < 1e-7 and relerr(es.temperature, want[:, 2]) < 1e-7
    assert relerr(ens.boundary()[1:4, 1:], blk[1:4, 1:]) < 1e-7
    lines = ens.pipe_lines()
    for r in range(1, L):
        assert relerr(lines[:D[r], :3, r], np.array(line[r])) < 1e-7 and np.array_equal(lines[:D[r], 3, r], np.array(t[r - 1]) - DT * np.arange(D[r])[::-1])
    got = ens.solver_stats()
    assert [tuple(got[r][:4]) for r in range(L)] == [(s.nfev, s.njev, s.nlu, s.nsteps) for s in stats]
    ens.close()
