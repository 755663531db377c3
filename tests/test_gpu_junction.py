"""The junction program (include/wtphys.h ``wt_ensemble_junction_*``): flow-weighted merges and splits of a treatment
train inside the step call.  The fused call gives the bits of the host loop of one-step calls with the numpy blend
between them (junction_ref.py) wherever no blended pH enters, and that blend within ``PH_TOL`` where one does, at every
kernel instantiation class and wavefront packing, whatever the schedule and the placement, with pipes and the rest of
the plant around it; a program of single upstream sources is the train program; a throttled branch shifts the blend; a
frozen source holds the junction; refusals and lifetime; checkpoints; and one diamond stepped tank by tank with the CPU
oracle."""
import numpy as np
import pytest

import junction_ref as JR
from program_helpers import DT, MASTER, assert_all_equal, full_waves, pi_loops, plant, plant_state  # noqa: F401

pytestmark = pytest.mark.gpu

K = 12
E_NO_TRAIN = "no train program is set (wt_ensemble_train_set)"
E_NOT_SET = "no junction program is set (wt_ensemble_junction_set)"
E_PIPES = "junctions must be set before the pipes (a line holds what its junction delivered)"
E_PLANT_IO = "a carried flow cannot be combined with plant I/O (the scan's command path writes row 0 in the same outer step)"
E_ROW0 = "rows 0, 4 and 6 (inlet, acid and chlorine flow) belong to the command path or the master"
E_FED_ROW = "a disturbance slot targets an inlet row (1, 2 or 3) that the train program feeds into that reactor"
E_STAGE = "a source's stage must be -1 (the slot is unused) or a whole number in 0..length - 1 (a stage of the same train)"
E_OWN = "a junction cannot be its own source"
E_TWICE = "a stage can be a source of a junction once only"
E_SHARE = "a source's share must be finite and in (0, 1]"
E_LINK = "a junction needs a linked reactor (the train program's link; a first stage has none)"
E_CARRY = "carry must be 0 or 1"
E_CARRY_NONE = "carry needs a junction: a reactor without a used slot carries no flow"

# (n, L) -> junctions as (to_stage, from_stages, carry): the diamonds, a 3-way merge with a recycle in a ROW = false
# kernel, a merge that straddles the rows of the n = 20 kernel, one carried single source at two lanes per reactor half
SHAPES = {(4, 4): [(3, (1, 2), True)], (8, 4): [(3, (1, 2), True)],
          (5, 5): [(4, (1, 2, 3), True), (1, (0, 4), False)],
          (20, 3): [(2, (0, 1), True)], (32, 2): [(1, (0,), True)]}


def _open(wt, cols, bc, n):
    ens = wt.ReactorEnsemble(cols, n_zones=n)
    ens.set_boundary(bc)
    return ens


def _core(ens):
    es = ens.state
    return (es.pH, es.chlorine, es.temperature, es.time, es.flow_rate, es.status, ens.solver_stats(), ens.boundary())


def _jstate(ens):
    """In the order of ``JunctionRef.state``."""
    ts, js = ens.train_state(), ens.junction_state()
    return ts.n_fed, ts.t_last, js.n_blend, js.n_held, js.q_last


def _refused(fn, *args):
    with pytest.raises(ValueError) as ei:
        fn(*args)
    return str(ei.value)


def _case(wt, n, L, full, carry=True, rows=(2, 4, 6), seed=0):
    """N reactors in 3 wavefront-groups, the last one partial; junctions with shares that differ from train to train on
    all but every fourth train; a few plain stages unlinked.  Returns (N, R, link, rows, wt.Junction list, ref spec)."""
    R = L * ((64 // n) // L) if full else L
    N = 2 * R + L
    rng = np.random.default_rng(100 * n + L + seed)
    trains = np.nonzero(np.arange(N // L) % 4 != 3)[0]
    if trains.size == N // L:                          # fewer than four trains: the last one stays a plain chain
        trains = trains[:-1]
    junctions, spec, is_j = [], [], np.zeros(N, dtype=bool)
    for to, src, c in SHAPES[(n, L)]:
        shares = np.round(rng.uniform(0.1, 1.0, (len(src), trains.size)), 3)
        junctions.append(wt.Junction(to, src, shares, carry=c and carry, trains=trains))
        spec.append((to, src, shares, c and carry, trains))
        is_j[trains * L + to] = True
    u = rng.random(N)
    link = ((u > 0.15) | is_j).astype(np.float64)
    link[::L] = 0.0
    link[N - L + 1:] = 1.0                             # the last train: a plain chain, every stage fed by its upstream
    row = np.asarray(rows)[rng.integers(0, len(rows), N)]
    return N, R, link, row, junctions, spec


def _ref(N, L, link, rows, spec, delay=None):
    return JR.JunctionRef(N, L, *JR.program(N, L, spec), link=link, rows=rows, delay=delay)


# ---- 1. fused equals host loop, bit for bit (no blended pH enters: the rows mask is within chlorine | temperature)
@pytest.mark.parametrize("full", [True, False], ids=["full_waves", "spread"])
@pytest.mark.parametrize("n, L", list(SHAPES))
def test_fused_equals_host_loop(gpu, wt, monkeypatch, n, L, full):
    if full:
        monkeypatch.setenv("WT_FULL_WAVES", "1")
    N, R, link, rows, junctions, spec = _case(wt, n, L, full)
    cols, bc = wt.make_ensemble(N, seed=40 + n + L)
    a = _open(wt, cols, bc, n)
    a.set_trains(L, linked=link, rows=rows)
    a.set_junctions(*junctions)
    assert a.train_state().per_wavefront == R and a.info(gpu.WT_INFO_JUNCTION) == 1
    a.step(DT, n_steps=K, download=False)
    b = _open(wt, cols, bc, n)
    ref = JR.host_junction_loop(b, K, _ref(N, L, link, rows, spec))
    assert_all_equal(_core(b), _core(a), (n, L, full))
    assert not a.status().any()
    assert_all_equal(ref.state(), _jstate(a), "n_fed, t_last, n_blend, n_held, q_last")
    blk, carry = a.junction_params()
    assert np.array_equal(blk[:, 0], ref.stage) and np.array_equal(blk[:, 1], ref.share) and np.array_equal(carry, ref.carry)
    # the case is one: junctions that blended every step, a carried flow that differs from the base, plain links too
    base = wt.boundary_block(bc, N)
    assert ref.n_blend.max() == K and (ref.n_blend == 0).sum() > N // L
    carriers = ref.carry == 1.0
    assert carriers.any() and not np.any(a.boundary()[0, carriers] == base[0, carriers])
    assert np.array_equal(a.boundary()[0, ~carriers], base[0, ~carriers]) and np.array_equal(a.boundary()[1], base[1])
    assert ((ref.n_fed == K) & (ref.n_blend == 0)).any()
    a.close(); b.close()


# ---- 2. every row, the blended pH too; schedule and placement change no bit
def _runs(wt, monkeypatch, n, L, link, rows, junctions, cols, bc, v):
    if v.get("tickets"):
        monkeypatch.setenv("WT_Q_TICKETS", "1")
    if v.get("adaptive"):
        monkeypatch.setenv("WT_PLACE_MIN", "5")
    ens = _open(wt, cols, bc, n)
    monkeypatch.delenv("WT_Q_TICKETS", raising=False)
    monkeypatch.delenv("WT_PLACE_MIN", raising=False)
    ens.set_placement(v.get("adaptive", False))
    ens.set_schedule(0, v.get("chunk", 50))
    ens.set_trains(L, linked=link, rows=rows)
    ens.set_junctions(*junctions)
    return ens


@pytest.mark.parametrize("full", [True, False], ids=["full_waves", "spread"])
@pytest.mark.parametrize("n, L", list(SHAPES))
def test_every_row_with_the_blended_pH(gpu, wt, monkeypatch, n, L, full):
    if full:
        monkeypatch.setenv("WT_FULL_WAVES", "1")
    N, R, link, rows, junctions, spec = _case(wt, n, L, full, rows=(7, 7, 3, 5), seed=1)
    cols, bc = wt.make_ensemble(N, seed=60 + n + L)
    # K one-step calls on the programmed handle: after each, the fed rows are the numpy blend of that call's state and
    # the row 0 in force during it -- chlorine, temperature and the carried flow in its bits, the pH within PH_TOL
    a = _runs(wt, monkeypatch, n, L, link, rows, junctions, cols, bc, {})
    ref = _ref(N, L, link, rows, spec)
    es, blk = a.state, a.boundary()
    want = wt.boundary_block(bc, N).copy()              # (the block may be ``bc`` itself: the later runs start from it)
    ref.feed_outside(want, es)
    worst = float(np.max(np.abs(blk[1] - want[1])))
    assert np.array_equal(blk[[0, 2, 3]], want[[0, 2, 3]]) and np.array_equal(blk[4:], want[4:]) and worst <= JR.PH_TOL
    for k in range(K):
        t0, want = es.time, blk.copy()
        es = a.step(DT, n_steps=1)
        ref.after_step(want, es, t0, blk[0])
        blk = a.boundary()
        assert np.array_equal(blk[[0, 2, 3]], want[[0, 2, 3]]) and np.array_equal(blk[4:], want[4:]), k
        worst = max(worst, float(np.max(np.abs(blk[1] - want[1]))))
    print(f"n={n} L={L} full={full}: max |pH(device) - pH(numpy)| over {K} feeds = {worst:.3e}")
    assert worst <= JR.PH_TOL
    assert_all_equal(ref.state(), _jstate(a), "counters")
    blended = (ref.n_blend == K) & (np.asarray(rows) & 1 == 1) & np.array([len(ref.sources(d)) > 1 for d in range(N)])
    assert blended.any() == any(len(src) > 1 for _, src, _ in SHAPES[(n, L)]) and not a.status().any()
    calls = _core(a) + _jstate(a)
    a.close()
    # the K-step fused call, the queue's chunks, separate launches, the ticket split and a re-dealt placement: the same bits
    for v in (dict(), dict(chunk=1), dict(chunk=7), dict(fused=False), dict(tickets=True, chunk=7), dict(adaptive=True, calls=(6, K - 6))):
        ens = _runs(wt, monkeypatch, n, L, link, rows, junctions, cols, bc, v)
        for c in v.get("calls", (K,)):
            ens.step(DT, n_steps=c, fused=v.get("fused", True), download=False)
        assert_all_equal(calls, _core(ens) + _jstate(ens), (n, L, full, v))
        if v.get("adaptive"):
            perm = ens.placement()[1]
            assert ens.schedule()["redeals"] >= 1 and np.all(perm[::L] % L == 0)
            assert all(np.array_equal(perm[j::L], perm[::L] + j) for j in range(1, L))
        ens.close()
    # the host loop with the numpy blend: its pH rows differ in the last bits, the trajectories agree as trajectories do
    from conftest import relerr
    b = _open(wt, cols, bc, n)
    JR.host_junction_loop(b, K, _ref(N, L, link, rows, spec))
    cb = _core(b)
    assert all(relerr(calls[i], cb[i]) < 1e-7 for i in range(3)) and np.array_equal(calls[3], cb[3])
    b.close()


# ---- 3. single upstream sources, no sources, set and clear: the train program's bits
def test_single_source_and_empty_programs_are_the_train_program(gpu, wt, full_waves):
    n, L, N = 8, 4, 40
    cols, bc = wt.make_ensemble(N, seed=12)
    rows = np.where(np.arange(N) % 3 == 0, 2, 7)
    got = {}
    for v in ("trains", "chain", "empty", "cleared"):
        ens = _open(wt, cols, bc, n)
        ens.set_trains(L, rows=rows)
        if v == "chain":                               # every stage names its upstream, with some share of its flow
            ens.set_junctions(*[wt.Junction(s, (s - 1,), 0.25 * s) for s in range(1, L)])
        if v == "empty":
            ens.set_junctions()
        if v == "cleared":
            ens.set_junctions(wt.Junction(3, (1, 2), 0.5, carry=True), wt.Junction(1, (0, 3), (1.0, 0.1)))
            assert not np.array_equal(ens.boundary()[0], wt.boundary_block(bc, N)[0])
            ens.clear_junctions()
            assert _refused(ens.junction_state) == E_NOT_SET and ens.info(gpu.WT_INFO_JUNCTION) == 0
        if v == "trains":
            first = ens.boundary()
        else:
            assert np.array_equal(ens.boundary(), first), v
        ens.step(DT, n_steps=K, download=False)
        ts = ens.train_state()
        got[v] = _core(ens) + (ts.n_fed, ts.t_last)
        if v == "chain":
            js = ens.junction_state()
            assert np.all(js.n_blend[np.arange(N) % L != 0] == K) and not js.n_held.any()
            stage = np.arange(N) % L
            assert np.array_equal(js.q_last[stage != 0], (0.25 * stage * ens.boundary()[0, np.arange(N) - 1])[stage != 0])
        if v == "empty":
            js = ens.junction_state()
            assert not js.n_blend.any() and not js.n_held.any() and np.isnan(js.q_last).all()
        ens.close()
    for v in ("chain", "empty", "cleared"):
        assert_all_equal(got["trains"], got[v], v)
    assert np.all(got["trains"][8][np.arange(N) % L != 0] == K)


# ---- 4. it does what a merge does
def test_a_chlorine_step_on_one_branch_reaches_the_merge_with_its_weight(gpu, wt):
    n, L = 8, 4
    cfgs = [wt.ReactorConfiguration(n_zones=n, initial_chlorine=1.0)] * L
    flows = (12.0, 8.0, 4.0, 5.0)
    b0 = [wt.BoundaryConditions(inlet_chlorine=1.0, inlet_flow_rate=q) for q in flows]
    f1, f2 = 0.75, 0.5
    runs = []
    for raised in (False, True):
        ens = wt.ReactorEnsemble(cfgs)
        ens.set_boundary(b0)
        ens.set_trains(L, linked=[0, 1, 1, 1], rows=("chlorine", "temperature"))
        ens.set_junctions(wt.Junction(1, (0,), 0.6), wt.Junction(2, (0,), 0.4), wt.Junction(3, (1, 2), (f1, f2), carry=True))
        bnd, out, q_last = [ens.boundary()], [], []
        for k in range(K):
            if raised and k == 2:                       # stage 1's outlet steps up: a new state, fed again from memory
                s = ens.state
                cl = s.chlorine.copy()
                cl[1] += 2.0
                ens.set_state(s.pH, cl, s.temperature, s.time)
            if raised and k == 7:                       # stage 1's valve halves: a new base, the blend moves to stage 2
                blk = ens.boundary()
                blk[0, 1] *= 0.5
                blk[0, 3] = flows[3]
                ens.set_boundary(blk)
            es = ens.step(DT, n_steps=1)
            bnd.append(ens.boundary()); out.append(es.chlorine[:, -1].copy()); q_last.append(ens.junction_state().q_last[3])
        runs.append((np.array(bnd), np.array(out), np.array(q_last)))
        ens.close()
    (b_q, o_q, q_q), (b_r, o_r, q_r) = runs
    # until the step the bits are the quiet run's; the feed after it is the numpy blend, bit for bit
    assert np.array_equal(b_r[:3], b_q[:3]) and np.array_equal(o_r[:2], o_q[:2])
    Q1, Q2 = f1 * flows[1], f2 * flows[2]
    for k in (2, 5):
        (_, cl, _), Qs = JR.blend([7.0, 7.0], o_r[k, 1:3], [20.0, 20.0], [Q1, Q2])
        assert b_r[k + 1, 2, 3] == cl and b_r[k + 1, 0, 3] == Qs == Q1 + Q2 == q_r[k]
    w = Q1 / (Q1 + Q2)
    rise = b_r[3, 2, 3] - b_q[3, 2, 3]
    assert abs(rise - w * (o_r[2, 1] - o_q[2, 1])) < 1e-12 and rise > 0.5
    assert np.array_equal(o_r[2, [0, 2]], o_q[2, [0, 2]]) and o_r[-1, 3] > o_q[-1, 3]          # the other branch knows nothing
    # the halved valve: Qs and the weights follow at the next feed
    (_, cl, _), Qs = JR.blend([7.0, 7.0], o_r[8, 1:3], [20.0, 20.0], [0.5 * Q1, Q2])
    assert q_r[6] == Q1 + Q2 and q_r[8] == Qs == 0.5 * Q1 + Q2 and b_r[9, 2, 3] == cl and b_r[9, 0, 3] == Qs
    assert np.all(q_q == Q1 + Q2)


# ---- 5. a frozen source
def test_a_source_that_raises_holds_the_junction(gpu, wt):
    from conftest import golden_json
    g = golden_json("g4_faults.json")["cold_run"]
    cold = wt.ReactorConfiguration(**g["config"])
    cb = wt.BoundaryConditions(**dict(zip(wt.params.BOUNDARY_FIELDS, g["bc"])))
    warm, wb = wt.ReactorConfiguration(n_zones=cold.n_zones), wt.BoundaryConditions()
    cfgs, bcs, L, steps = [warm, cold, warm, warm] * 2, [wb, cb, wb, wb] * 2, 4, 60
    rows = np.array([6] * 4 + [2] * 4)                  # (train 0 takes the cold blend's temperature too, train 1 chlorine only)
    spec = [(3, (1, 2), (0.5, 0.75), True, None)]

    def start():
        ens = wt.ReactorEnsemble(cfgs)
        ens.set_boundary(bcs)
        return ens

    a = start()
    a.set_trains(L, rows=rows)
    a.set_junctions(wt.Junction(3, (1, 2), (0.5, 0.75), carry=True))
    es = a.step(1.0, n_steps=steps)
    b = start()
    ref = JR.host_junction_loop(b, steps, _ref(8, L, None, rows, spec), dt=1.0)
    ca, cb_ = _core(a), _core(b)
    # (the solver counters of a reactor whose step raised are those of the launch that last stepped it)
    cold_r = np.array([1, 5])
    keep = np.setdiff1d(np.arange(8), cold_r)
    assert_all_equal(cb_[:6] + (cb_[6][keep], cb_[7]), ca[:6] + (ca[6][keep], ca[7]), "frozen source")
    assert_all_equal(ref.state(), _jstate(a), "counters")
    t_stop = es.time[1]
    assert es.status[1] & 1 and 0 < t_stop < steps and np.all(es.time[keep] == steps) and not es.status[keep].any()
    js = a.junction_state()
    assert js.n_blend[3] == t_stop and js.n_held[3] == steps - t_stop and js.n_blend[7] == t_stop
    assert a.train_state().t_last[3] == t_stop and js.n_held[[1, 2]].tolist() == [0, 0]
    a.close(); b.close()


# ---- 6. pipes on top: the lines carry blended samples
def _same_lines(got, want):
    """Chlorine, temperature and stamps in their bits; the pH of a blended sample within PH_TOL."""
    assert got.shape == want.shape and np.array_equal(got[:, 1:], want[:, 1:], equal_nan=True)
    assert np.array_equal(np.isnan(got[:, 0]), np.isnan(want[:, 0])) and np.nanmax(np.abs(got[:, 0] - want[:, 0])) <= JR.PH_TOL


@pytest.mark.parametrize("n, L", [(8, 4), (5, 5)])
def test_pipes_carry_the_blend(gpu, wt, full_waves, n, L):
    N, R, link, rows, junctions, spec = _case(wt, n, L, True, seed=2)
    cols, bc = wt.make_ensemble(N, seed=33 + n)
    probe = _ref(N, L, link, rows, spec)
    delay = np.zeros(N, dtype=np.int64)
    js = np.array([d for d in range(N) if probe.sources(d)])
    delay[js] = np.array([2, 0, K + 3])[np.arange(js.size) % 3]
    plain = np.nonzero((link == 1.0) & (delay == 0))[0]
    delay[plain[::2]] = 1
    delay[js[1]] = 0
    a = _open(wt, cols, bc, n)
    a.set_trains(L, linked=link, rows=rows)
    a.set_junctions(*junctions)
    a.set_pipes(delay)
    assert _refused(a.set_junctions, *junctions) == E_PIPES and _refused(a.clear_junctions) == E_PIPES
    b = _open(wt, cols, bc, n)
    ref = _ref(N, L, link, rows, spec, delay=delay)
    # the lines from the start: D copies of the blend from memory
    es0, base = b.state, wt.boundary_block(bc, N)
    first = base.copy()
    ref.feed_outside(first, es0)
    ref.fill(es0, first[0])
    lines = a.pipe_lines()
    _same_lines(lines, ref.lines())
    d2 = js[0]
    (_, cl, _, _), Qs, _ = ref.sample(d2, es0, first[0])
    assert lines[0, 1, d2] == lines[1, 1, d2] == cl and Qs > 0
    a.step(DT, n_steps=K, download=False)
    JR.host_junction_loop(b, K, ref)
    assert_all_equal(_core(b), _core(a), (n, L))
    ps, ts = a.pipe_state(), a.train_state()
    assert_all_equal(ref.state() + (ref.n_sent, ref.t_sent), _jstate(a) + (ps.n_sent, ps.t_sent), "counters")
    _same_lines(a.pipe_lines(), ref.lines())
    assert ref.n_sent[d2] == K and np.isfinite(ref.t_sent[d2]) and np.isnan(ref.t_sent[delay == K + 3]).all()
    a.close(); b.close()


# ---- 7. with plant I/O, both PI loops, a wire from the merged stage and a disturbance
def test_with_plant_io_control_wire_and_disturbance(gpu, wt, full_waves):
    n, L = 8, 4
    N, R, link, rows, junctions, spec = _case(wt, n, L, True, carry=False, seed=3)
    cols, bc = wt.make_ensemble(N, seed=5)
    base = wt.boundary_block(bc, N)
    chlorine, acid = pi_loops(wt, cols)
    dist = (wt.Disturbance.ou("ambient_temperature", 1.5, 300.0),)

    def start(linked):
        ens = plant(wt, cols, bc, n)
        ens.set_schedule(0, 1)                          # a scan after every outer step, as the one-step calls have it
        ens.write_commands(*MASTER)
        ens.enable_control(chlorine, acid)
        ens.set_disturbances(*dist, seed=3)
        ens.set_trains(L, linked=linked, rows=rows)
        ens.set_wires(wt.Wire("chlorine_outlet", 0, 3))  # stage 0 doses on the merged stage's analyser
        return ens

    everything = lambda ens: plant_state(ens) + ens.input_image() + (ens.control_state().block(),) + (
        ens.disturbance_state().value, ens.disturbance_state().x, ens.wire_state().block())
    a = start(link)
    a.set_junctions(*junctions)
    a.step(DT, n_steps=K, download=False)
    b = start(False)                                    # the wires need a train program: one that links nothing
    ref = JR.host_junction_loop(b, K, _ref(N, L, link, rows, spec), base=base)
    assert_all_equal(everything(b), everything(a), "plant")
    assert_all_equal(ref.state(), _jstate(a), "counters")
    got = a.boundary()
    assert not np.array_equal(got[[4, 6]], base[[4, 6]]) and not np.array_equal(got[8], base[8]) and not a.status().any()
    assert np.array_equal(got[1], base[1]) and ref.n_blend.max() == K and a.wire_state().n_routed[3, ::L].min() == K
    a.close(); b.close()


# ---- 8. refusals and lifetime
def test_refusals(gpu, wt):
    L_ = gpu.lib()
    n, N, L = 8, 16, 4
    cols, bc = wt.make_ensemble(N, seed=3)
    ens = _open(wt, cols, bc, n)
    assert _refused(ens.set_junctions, wt.Junction(3, (1, 2))) == E_NO_TRAIN
    assert _refused(ens.junction_state) == E_NOT_SET and _refused(ens.junction_params) == E_NOT_SET
    ens.clear_junctions()                               # no effect while none is set
    linked = np.arange(N) % L != 2
    ens.set_trains(L, linked=linked)
    assert _refused(ens.junction_state) == E_NOT_SET

    def raw(at=(), carry=()):
        blk = np.zeros((4, 2, N)); blk[:, 0] = -1.0
        blk[0, :, 3], blk[1, :, 3] = (1.0, 0.5), (0.0, 0.25)
        for k, f, r, v in at:
            blk[k, f, r] = v
        c = np.zeros(N)
        for r, v in carry:
            c[r] = v
        rc = L_.wt_ensemble_junction_set(ens._h, gpu.dptr(blk), gpu.dptr(c))
        return rc, L_.wt_last_error().decode()

    for at, carry, msg in ((((2, 0, 3, 4.0),), (), E_STAGE), (((2, 0, 3, 0.5),), (), E_STAGE), (((2, 0, 3, 3.0),), (), E_OWN),
                           (((2, 0, 3, 1.0),), (), E_TWICE), (((1, 1, 3, 0.0),), (), E_SHARE), (((1, 1, 3, np.nan),), (), E_SHARE),
                           (((0, 0, 2, 1.0), (0, 1, 2, 1.0)), (), E_LINK), (((0, 0, 4, 1.0), (0, 1, 4, 1.0)), (), E_LINK),
                           ((), ((3, 0.5),), E_CARRY), ((), ((5, 1.0),), E_CARRY_NONE),
                           # in this order at one reactor, and the first bad reactor speaks
                           (((2, 0, 3, 9.0), (1, 0, 3, 3.0), (0, 1, 3, 2.0)), ((3, 2.0),), E_STAGE),
                           (((1, 0, 3, 3.0), (0, 1, 3, 2.0)), ((3, 2.0),), E_OWN), (((0, 1, 3, 2.0),), ((3, 2.0),), E_SHARE),
                           (((0, 1, 3, 2.0), (0, 0, 7, 9.0)), (), E_SHARE), (((0, 0, 7, 9.0),), ((3, 2.0),), E_CARRY)):
        assert raw(at, carry) == (gpu.WT_E_ARG, msg), (at, carry)
    assert L_.wt_ensemble_junction_set(ens._h, None, None) == gpu.WT_E_ARG and _refused(ens.junction_state) == E_NOT_SET
    assert raw()[0] == gpu.WT_OK and raw(carry=((3, 1.0),))[0] == gpu.WT_OK
    # the disturbance program: row 0 is never its to move, carried or not, so the two cannot meet; a junction's fed
    # rows are the train program's
    assert E_ROW0 in _refused(ens.set_disturbances, wt.Disturbance.step(0, 0.5))
    assert _refused(ens.set_disturbances, wt.Disturbance.step("inlet_chlorine", 0.5)) == E_FED_ROW
    ens.set_disturbances(wt.Disturbance.step("ambient_temperature", 1.0))
    assert raw(carry=((3, 1.0),))[0] == gpu.WT_OK       # ... in either order
    ens.clear_disturbances()
    # a carried flow against plant I/O, junctions first ...
    assert raw(carry=((3, 1.0),))[0] == gpu.WT_OK
    ens.enable_sensors(seed=1)
    with pytest.raises(gpu.WtError) as ei:
        ens.enable_plant_io()
    assert (ei.value.code, ei.value.message) == (gpu.WT_E_STATE, E_PLANT_IO)
    assert raw()[0] == gpu.WT_OK
    ens.enable_plant_io()
    # ... and plant I/O first
    assert raw(carry=((3, 1.0),)) == (gpu.WT_E_STATE, E_PLANT_IO) and raw()[0] == gpu.WT_OK
    # the pipes come last
    ens.set_pipes(2)
    assert raw() == (gpu.WT_E_STATE, E_PIPES) and _refused(ens.clear_junctions) == E_PIPES
    ens.clear_pipes()
    ens.clear_junctions()
    ens.close()


def test_lifetime(gpu, wt, full_waves):
    n, N, L = 8, 44, 4
    cols, bc = wt.make_ensemble(N, seed=21)
    base = wt.boundary_block(bc, N)
    ens, fresh = _open(wt, cols, bc, n), _open(wt, cols, bc, n)
    ens.set_trains(L)
    fresh.set_trains(L)
    ens.set_junctions(wt.Junction(3, (1, 2), (0.5, 0.25), carry=True))
    ens.step(DT, n_steps=3, download=False)
    js = ens.junction_state()
    assert np.all(js.n_blend[3::L] == 3) and not js.n_blend[np.arange(N) % L != 3].any()
    assert np.array_equal(js.q_last[3::L], 0.5 * base[0, 1::L] + 0.25 * base[0, 2::L])
    # a second set replaces the first: the old carriers' flows back at the base, the state from the start
    ens.set_junctions(wt.Junction(2, (0, 1), 1.0, carry=True, trains=[0, 1]))
    js, got = ens.junction_state(), ens.boundary()
    assert not js.n_blend.any() and np.isnan(js.q_last).all()
    assert np.array_equal(got[0, 3::L], base[0, 3::L]) and np.array_equal(got[0, [2, 6]], base[0, [0, 4]] + base[0, [1, 5]])
    assert np.array_equal(got[0, 10::L], base[0, 10::L])
    blk, carry = ens.junction_params()
    assert blk[:, 0, 2].tolist() == [0, 1, -1, -1] and blk[0, 0, 3] == -1 and carry.nonzero()[0].tolist() == [2, 6]
    ens.step(DT, n_steps=3, download=False)
    # clear restores rows and row 0, then feeds as the train program: the handle goes on like one that never had junctions
    state = ens.state
    ens.clear_junctions()
    fresh.set_state(state.pH, state.chlorine, state.temperature, state.time)
    assert np.array_equal(ens.boundary(), fresh.boundary()) and np.array_equal(ens.boundary()[0], base[0])
    ens.step(DT, n_steps=K, download=False); fresh.step(DT, n_steps=K, download=False)
    assert_all_equal(_core(fresh), _core(ens), "after clear")
    # train_clear clears the junctions: rows and carried flows back at the base
    ens.set_junctions(wt.Junction(3, (1, 2), 0.5, carry=True))
    assert not np.array_equal(ens.boundary()[0], base[0])
    ens.clear_trains()
    assert np.array_equal(ens.boundary(), base) and ens.info(gpu.WT_INFO_JUNCTION) == 0
    ens.set_trains(L)
    assert _refused(ens.junction_state) == E_NOT_SET    # a new train program starts without junctions
    ens.set_junctions(wt.Junction(3, (1, 2), 0.5, carry=True))
    ens.set_trains(L)                                   # ... and a set over a program clears them too
    assert np.array_equal(ens.boundary()[0], base[0]) and _refused(ens.junction_state) == E_NOT_SET
    ens.close(); fresh.close()
    # destroying the handle with a program set
    ens = _open(wt, cols, bc, n)
    ens.set_trains(L)
    ens.set_junctions(wt.Junction(3, (1, 2), 0.5, carry=True))
    ens.step(DT, n_steps=2, download=False)
    ens.close()


# ---- 9. checkpoints carry the program
def test_checkpoint_clone_and_rewind_continue_alike(gpu, wt, full_waves):
    import checkpoint_helpers as CH
    n, L = 8, 4
    N, R, link, rows, junctions, spec = _case(wt, n, L, True, rows=(7, 6, 3), seed=4)
    cols, bc = wt.make_ensemble(N, seed=9)
    delay = np.where((link == 1.0) & (np.arange(N) % 3 == 0), 2, 0)

    def build():
        ens = _open(wt, cols, bc, n)
        ens.set_trains(L, linked=link, rows=rows)
        ens.set_junctions(*junctions)
        ens.set_pipes(delay)
        return ens

    def snap(ens):
        return CH.snapshot(ens) + _jstate(ens) + ens.junction_params()

    a = build()
    a.step(DT, n_steps=5, download=False)
    blob = a.checkpoint()
    a.mark()
    twin = a.clone()
    other = _open(wt, cols, bc, n)
    other.restore(blob)
    assert other.info(gpu.WT_INFO_JUNCTION) == 1
    CH.same("restored", snap(a)[1:], snap(other)[1:])   # (the info codes differ in WT_INFO_MARK)
    CH.same("clone", snap(a)[1:], snap(twin)[1:])
    a.step(DT, n_steps=4, download=False)
    want4 = snap(a)
    a.step(DT, n_steps=3, download=False)
    want7 = snap(a)
    for name, ens in (("restored", other), ("clone", twin)):
        ens.step(DT, n_steps=4, download=False)
        CH.same((name, 4), want4[1:], snap(ens)[1:])
        ens.step(DT, n_steps=3, download=False)
        CH.same((name, 7), want7[1:], snap(ens)[1:])
    a.clear_pipes(); a.clear_junctions()                # the rewind brings both back
    a.rewind()
    a.step(DT, n_steps=4, download=False)
    CH.same("rewound", want4, snap(a))
    assert a.junction_state().n_blend.max() == 9
    for ens in (a, twin, other):
        ens.close()


# ---- 10. against the oracle, tank by tank
@pytest.mark.parametrize("n", [4, 8])
def test_one_diamond_against_the_oracle(gpu, wt, oracle, n):
    from conftest import relerr
    L, steps = 4, 40
    cols, bc = wt.make_ensemble(L, seed=8 + n)
    ens = _open(wt, cols, bc, n)
    s0 = ens.state
    ens.set_trains(L)
    ens.set_junctions(wt.Junction(1, (0,), 0.6), wt.Junction(2, (0,), 0.4), wt.Junction(3, (1, 2), (0.7, 0.9), carry=True))
    es = ens.step(DT, n_steps=steps)
    par, blk = ens.constants, wt.boundary_block(bc, L)
    y = [np.concatenate([s0.pH[r], s0.chlorine[r], s0.temperature[r]]) for r in range(L)]
    t, stats = [0.0] * L, [None] * L
    out = lambda r: y[r][[n - 1, 2 * n - 1, 3 * n - 1]]

    def feed():
        q0 = blk[0].copy()
        blk[1:4, 1], blk[1:4, 2] = out(0), out(0)
        (p, c, T), Qs = JR.blend(*np.array([out(1), out(2)]).T, [0.7 * q0[1], 0.9 * q0[2]])
        blk[1:4, 3], blk[0, 3] = (p, c, T), Qs

    feed()
    for _ in range(steps):
        for r in range(L):
            y[r], t[r], _, status, stats[r] = oracle.step(n, par[:, r], blk[:, r], DT, y[r], t[r], want_stats=True)
            assert status == 0
        feed()
    want = np.array(y).reshape(L, 3, n)
    assert not es.status.any() and np.array_equal(es.time, t)
    assert relerr(es.pH, want[:, 0]) < 1e-7 and relerr(es.chlorine, want[:, 1]) < 1e-7 and relerr(es.temperature, want[:, 2]) < 1e-7
    assert relerr(ens.boundary()[:4, 1:], blk[:4, 1:]) < 1e-7
    got = ens.solver_stats()
    assert [tuple(got[r][:4]) for r in range(L)] == [(s.nfev, s.njev, s.nlu, s.nsteps) for s in stats]
    ens.close()
