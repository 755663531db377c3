"""Per-reactor disturbance programs after every outer step (include/wtphys.h ``wt_ensemble_disturb_*``): invisible when
off, the device follows the restatement in disturb_ref.py, a disturbed run replays bit for bit through a boundary
schedule, results do not depend on the schedule or the sharding, the OU statistics hold, and a PI loop feels it."""
import ctypes as C
import math

import numpy as np
import pytest

from disturb_ref import DS_N_DRAW, DS_N_EVAL, DS_VALUE, DS_X, DisturbRef, clamp_row, compose_rows
from program_helpers import DT, MASTER, assert_all_equal, pi_loops, plant, plant_state, refused_as_checked

pytestmark = pytest.mark.gpu

INF = np.inf


def _mixed(wt, N, seed=3):
    """OU on inlet pH and inlet chlorine, SINE on inlet temperature, STEP on ambient (per-reactor parameters)."""
    u = np.random.default_rng(seed).random((6, N))
    return (wt.Disturbance.ou("inlet_pH", 0.05 + 0.2 * u[0], 300.0 + 600.0 * u[1]),
            wt.Disturbance.ou("inlet_chlorine", 0.05 + 0.2 * u[2], 600.0),
            wt.Disturbance.sine("inlet_temperature", 2.0 + u[3], 1800.0, phase=u[4]),
            wt.Disturbance.step("ambient_temperature", -4.0, 200.0 + 400.0 * u[5], 2000.0))


def _open(wt, cols, bc, n):
    ens = wt.ReactorEnsemble(cols, n_zones=n)
    ens.set_boundary(bc)
    return ens


def _dsts(ens):
    st = ens.disturbance_state()
    off, filled = ens.disturbance_history()
    return (st.value, st.x, st.n_eval, st.n_draw, st.base, st.t_prev, off, filled, ens.boundary())


@pytest.mark.parametrize("n", [4, 8, 20, 32])
def test_invisible_when_off(gpu, wt, n):
    N, K = 96, 40
    cols, bc = wt.make_ensemble(N, seed=900 + n)
    outs = []
    for mode in ("none", "off", "cleared"):
        ens = plant(wt, cols, bc, n, seed=4)
        ens.write_commands(*MASTER)
        if mode == "off":
            ens.set_disturbances(wt.Disturbance("inlet_pH"), wt.Disturbance(8, "off"), history=5)
        if mode == "cleared":
            ens.set_disturbances(*_mixed(wt, N), history=5)
            ens.clear_disturbances()
        ens.step(DT, n_steps=K, download=False)
        outs.append(plant_state(ens) + ens.input_image())
        if mode == "off":
            assert np.all(ens.disturbance_state().n_eval == K + 1)
        ens.close()
    assert_all_equal(outs[0], outs[1], "all-OFF program")
    assert_all_equal(outs[0], outs[2], "cleared program")


def test_matches_restatement(gpu, wt):
    N, n, K = 64, 8, 30
    cols, bc = wt.make_ensemble(N, seed=17)
    u = np.random.default_rng(2).random((4, N))
    prog = (wt.Disturbance.step("inlet_temperature", 3.0 * u[0], 50.0 + 100.0 * u[1], 200.0),
            wt.Disturbance.ramp("chlorine_concentration", -1e-4, 30.0, 250.0, offset=0.02),
            wt.Disturbance.sine("ambient_temperature", 5.0, 120.0 + 60.0 * u[2], phase=u[3]),
            wt.Disturbance.ou("inlet_chlorine", 0.3, 90.0, 20.0, 220.0))
    block = wt.disturbance_block(N, *prog)
    ens = _open(wt, cols, bc, n)
    ens.set_disturbances(*prog, seed=99, reactor_base=5, history=K + 4)
    ref = DisturbRef(block, wt.boundary_block(bc, N), np.zeros(N), seed=99, reactor_base=5, history=K + 4)
    exact = [0, 1, 3, 4, 5, 6, 7, 9]       # untouched, STEP and RAMP rows: bit for bit
    for k in range(K + 1):
        got = ens.boundary()
        assert np.array_equal(got[exact], ref.bc[exact]), k
        np.testing.assert_allclose(got[8], ref.bc[8], rtol=0, atol=5.0 * 1e-13)      # SINE: 1e-13 of the amplitude
        np.testing.assert_allclose(got[2], ref.bc[2], rtol=0, atol=1e-4 * 0.3)       # OU: 1e-4 sigma
        if k < K:
            es = ens.step(DT, n_steps=1)
            assert not es.status.any()
            ref.evaluate(es.time)
    st = ens.disturbance_state()
    off, filled = ens.disturbance_history()
    assert np.array_equal(st.n_eval, ref.st[:, DS_N_EVAL]) and np.array_equal(st.n_draw, ref.st[:, DS_N_DRAW])
    assert np.array_equal(filled, ref.n_filled()) and np.all(filled == K + 1)
    assert np.array_equal(st.value[:2], ref.st[:2, DS_VALUE]) and np.array_equal(off[:, :2], ref.hist[:, :2])
    assert not off[K + 1:].any()                          # entries not filled yet hold 0
    np.testing.assert_allclose(off[:, 2], ref.hist[:, 2], rtol=0, atol=5.0 * 1e-13)
    np.testing.assert_allclose(off[:, 3], ref.hist[:, 3], rtol=0, atol=1e-4 * 0.3)
    np.testing.assert_allclose(st.x[3], ref.st[3, DS_X], rtol=0, atol=1e-4 * 0.3)
    assert np.array_equal(st.t_prev, ens.state.time) and np.array_equal(st.base, wt.boundary_block(bc, N))
    ens.close()


def test_bit_exact_replay_through_a_schedule(gpu, wt):
    N, n, K = 96, 8, 60
    cols, bc = wt.make_ensemble(N, seed=23)
    a = _open(wt, cols, bc, n)
    a.set_disturbances(*_mixed(wt, N), seed=12, history=K)
    a.step(DT, n_steps=K, download=False)
    off, filled = a.disturbance_history()
    assert np.all(filled == K)
    params, base = wt.disturbance_block(N, *_mixed(wt, N)), a.disturbance_state().base
    sched = np.stack([compose_rows(params, base, off[k]) for k in range(K)])
    b = _open(wt, cols, bc, n)
    b.step(DT, n_steps=K, boundary_schedule=sched, download=False)
    sa, sb = a.state, b.state
    assert_all_equal((sa.pH, sa.chlorine, sa.temperature, sa.time, sa.status), (sb.pH, sb.chlorine, sb.temperature, sb.time, sb.status), "replay")
    assert not sa.status.any()
    assert np.unique(sched[:, 1], axis=0).shape[0] > 1    # the rows did move
    a.close(); b.close()


def test_schedule_independence(gpu, wt, monkeypatch):
    N, n, K = 160, 8, 70
    cols, bc = wt.make_ensemble(N, seed=61)
    chlorine, acid = pi_loops(wt, cols)
    prog = _mixed(wt, N, seed=8)

    def run(v):
        if v.get("tickets"):
            monkeypatch.setenv("WT_Q_TICKETS", "1")
        ens = plant(wt, cols, bc, n)
        ens.set_placement(v.get("adaptive", False))
        ens.set_schedule(v.get("streams", 0), v["chunk"])
        ens.write_commands(*MASTER)
        ens.enable_control(chlorine, acid)
        ens.set_disturbances(*prog, seed=5, history=K + 1)
        calls = v.get("calls", 1)
        for _ in range(calls):
            ens.step(DT, n_steps=K // calls, fused=v.get("fused", True), download=False)
        out = plant_state(ens) + ens.input_image() + (ens.control_state().block(),) + _dsts(ens)
        ens.close()
        monkeypatch.delenv("WT_Q_TICKETS", raising=False)
        return out

    ref = {c: run(dict(chunk=c)) for c in (1, 7, 50)}
    assert not ref[7][5].any()
    # every call closes with a scan, and fused=False scans every step: those runs are the scan-every-step run
    for v, want in ((dict(streams=3, chunk=7), 7), (dict(chunk=7, tickets=True), 7), (dict(chunk=1, adaptive=True, calls=5), 1),
                    (dict(chunk=7, calls=K), 1), (dict(chunk=50, fused=False), 1)):
        assert_all_equal(ref[want], run(v), v)
    # the disturbance itself does not depend on the scan interval (only its boundary rows 0 / 4 / 6 do)
    assert_all_equal(ref[1][-9:-1], ref[50][-9:-1], "offsets")


def test_sharding(gpu, wt):
    M, n, K = 48, 4, 40
    cols, bc = wt.make_ensemble(2 * M, seed=71)
    bcb = wt.boundary_block(bc, 2 * M)
    prog = _mixed(wt, 2 * M, seed=9)
    whole = _open(wt, cols, bc, n)
    whole.set_disturbances(*prog, seed=33, history=K + 1)
    whole.step(DT, n_steps=K, download=False)
    w_off, _ = whole.disturbance_history()
    w_st = whole.state
    for part in (0, 1):
        sl = slice(part * M, (part + 1) * M)
        sub_cols = {k: np.asarray(v)[sl] for k, v in cols.items()}
        ens = _open(wt, sub_cols, bcb[:, sl], n)
        sub = [wt.Disturbance(d.row, d.kind, *(np.broadcast_to(np.asarray(getattr(d, f), dtype=float), (2 * M,))[sl]
                                                for f in ("t_start", "t_end", "a", "b", "c"))) for d in prog]
        ens.set_disturbances(*sub, seed=33, reactor_base=part * M, history=K + 1)
        ens.step(DT, n_steps=K, download=False)
        off, _ = ens.disturbance_history()
        st = ens.state
        assert np.array_equal(off, w_off[:, :, sl])
        assert_all_equal((w_st.pH[sl], w_st.chlorine[sl], w_st.temperature[sl], w_st.time[sl]),
                         (st.pH, st.chlorine, st.temperature, st.time), part)
        ens.close()
    whole.close()


def test_ou_statistics(gpu, wt):
    N, n, K, tau, sigma, dt = 4096, 2, 400, 600.0, 0.2, 10.0
    cols, bc = wt.make_ensemble(N, seed=5)

    def run(seed):
        ens = _open(wt, cols, bc, n)
        ens.set_disturbances(wt.Disturbance.ou("inlet_temperature", sigma, tau), seed=seed, history=K + 1)
        ens.step(dt, n_steps=K, download=False)
        off = ens.disturbance_history()[0][:, 0]
        ens.close()
        return off

    x = run(1)
    # the stationary part: from x0 = 0 the variance is sigma^2 (1 - phi^(2k)); use k >= 200 (phi^400 < 1.3e-3)
    s = x[200:]
    phi = math.exp(-dt / tau)
    m, v = s.mean(), s.var()
    n_eff = N * len(s) * (1 - phi) / (1 + phi)        # effective sample size of an AR(1) series
    assert abs(m) < 5 * sigma / math.sqrt(n_eff)
    assert abs(v / sigma ** 2 - 1) < 5 * math.sqrt(2.0 / n_eff) + 2e-3
    rho = np.mean(s[1:] * s[:-1]) / np.mean(s * s)
    assert abs(rho - phi) < 5 * math.sqrt((1 - phi ** 2) / (N * len(s))) * 3
    assert np.array_equal(run(1), x)
    y = run(2)
    assert not np.array_equal(y, x) and abs(np.corrcoef(x[-1], y[-1])[0, 1]) < 0.1


def test_closed_loop_effect(gpu, wt):
    N, n, K = 64, 4, 300
    cols, bc = wt.make_ensemble(N, seed=45)
    chlorine, _ = pi_loops(wt, cols)
    res = []
    for disturbed in (False, True):
        ens = plant(wt, cols, bc, n)
        ens.set_schedule(0, 6)
        ens.write_commands(*MASTER)
        ens.enable_control(chlorine)
        if disturbed:
            ens.set_disturbances(wt.Disturbance.ou("inlet_chlorine", 0.5, 300.0), seed=3, history=K + 1)
        rows = []
        for _ in range(K // 30):
            ens.step(DT, n_steps=30, download=False)
            rows.append(ens.boundary())
        cs = ens.control_state().chlorine
        res.append((np.array(rows), cs.iae.copy(), cs.dose.copy()))
        ens.close()
    (r0, iae0, dose0), (r1, iae1, dose1) = res
    assert np.mean(iae1) > np.mean(iae0) and np.median(iae1) > np.median(iae0)
    # the dose follows the disturbance: more inlet chlorine, less dosing
    d_cl = r1[:, 2] - r0[:, 2]
    d_dose = r1[:, 6] - r0[:, 6]
    assert np.corrcoef(d_cl[2:].ravel(), d_dose[2:].ravel())[0, 1] < 0 and not np.array_equal(dose0, dose1)
    # rows 0 / 4 / 6 belong to the command path: the master's inlet and acid words, the loop's chlorine flow
    assert np.all(r1[:, 0] == MASTER[2]) and np.all(r1[:, 4] == MASTER[0]) and np.array_equal(r0[:, 0], r1[:, 0])


def test_errors_and_lifetime(gpu, wt):
    nat = gpu
    for nz in (33, 40):
        cols, bc = wt.make_ensemble(4, seed=1)
        ens = _open(wt, cols, bc, nz)
        with pytest.raises(ValueError, match="up to 32 zones"):
            ens.set_disturbances(wt.Disturbance.step(1, 0.1))
        ens.close()
    # before set_boundary (the ensemble sets the state at creation), and before set_state through the C ABI
    L = nat.lib()
    cols, bc = wt.make_ensemble(4, seed=2)
    ens = wt.ReactorEnsemble(cols, n_zones=4)
    with pytest.raises(ValueError, match="set_state and set_boundary must precede"):
        ens.set_disturbances(wt.Disturbance.step(1, 0.1))
    h = C.c_void_p()
    nat.check(L.wt_ensemble_create(4, 4, 0, nat.dptr(np.ascontiguousarray(ens.constants)), C.byref(h)))
    blk = np.ascontiguousarray(wt.disturbance_block(4, wt.Disturbance.step(1, 0.1)))
    assert L.wt_ensemble_disturb_set(h, nat.dptr(blk), 1, 0, 0) == nat.WT_E_STATE
    assert L.wt_ensemble_disturb_get(h, None, None, None) == nat.WT_E_STATE
    L.wt_ensemble_destroy(h)
    ens.close()

    N, n = 32, 4
    cols, bc = wt.make_ensemble(N, seed=3)
    base = wt.boundary_block(bc, N)
    ens = _open(wt, cols, bc, n)
    # a refused block gives wt_program_check's message
    bad = np.ascontiguousarray(wt.disturbance_block(N, wt.Disturbance.step(1, 0.1)))
    bad[0, 1] = 4.0
    with pytest.raises(ValueError):
        ens._program_call(nat.lib().wt_ensemble_disturb_set, nat.dptr(bad), C.c_uint64(1), 0, 0)
    assert refused_as_checked(nat, nat.WT_PROG_DISTURB, bad)
    with pytest.raises(ValueError, match="no disturbance program"):
        ens.disturbance_state()
    ens.set_disturbances(wt.Disturbance.step("inlet_temperature", 2.0), wt.Disturbance.ramp("inlet_pH", 1e-3))
    assert np.array_equal(ens.boundary()[3], base[3] + 2.0)
    sched = np.repeat(base[None], 3, axis=0)
    with pytest.raises(ValueError, match="disturbance program"):
        ens.step(DT, n_steps=3, boundary_schedule=sched)
    assert L.wt_ensemble_step_scheduled(ens._h, DT, 3, 1, nat.dptr(np.ascontiguousarray(sched))) == nat.WT_E_STATE
    assert "disturbance program" in L.wt_last_error().decode()
    ens.step(DT, n_steps=5)
    # set_boundary replaces the base and recomposes from the current offsets (no evaluation)
    nb = base.copy(); nb[3] += 1.0; nb[1] -= 0.5; nb[8] += 3.0
    ens.set_boundary(nb)
    st = ens.disturbance_state()
    assert np.array_equal(st.base, nb) and np.all(st.n_eval == 6)
    got = ens.boundary()
    assert np.array_equal(got[3], nb[3] + 2.0) and np.array_equal(got[1], clamp_row(1, nb[1] + st.value[1]))
    assert np.array_equal(got[8], nb[8])
    # set twice replaces: the old rows go back to the base first
    ens.set_disturbances(wt.Disturbance.step("ambient_temperature", -1.0))
    got = ens.boundary()
    assert np.array_equal(got[[1, 3]], nb[[1, 3]]) and np.array_equal(got[8], nb[8] - 1.0)
    assert np.array_equal(ens.disturbance_state().base, nb)
    # clear restores the base rows, and schedules work again
    ens.clear_disturbances()
    assert np.array_equal(ens.boundary(), nb)
    ens.step(DT, n_steps=3, boundary_schedule=sched)
    ens.close()


def test_frozen_reactors_get_no_evaluation(gpu, wt):
    from conftest import golden_json
    g = golden_json("g4_faults.json")["cold_run"]
    cfg = wt.ReactorConfiguration(**g["config"])
    b = wt.BoundaryConditions(**dict(zip(wt.params.BOUNDARY_FIELDS, g["bc"])))
    ens = wt.ReactorEnsemble([cfg, wt.ReactorConfiguration(n_zones=4)])
    ens.set_boundary([b, wt.BoundaryConditions()])
    ens.set_disturbances(wt.Disturbance.ou("inlet_pH", 0.1, 100.0), history=80)
    Kc = 60
    es = ens.step(1.0, n_steps=Kc)
    st = ens.disturbance_state()
    assert es.status[0] & 1 and es.time[0] < Kc and es.time[1] == Kc
    assert st.t_prev.tolist() == [es.time[0], Kc]
    assert st.n_eval[0].tolist() == [es.time[0] + 1, Kc + 1]
    ens.close()
    # a non-finite state: the reactor never steps
    N, n = 8, 4
    cols, bc = wt.make_ensemble(N, seed=6)
    ens = _open(wt, cols, bc, n)
    pH = np.full((N, n), 7.0); pH[3, 1] = np.nan
    ens.set_state(pH, 1.0, 20.0, 0.0)
    ens.set_disturbances(wt.Disturbance.ou("inlet_pH", 0.1, 100.0))
    ens.step(DT, n_steps=4, download=False)
    st = ens.disturbance_state()
    assert st.n_eval[0, 3] == 1 and np.all(np.delete(st.n_eval[0], 3) == 5) and st.n_draw[0, 3] == 0
    ens.close()
