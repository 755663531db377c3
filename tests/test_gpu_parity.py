"""Parity of the HIP path (through the C ABI) with the CPU oracle and with the
reference's golden vectors.  Tolerance: per-zone pH / Cl / T within 1e-6
relative of the reference CPU step (BASELINE.json north_star); observed
agreement is orders of magnitude tighter and is asserted at 1e-7 for the
golden trajectories and 1e-8 against the oracle on the bench ensemble."""
import sys

import numpy as np
import pytest

from conftest import SCENARIOS, cfg_columns, golden_json, golden_npz, relerr
from program_helpers import both_packings, packing  # noqa: F401  (a fixture)

pytestmark = pytest.mark.gpu

TOL = 1e-6  # stated fp64 tolerance of the north star


def _ens_from_golden(wt, g, n):
    cols = cfg_columns(g["cfg"], g["cfg_fields"])
    return wt.ReactorEnsemble(cols, n_zones=n), cols


def _initial(cols, S, n):
    shape = (S, n)
    return (np.broadcast_to(np.asarray(cols["initial_pH"], dtype=float)[:, None], shape).copy(),
            np.broadcast_to(np.asarray(cols["initial_chlorine"], dtype=float)[:, None], shape).copy(),
            np.broadcast_to(np.asarray(cols["temperature"], dtype=float)[:, None], shape).copy())


@pytest.mark.parametrize("n", [4, 8, 20])
def test_rhs_vs_reference_and_oracle(gpu, wt, oracle, n):
    g = golden_npz(f"g2_rhs_n{n}.npz")
    ens, cols = _ens_from_golden(wt, g, n)
    ens.set_boundary(np.ascontiguousarray(g["bc"].T))
    y = g["y"]
    dpH, dCl, dT, fl = ens.derivatives(y[:, :n], y[:, n:2 * n], y[:, 2 * n:])
    assert not fl.any()
    f = np.concatenate([dpH, dCl, dT], axis=1)
    ref = g["f"]
    par = ens.constants
    for c in range(y.shape[0]):
        fo, _ = oracle.rhs(n, par[:, c], g["bc"][c], y[c])
        K = par[wt.params.P_KEX, c]
        H = 10.0 ** (-y[c][:n])
        mag = np.concatenate([np.abs(ref[c][:n]) + 4 * K * H.max() / 1e-4,
                              np.abs(ref[c][n:2 * n]) + 4 * K * np.abs(y[c][n:2 * n]).max() + 1e-300,
                              np.abs(ref[c][2 * n:]) + 4 * K * np.abs(y[c][2 * n:]).max()])
        assert np.all(np.abs(f[c] - ref[c]) <= 2e-12 * mag), f"case {c} vs reference"
        assert np.all(np.abs(f[c] - fo) <= 2e-12 * mag), f"case {c} vs oracle"
    # temperature rows are pure arithmetic (stencil in dgemv order + inlet): bit-identical to the reference where
    # there is no heat loss (the kernel multiplies by a precomputed U A / (rho cp V), the reference divides)
    no_loss = g["bc"][:, 9] == 0
    assert no_loss.sum() > 50 and np.array_equal(dT[no_loss], ref[no_loss, 2 * n:])
    ens.close()


def test_rhs_flags_temperature_range(gpu, wt):
    ens = wt.ReactorEnsemble([wt.ReactorConfiguration(n_zones=4) for _ in range(3)])
    ens.set_boundary(wt.BoundaryConditions())
    T = np.full((3, 4), 20.0); T[1, 2] = 100.5; T[2, 0] = -0.1
    _, _, _, fl = ens.derivatives(np.full((3, 4), 7.0), np.full((3, 4), 2.0), T)
    assert list(fl) == [0, 1, 1]
    r = wt.IntegratedCSTR(wt.ReactorConfiguration(n_zones=4))
    with pytest.raises(ValueError, match="outside liquid water range"):
        r.derivatives(0.0, np.concatenate([np.full(4, 7.0), np.full(4, 2.0), [20, 20, 101, 20]]), wt.BoundaryConditions())
    ens.close()


@pytest.mark.parametrize("n", [4, 8, 20])
@pytest.mark.parametrize("scen", SCENARIOS)
def test_dropin_trajectory_vs_reference(gpu, wt, n, scen):
    """IntegratedCSTR.step() (one-reactor drop-in) step by step against the
    reference trajectory, including scipy's decision counters on every step."""
    g = golden_npz(f"g3_traj_{scen}_n{n}.npz")
    fields = [str(x) for x in g["cfg_fields"]]
    kw = {k: (bool(v) if k == "enable_thermal_stratification" else (int(v) if k == "n_zones" else float(v)))
          for k, v in zip(fields, g["cfg"])}
    r = wt.IntegratedCSTR(wt.ReactorConfiguration(**kw))
    b = wt.BoundaryConditions(**{k: float(v) for k, v in zip(wt.params.BOUNDARY_FIELDS, g["bc"])})
    dt = float(g["dt"])
    traj, stats = g["traj"], g["stats"]
    nst = min(traj.shape[0] - 1, 250)
    worst = np.zeros(3)
    mismatched = 0
    prev = r.state
    for k in range(nst):
        s = r.step(dt, b)
        assert s is prev                                         # same mutable object (reactor.py:509)
        got = np.stack([s.pH, s.chlorine, s.temperature])
        worst = np.maximum(worst, np.max(np.abs(got - traj[k + 1]) / np.abs(traj[k + 1]), axis=1))
        st = r._ens.solver_stats()[0]
        mismatched += int(tuple(st[:4]) != tuple(stats[k][:4]))
        assert abs(s.time - g["time"][k]) < 1e-9 and s.flow_rate == g["flow"][k]
        der = np.stack([s.H_concentration, s.density, s.chlorine_decay_rate])
        assert relerr(der, g["derived"][k]) < TOL
    assert np.all(worst < 1e-7), worst
    assert mismatched == 0, f"{mismatched} of {nst} steps took a different solver decision sequence"


@pytest.mark.parametrize("n", [4, 8, 20])
def test_synthetic_sample_vs_reference(gpu, wt, n):
    """First 64 reactors of the bench ensemble, 50 steps, against the reference."""
    g = golden_npz(f"g6_ensemble_n{n}.npz")
    S, steps, every = int(g["n_reactors"]), int(g["steps"]), int(g["every"])
    cols, bc = wt.make_ensemble(S)
    ens = wt.ReactorEnsemble(cols, n_zones=n)
    ens.set_boundary(bc)
    for k in range(steps // every):
        es = ens.step(1.0, n_steps=every, fused=(k % 2 == 0))
        snap = g["snaps"][k]
        assert not es.status.any()
        assert relerr(es.pH, snap[:, 0]) < 1e-7
        assert relerr(es.chlorine, snap[:, 1]) < 1e-7
        assert relerr(es.temperature, snap[:, 2]) < 1e-7
    # decision counters of the last step
    st = ens.solver_stats()
    assert np.array_equal(st[:, :4], g["stats"][:, steps - 1, :4])
    ens.close()


@pytest.mark.parametrize("n,N", [(4, 10000), (8, 10000), (8, 12500), (20, 10000)])
def test_full_size_ensemble_vs_oracle(gpu, wt, oracle, n, N):
    """BASELINE configs 2-4 at full size (12 500 x 8 is config 4's per-GPU share of 100 000): every reactor,
    every zone against the oracle after 8 steps, plus size-independent properties: schedule invariance
    (work-queue launch == per-step scans == round-1 stream launches, bitwise), and independence of a
    reactor from its neighbours in the wavefront.  The reactors on which the solver's step sequence is
    sensitive to rounding are pinned against the reference itself in test_outlier_reactors_vs_reference."""
    cols, bc = wt.make_ensemble(N)
    ens = wt.ReactorEnsemble(cols, n_zones=n)
    ens.set_boundary(bc)
    st0 = ens.state
    steps = 8
    es = ens.step(1.0, n_steps=steps, fused=True)
    pH, Cl, T, t, ost = oracle.ensemble_step(n, ens.constants, bc, 1.0, steps, st0.pH, st0.chlorine,
                                             st0.temperature, st0.time, nthreads=16)
    assert np.array_equal(es.status != 0, ost != 0)
    ok = ost == 0
    err = np.stack([np.abs(es.pH - pH) / np.abs(pH), np.abs(es.chlorine - Cl) / np.abs(Cl),
                    np.abs(es.temperature - T) / np.abs(T)])[:, ok]
    # North-star tolerance 1e-6.  A reactor whose solve crosses a stratification flip with repeated
    # rejections is chaotic at the 1-ulp level (two CPU executions of the same
    # algorithm drift apart by up to 3e-6 there), so the bound is asserted on all but 1e-5 of the
    # samples and the solver's own tolerance bounds the rest.
    assert np.mean(err < TOL) > 1 - 1e-5
    assert err.max() < 1e-5
    # report-style tight bound: all but a handful of (reactor, zone) samples agree to 1e-9
    assert np.mean(err < 1e-9) > 0.999
    assert np.allclose(es.time[ok], steps * 1.0)
    # stepwise launches of the stream schedule give bitwise the same answer as the work-queue launch
    ens.set_state(st0.pH, st0.chlorine, st0.temperature, st0.time)
    ens.set_schedule(3, 1)
    es2 = ens.step(1.0, n_steps=steps, fused=False)
    for a, b in ((es.pH, es2.pH), (es.chlorine, es2.chlorine), (es.temperature, es2.temperature),
                 (es.H_concentration, es2.H_concentration), (es.density, es2.density),
                 (es.chlorine_decay_rate, es2.chlorine_decay_rate)):
        assert np.array_equal(a, b)
    ens.close()
    # a reactor's result does not depend on which reactors share its wavefront
    perm = np.random.default_rng(7).permutation(N)[:2000]
    sub_cols = {k: v[perm] for k, v in cols.items()}
    ens_p = wt.ReactorEnsemble(sub_cols, n_zones=n)
    ens_p.set_boundary(np.ascontiguousarray(bc[:, perm]))
    esp = ens_p.step(1.0, n_steps=steps, fused=True)
    assert np.array_equal(esp.pH, es.pH[perm]) and np.array_equal(esp.chlorine, es.chlorine[perm])
    assert np.array_equal(esp.temperature, es.temperature[perm])
    ens_p.close()


@pytest.mark.parametrize("n", [4, 8, 20])
def test_results_do_not_depend_on_the_launch_schedule(gpu, wt, n):
    """Reactor ranges / streams, steps per launch and the wavefront rendez-vous are throughput
    knobs: every combination gives bitwise the same state, status and solver counters."""
    N, steps = 3000, 12
    cols, bc = wt.make_ensemble(N, seed=4242)
    ref = None
    for streams, chunk, sync in ((0, 50, True), (1, 0, True), (0, 1, True), (1, 1, False), (4, 5, True), (3, 7, False), (8, 25, True), (0, 7, True)):
        ens = wt.ReactorEnsemble(cols, n_zones=n)
        ens.set_boundary(bc)
        ens.set_schedule(streams, chunk)
        ens.set_sync(sync)
        es = ens.step(1.0, n_steps=steps)
        got = (es.pH, es.chlorine, es.temperature, es.time, es.status, es.H_concentration, es.density,
               es.chlorine_decay_rate, ens.solver_stats())
        if ref is None:
            ref = got
        else:
            for a, b in zip(ref, got):
                assert np.array_equal(a, b), (streams, chunk, sync)
        ens.close()


@pytest.mark.parametrize("n", [4, 8, 20])
def test_placement_changes_no_bit(gpu, wt, n):
    """Reactors of similar solver cost are dealt into the same wavefronts (wt_place.hpp) once 32 outer steps of
    counters are in.  The slot table is then a permutation in order of cost, and state, status, solver counters,
    sensor readings, register images and the commanded boundary are those of the fixed placement, bit for bit."""
    N, calls, steps = 3000, 3, 40
    cols, bc = wt.make_ensemble(N, seed=2024)
    def run(adaptive):
        ens = wt.ReactorEnsemble(cols, n_zones=n); ens.set_boundary(bc)
        ens.set_placement(adaptive)
        ens.enable_sensors(seed=9); ens.enable_plant_io()
        ens.write_commands(bc[4], bc[6], bc[0])             # the masters' setpoints = the synthetic boundary (as float32)
        cost = np.zeros(N)
        for c in range(calls):
            es = ens.step(1.0, n_steps=steps)
            if c == 0:
                first_call_perm = ens.placement()[1].copy()
        for k in range(8):
            es = ens.step(1.0, n_steps=1); cost += ens.solver_stats()[:, 0]
        mode, perm = ens.placement()
        ens.set_schedule(3, 4)                               # the stream schedule walks the same slot table
        es = ens.step(1.0, n_steps=9)
        out = (es.pH, es.chlorine, es.temperature, es.time, es.status, es.H_concentration, es.density, es.chlorine_decay_rate,
               ens.solver_stats(), *ens.sensor_readings(), *ens.input_image(), ens.boundary())
        ens.close()
        return out, mode, perm, first_call_perm, cost
    ref, mode0, perm0, _, _ = run(False)
    got, mode1, perm1, first, cost = run(True)
    assert mode0 is False and np.array_equal(perm0, np.arange(N))
    assert mode1 is True and np.array_equal(first, np.arange(N))            # nothing to go by during the first call
    assert np.array_equal(np.sort(perm1), np.arange(N)) and not np.array_equal(perm1, np.arange(N))
    # the table is in order of the cost history it was dealt from; the costs persist, so later costs follow it closely
    ordered = cost[perm1]
    assert np.corrcoef(np.arange(N), ordered)[0, 1] > 0.5
    R = 64 // n
    m = (N // R) * R
    assert ordered[:m].reshape(-1, R).max(1).sum() < 0.97 * cost[:m].reshape(-1, R).max(1).sum()
    for a_, b_ in zip(ref, got):
        assert np.array_equal(a_, b_, equal_nan=True)


def _mixed_columns(wt, mask, a, b):
    """Configuration columns that are `a`'s where `mask` is set and `b`'s elsewhere; a column one side does not name
    has ReactorConfiguration's default there."""
    defaults = wt.ReactorConfiguration()
    side = lambda cols, k: np.broadcast_to(np.asarray(cols.get(k, getattr(defaults, k))), mask.shape)
    return {k: np.where(mask, side(a, k), side(b, k)) for k in sorted(set(a) | set(b))}


@both_packings("n", [5, 8, 12, 20, 40], packed=[5, 8, 12, 20])
def test_solve_fast_paths_change_no_bit(gpu, wt, monkeypatch, packing, n):
    """A wavefront none of whose Jacobians couples a row to a neighbour's temperature skips those terms in every solve,
    and at the row-straddling zone counts solves the T and the pH system in lock step (wt_pcr.hpp: jac_t_dense,
    pcr_rc_pair).  Which path a reactor takes depends on the other reactors of its wavefront, so the paths must agree
    bit for bit: WT_DENSE_COUPLING sends every solve down the general path, and state, status and solver counters are
    those of the default run.

    Spread: 1500 benign reactors (300 at n = 40), which the library deals two to a wavefront on an MI355X where twelve
    fit at n = 5.  Packed: five full wavefronts under the identity placement, the even slots of each from
    _random_edge_ensemble -- reactors at stratification switches, where jac_t_dense fires -- and the odd slots from
    make_ensemble, an attempt limit of 300 on both runs as in test_edge_configurations_vs_oracle.  Nothing the host can
    read records which solves took the general path in the default run (and the kernel gets no counter for it): that the
    packed wavefronts mix the paths rests on the population, not on an assertion."""
    if packing.packed:
        R = 64 // n
        N = 5 * R
        edge = (np.arange(N) % R) % 2 == 0
        ecols, ebc = _random_edge_ensemble(wt, N, seed=7700 + n)
        bcols, bbc = wt.make_ensemble(N, seed=77)
        cols, bc = _mixed_columns(wt, edge, ecols, bcols), np.ascontiguousarray(np.where(edge, ebc, bbc))
    else:
        N = 1500 if n <= 20 else 300
        cols, bc = wt.make_ensemble(N, seed=77)
    def run(dense):
        if dense:
            monkeypatch.setenv("WT_DENSE_COUPLING", "1")
        else:
            monkeypatch.delenv("WT_DENSE_COUPLING", raising=False)
        ens = packing.place(wt.ReactorEnsemble(cols, n_zones=n)); ens.set_boundary(bc)       # (the knob is read at creation)
        if packing.packed:
            ens.set_step_limit(300)
        es = ens.step(1.0, n_steps=25)
        out = (es.pH, es.chlorine, es.temperature, es.time, es.status, ens.solver_stats())
        packing.check(ens)
        ens.close()
        return out
    fast, general = run(False), run(True)
    for a, b in zip(fast, general):
        assert np.array_equal(a, b, equal_nan=True)


def test_very_long_calls_are_split_without_a_trace(gpu, wt, monkeypatch):
    """The queue's tickets are 32-bit: a call that would need more than 2^30 of them is cut into several launches
    (wtphys.hip).  With the ticket budget turned down (WT_Q_TICKETS, test knob, read when the ensemble is created) a
    23-step call becomes eight queue launches of one 3-step item per group: state, counters, sensor readings, register
    images and the commanded boundary equal, bit for bit, those of the single plain launch that an ensemble with a
    worker per group gets (88 wavefront-groups here)."""
    N, n, steps = 700, 8, 23
    cols, bc = wt.make_ensemble(N, seed=77)
    def run(item):
        ens = wt.ReactorEnsemble(cols, n_zones=n); ens.set_boundary(bc)
        ens.set_schedule(0, 5)
        ens.enable_sensors(seed=5); ens.enable_plant_io()
        ens.write_commands(0.1, 0.05, cols["flow_rate"] * 1.1)
        assert ens.item_steps(steps) == item
        es = ens.step(1.0, n_steps=steps)
        out = (es.pH, es.chlorine, es.temperature, es.time, es.status, ens.solver_stats(), *ens.sensor_readings(), *ens.input_image(), ens.boundary())
        ens.close()
        return out
    ref = run(steps)
    monkeypatch.setenv("WT_Q_TICKETS", "1")                       # fewer tickets than groups: one item per group and launch
    got = run(3)
    for a, b in zip(ref, got):
        assert np.array_equal(a, b, equal_nan=True)


def test_device_export_and_rccl_gather(gpu):
    """The multi-GPU path's device side on one card: wt_ensemble_export_state_device writes the (3, N, n) fp64 block
    straight into a torch tensor, and gather_state runs the RCCL all_gather (world of one rank) on it.  In a process
    of its own, torch first: torch brings its own HIP runtime, which must be the first one up (as in bench.py)."""
    import os, subprocess
    r = subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), "gpu_export_gather.py")],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "export and gather ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


def test_plain_c_client_equals_the_python_host(gpu, wt, tmp_path):
    """tests/c_abi/abi_client.c (C99, gcc) drives create / set_state / set_boundary / step / get_state through
    include/wtphys.h in its own process: same bits as the ctypes host."""
    import subprocess
    from test_host_api import _build_c_client
    exe = _build_c_client(tmp_path)
    N, n, steps, dt = 500, 8, 7, 1.0
    cols, bc = wt.make_ensemble(N, seed=31)
    ens = wt.ReactorEnsemble(cols, n_zones=n); ens.set_boundary(bc)
    s0 = ens.state
    req, rep = tmp_path / "req.bin", tmp_path / "rep.bin"
    with open(req, "wb") as f:
        np.array([N, n, steps], dtype=np.int64).tofile(f); np.array([dt]).tofile(f)
        for arr in (ens.constants, bc, s0.pH, s0.chlorine, s0.temperature):
            np.ascontiguousarray(arr, dtype=np.float64).tofile(f)
    r = subprocess.run([exe, str(req), str(rep)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    out = np.fromfile(rep, dtype=np.float64)
    es = ens.step(dt, n_steps=steps)
    k = N * n
    assert np.array_equal(out[:k].reshape(N, n), es.pH) and np.array_equal(out[k:2 * k].reshape(N, n), es.chlorine)
    assert np.array_equal(out[2 * k:3 * k].reshape(N, n), es.temperature)
    assert np.array_equal(out[3 * k:3 * k + N], es.time) and np.array_equal(out[3 * k + N:], es.status.astype(np.float64))
    ens.close()


_RAGGED = [(2, 5), (3, 33), (5, 1), (7, 100), (16, 9), (31, 4), (64, 3)]
_RAGGED_ORACLE = {}


@both_packings("n,N", _RAGGED, packed=[(n, N) for n, N in _RAGGED if n <= 32])
def test_ragged_shapes_vs_oracle(gpu, wt, oracle, packing, n, N):
    """Zone counts that do not divide 64, a single reactor, the 64-zone maximum.  Spread, these ensembles run one
    reactor per wavefront; packed (n <= 32), wavefronts that are part full, with idle lanes behind the last segment
    where n does not divide 64.  The oracle's result is computed once per shape."""
    cols, bc = wt.make_ensemble(N, seed=99)
    ens = packing.place(wt.ReactorEnsemble(cols, n_zones=n))
    ens.set_boundary(bc)
    st0 = ens.state
    es = ens.step(1.0, n_steps=5)
    if (n, N) not in _RAGGED_ORACLE:
        _RAGGED_ORACLE[n, N] = oracle.ensemble_step(n, ens.constants, bc, 1.0, 5, st0.pH, st0.chlorine, st0.temperature,
                                                    st0.time, nthreads=4)
    pH, Cl, T, t, ost = _RAGGED_ORACLE[n, N]
    assert np.array_equal(es.status, ost.astype(np.uint32))
    assert relerr(es.pH, pH) < 1e-7 and relerr(es.chlorine, Cl) < 1e-7 and relerr(es.temperature, T) < 1e-7
    packing.check(ens)
    ens.close()


def test_zone_count_limits(gpu, wt):
    with pytest.raises(ValueError, match="at least 2 zones"):
        wt.ReactorEnsemble({"volume": np.array([1000.0])}, n_zones=1)
    native = gpu
    with pytest.raises(native.WtError):
        wt.ReactorEnsemble({"volume": np.array([1000.0])}, n_zones=65)


def test_cold_run_freezes_like_reference(gpu, wt):
    """A reactor cooled below 0 degC: the reference raises ValueError out of step()
    at a known step index and leaves the state untouched."""
    g = golden_json("g4_faults.json")["cold_run"]
    cfg = wt.ReactorConfiguration(**g["config"])
    b = wt.BoundaryConditions(**dict(zip(wt.params.BOUNDARY_FIELDS, g["bc"])))
    r = wt.IntegratedCSTR(cfg)
    for k in range(200):
        try:
            s = r.step(1.0, b)
        except ValueError as e:
            assert "outside liquid water range" in str(e)
            assert k == g["raise_step_index"]
            # the text names the temperature the reference's message names (thermodynamics.py:151)
            head, tail = str(e).split("°C", 1)
            rhead, rtail = g["message"].split("°C", 1)
            assert tail == rtail and head.startswith("Temperature ")
            assert abs(float(head.split()[1]) - float(rhead.split()[1])) < 1e-8
            got = np.concatenate([r.state.pH, r.state.chlorine, r.state.temperature])
            assert relerr(got, np.concatenate(g["state_before_raise"])) < 1e-9
            assert r.state.time == g["time_before_raise"]
            break
    else:
        pytest.fail("no ValueError")
    # ensemble semantics: the flagged reactor is frozen, its neighbours keep stepping
    ens = wt.ReactorEnsemble([cfg, wt.ReactorConfiguration(n_zones=4)])
    ens.set_boundary([b, wt.BoundaryConditions()])
    es = ens.step(1.0, n_steps=60)
    assert es.status[0] & 1 and es.status[1] == 0
    assert es.time[0] == g["raise_step_index"] and es.time[1] == 60.0
    ens.close()


def test_batch_mode_construction_quirk(gpu, wt):
    assert golden_json("g4_faults.json")["batch_construction"] == "TypeError"
    with pytest.raises(TypeError):
        wt.IntegratedCSTR(wt.ReactorConfiguration(flow_rate=0.0))


def test_clamps_and_host_state_edits(gpu, wt, oracle):
    """State edited between steps is honoured (reactor.py:467-469); negative chlorine is
    clipped after the derived quantities are taken (reactor.py:503-507,534-536)."""
    cfg = wt.ReactorConfiguration(n_zones=4)
    b = wt.BoundaryConditions(inlet_chlorine=0.0)
    bv = np.array([getattr(b, k) for k in wt.params.BOUNDARY_FIELDS])
    r = wt.IntegratedCSTR(cfg)
    r.step(1.0, b)
    T1 = r.state.temperature.copy()
    # the host overwrites part of the state: zone 3 gets a chlorine value that decays below zero
    r.state.chlorine = np.array([2.0, 2.0, 2.0, -1e-3])
    r.state.pH = np.array([7.0, 7.1, 7.2, 7.3])
    s = r.step(1.0, b)
    par = r._ens.constants[:, 0]
    y0 = np.concatenate([[7.0, 7.1, 7.2, 7.3], [2.0, 2.0, 2.0, -1e-3], T1])
    yo, to, der, status = oracle.step(4, par, bv, 1.0, y0, 1.0)
    assert s.time == 2.0 == to
    got = np.concatenate([s.pH, s.chlorine, s.temperature])
    # Radau's own tolerances (rtol 1e-6, atol 1e-8) bound what "the same solve" means here
    assert np.all(np.abs(got - yo) <= 1e-6 * np.abs(yo) + 1e-8)
    assert int(r._ens.status()[0]) == status
    assert np.all(s.chlorine >= 0)
    # clamp flag: force a negative result (large negative chlorine everywhere, no inlet)
    ens = wt.ReactorEnsemble([cfg])
    ens.set_boundary(b)
    ens.set_state(np.full((1, 4), 7.0), np.full((1, 4), -0.5), np.full((1, 4), 20.0), np.array([0.0]))
    es = ens.step(1.0)
    yo, to, der, status = oracle.step(4, par, bv, 1.0, np.concatenate([np.full(4, 7.0), np.full(4, -0.5), np.full(4, 20.0)]), 0.0)
    assert status & oracle.ST_CLAMP_CL and int(es.status[0]) == status
    assert np.all(es.chlorine == 0.0) and np.all(yo[4:8] == 0.0)
    assert relerr(es.pH[0], yo[:4]) < 1e-9 and relerr(es.temperature[0], yo[8:]) < 1e-9
    ens.close()


def test_step_argument_errors(gpu, wt):
    ens = wt.ReactorEnsemble([wt.ReactorConfiguration(n_zones=4)])
    with pytest.raises(ValueError, match="boundary"):
        ens.step(1.0)
    ens.set_boundary(wt.BoundaryConditions())
    with pytest.raises(ValueError, match="max_step"):
        ens.step(0.0)
    with pytest.raises(ValueError, match="max_step"):
        ens.step(-1.0)
    ens.close()


def test_ph_solver_vs_reference(gpu, wt, oracle):
    g = golden_json("g5_ph_solver.json")
    cases = g["cases"]
    alk = np.array([c["alkalinity"] for c in cases]); ct = np.array([c["total_carbonate"] for c in cases])
    T = np.array([c["temperature"] for c in cases]); guess = np.array([c["guess"] for c in cases])
    pH, it, rc = wt.solve_pH(alk, ct, T, guess)
    for i, c in enumerate(cases):
        if c["rc"] == 0:
            assert rc[i] == 0 and abs(pH[i] - c["pH"]) < 1e-9, c
        else:
            assert rc[i] != 0
    chem = wt.AqueousChemistry(wt.BufferSystem(100.0, 2.0, 20.0))
    pH_eq = chem.calculate_pH()
    assert abs(pH_eq - g["pH_eq_default"]) < 1e-9
    assert abs(chem.add_acid(1000, 0.001, pH_eq) - g["add_acid_1000L_0p001mol"]) < 1e-9
    assert abs(chem.add_base(1000, 0.001, pH_eq) - g["add_base_1000L_0p001mol"]) < 1e-9
    # large batch against the oracle, including guesses that converge to different roots
    rng = np.random.default_rng(5)
    M = 20000
    alk, ct, T, guess = rng.uniform(50, 200, M), rng.uniform(1, 4, M), rng.uniform(5, 35, M), rng.uniform(2, 12, M)
    pH, it, rc = wt.solve_pH(alk, ct, T, guess)
    P = wt.params
    Kw = P.water_ionization_constant(T); Ka1 = P._pow10_neg(P.carbonate_pKa(T, 1)); Ka2 = P._pow10_neg(P.carbonate_pKa(T, 2))
    checked = 0
    for i in range(0, M, 97):
        po, ito, rco = oracle.calculate_pH(Kw[i], Ka1[i], Ka2[i], ct[i] / 1000.0, alk[i], guess[i])
        if rco == 0 and ito <= 12:
            # regular Newton path: same root, same iteration count
            assert rc[i] == 0 and it[i] == ito and abs(pH[i] - po) < 1e-9
            checked += 1
        elif rc[i] == 0:
            # the iteration is chaotic for this guess (f is non-monotone and the update is clipped
            # to [0,14]; the oracle itself needs > 12 iterations or fails): a 1-ulp difference picks
            # another path, so only require that what the GPU returns is a root of the charge balance
            H = 10.0 ** (-pH[i])
            D = H * H + Ka1[i] * H + Ka1[i] * Ka2[i]
            f = H - Kw[i] / H + (Ka1[i] * H / D + 2 * Ka1[i] * Ka2[i] / D) * ct[i] / 1000.0 - alk[i] / 50000.0
            assert abs(f) < 1e-8
    assert checked > 150


@pytest.mark.parametrize("n", [2, 3, 4, 5, 7, 8, 16, 20, 33, 64])
def test_cross_lane_primitives(gpu, n):
    """DPP row/wave shifts and the segment reduction agree with ds_bpermute on this GPU."""
    import ctypes as C
    m = C.c_int(-1)
    gpu.check(gpu.lib().wt_selftest_shuffles(0, n, C.byref(m)))
    assert m.value == 0


def _random_edge_ensemble(wt, N, seed):
    """Configurations and boundaries that sit on the branches of the RHS: no inlet flow, flow too
    small for a Richardson number (u <= 1e-6 -> Ri = inf), stratification off, temperatures around
    the 8 degC density branch and near the [0, 100] limits, extreme pH, dosing on/off."""
    rng = np.random.default_rng(seed)
    pick = lambda vals, p=None: rng.choice(vals, size=N, p=p)
    cols = {
        "initial_pH": pick([4.0, 6.0, 7.0, 8.3, 10.5]) + rng.uniform(-0.3, 0.3, N),
        "initial_chlorine": pick([0.0, 0.05, 2.0, 9.5]),
        "temperature": pick([0.5, 7.9, 8.1, 20.0, 39.5]),
        "flow_rate": pick([1e-4, 0.5, 5.0, 50.0]),
        "alkalinity": rng.uniform(20, 300, N),
        "total_carbonate": rng.uniform(0.2, 6, N),
        "enable_thermal_stratification": rng.random(N) < 0.8,
        "impeller_speed": pick([10.0, 60.0, 200.0]),
    }
    bc = np.empty((wt.params.NB, N))
    bc[0] = pick([0.0, 0.05, 5.0, 20.0]); bc[1] = rng.uniform(5.5, 9.5, N); bc[2] = pick([0.0, 1.0, 5.0])
    bc[3] = np.clip(cols["temperature"] + rng.uniform(-8, 8, N), 0.2, 60.0)
    bc[4] = pick([0.0, 0.5, 2.0]); bc[5] = 0.1; bc[6] = pick([0.0, 1.0]); bc[7] = 50.0
    bc[8] = rng.uniform(0, 30, N); bc[9] = pick([0.0, 5.0, 200.0])
    return cols, np.ascontiguousarray(bc)


_EDGE_ORACLE = {}


@both_packings("n,dt,steps", [(4, 1.0, 6), (8, 0.1, 6), (5, 10.0, 4), (8, 30.0, 3), (20, 100.0, 2)])
def test_edge_configurations_vs_oracle(gpu, wt, oracle, packing, n, dt, steps):
    """1500 reactors on the branches of the RHS against the oracle.  Spread, the library deals them two to a wavefront
    on an MI355X; packed, 64 // n under the identity placement, so a reactor that freezes, clamps or runs into the
    attempt limit does so beside up to fifteen that go on.  Same population, same bounds; the oracle's result is computed
    once per case."""
    N = 1500
    cols, bc = _random_edge_ensemble(wt, N, seed=1000 * n + int(dt * 10))
    ens = packing.place(wt.ReactorEnsemble(cols, n_zones=n))
    ens.set_boundary(bc)
    # some of these reactors slide along the 8 degC density jump: scipy's Radau then needs millions of
    # internal steps per outer step (hours in the reference); both sides stop after 300 attempts
    ens.set_step_limit(300)
    s0 = ens.state
    es = ens.step(dt, n_steps=steps)
    packing.check(ens)
    if (n, dt, steps) not in _EDGE_ORACLE:
        oracle.set_step_limit(300)
        try:
            _EDGE_ORACLE[n, dt, steps] = oracle.ensemble_step(n, ens.constants, bc, dt, steps, s0.pH, s0.chlorine,
                                                              s0.temperature, s0.time, nthreads=16)
        finally:
            oracle.set_step_limit(0)
    pH, Cl, T, t, ost = _EDGE_ORACLE[n, dt, steps]
    # same reactors freeze / clamp (temperature range, negative chlorine, ...); a reactor that hits the
    # attempt limit on one side is chaotic by construction and may just make it on the other
    lim = ((es.status | ost.astype(np.uint32)) & 128) != 0
    assert np.array_equal(es.status[~lim], ost.astype(np.uint32)[~lim])
    assert np.mean(lim) < 0.05
    assert np.array_equal(es.time[~lim], t[~lim])
    ok = ((ost & (oracle.ST_NONFINITE | oracle.ST_SOLVER_FAILED)) == 0) & ~lim
    got = np.stack([es.pH, es.chlorine, es.temperature])[:, ok]
    ref = np.stack([pH, Cl, T])[:, ok]
    # In units of Radau's own local tolerance (rtol 1e-6, atol 1e-8): 99.9 % of the samples agree to
    # better than one unit.  The rest belongs to reactors sliding along a discontinuity of the RHS,
    # where the step sequence is chaotic and errors of two correct executions accumulate over
    # hundreds of internal steps (observed: up to ~20 units); they stay far from anything physical.
    units = np.abs(got - ref) / (1e-6 * np.abs(ref) + 1e-8)
    assert np.percentile(units, 99.9) < 1.0
    assert units.max() < 200.0
    rel = np.abs(got - ref) / np.maximum(np.abs(ref), 1e-30)
    big = ref != 0
    assert np.mean(rel[big] < TOL) > 0.998   # adversarial ensemble: many reactors sit on a discontinuity
    ens.close()


@both_packings("n", [8], packed=[8, 5, 12, 20, 31])
def test_nonfinite_state_is_contained(gpu, wt, oracle, packing, n):
    """A reactor whose state is NaN / inf must not disturb the reactors sharing its wavefront, and ends like the
    reference: scipy's solve_ivp refuses the state (ValueError out of step(), tests/golden/g11_branches.json), so
    the reactor does not advance.

    Spread (n = 8, 24 reactors, a NaN in one zone of reactor 9 and an all-inf reactor 17) nobody shares a wavefront
    with anybody on an MI355X.  Packed, identity placement, N = 3 R + 1: an all-NaN reactor in the first slot of
    group 0, an all-inf one in the last slot of group 1 and one with a NaN in a single zone in a middle slot of group
    2, at n = 8 and at one zone count per level whose segments do not fill DPP rows (5, 12, 20, 31), where a lane reads
    its neighbours' values through the LDS exchange row.  The clean twin has the run's packing."""
    if packing.packed:
        R = 64 // n
        N = 3 * R + 1
        nan_all, inf_all, nan_one = 0, 2 * R - 1, 2 * R + R // 2
    else:
        N, nan_all, inf_all, nan_one = 24, None, 17, 9
    bad = [r for r in (nan_all, inf_all, nan_one) if r is not None]
    cols, bc = wt.make_ensemble(N, seed=5)
    ens = packing.place(wt.ReactorEnsemble(cols, n_zones=n))
    ens.set_boundary(bc)
    s0 = ens.state
    pH0 = s0.pH.copy(); pH0[nan_one, 3 % n] = np.nan; pH0[inf_all, :] = np.inf
    if nan_all is not None:
        pH0[nan_all, :] = np.nan
    ens.set_state(pH0, s0.chlorine, s0.temperature, s0.time)
    es = ens.step(1.0, n_steps=3)
    # clean twin
    ens2 = packing.place(wt.ReactorEnsemble(cols, n_zones=n))
    ens2.set_boundary(bc)
    es2 = ens2.step(1.0, n_steps=3)
    good = np.ones(N, bool); good[bad] = False
    assert np.array_equal(es.pH[good], es2.pH[good]) and np.array_equal(es.chlorine[good], es2.chlorine[good])
    assert np.array_equal(es.temperature[good], es2.temperature[good])
    assert not es.status[good].any()
    pHo, Clo, To, to, ost = oracle.ensemble_step(n, ens.constants, bc, 1.0, 3, pH0, s0.chlorine, s0.temperature,
                                                 s0.time, nthreads=2)
    assert np.array_equal(es.status, ost.astype(np.uint32))
    assert np.all(es.status[bad] == 64)                        # NONFINITE, nothing else
    assert np.all(es.time[bad] == 0.0) and np.all(es.time[good] == 3.0)
    assert np.array_equal(es.pH[bad], pH0[bad], equal_nan=True)              # state untouched
    assert np.array_equal(es.chlorine[bad], s0.chlorine[bad])
    packing.check(ens); packing.check(ens2)
    ens.close(); ens2.close()
    # the drop-in raises what the reference raises, and keeps its state
    nf = golden_json("g11_branches.json")["nonfinite"]
    r = wt.IntegratedCSTR(wt.ReactorConfiguration(n_zones=4))
    r.step(1.0, wt.BoundaryConditions())
    for bad in (np.nan, np.inf):
        r.state.pH = np.array([7.0, bad, 7.0, 7.0])
        with pytest.raises(ValueError) as ei:
            r.step(1.0, wt.BoundaryConditions())
        assert str(ei.value) == nf["nan"]["message"]
        assert r.state.time == nf["nan"]["time_after"] and np.array_equal(r.state.pH, [7.0, bad, 7.0, 7.0], equal_nan=True)


@pytest.mark.parametrize("n", [8, 20])
def test_full_size_hundred_steps_vs_oracle(gpu, wt, oracle, n):
    """BASELINE configs 2/3 at full size over 100 outer steps (ten checkpoints): every reactor and zone against the
    oracle -- the distribution tools/parity_report.py publishes (profiles/r3/parity_report.json), asserted here so that
    the driver's run sees it.  Observed: 99.99992 % (n = 8) / 99.9996 % (n = 20) of 2.4 M / 6 M samples within 1e-6,
    p99.99 5.6e-9 / 1.1e-7, max 2.2e-6 / 4.7e-6; the samples beyond 1e-6 belong to the reactors pinned against the
    reference itself in test_outlier_reactors_vs_reference."""
    N, steps, every = 10000, 100, 10
    cols, bc = wt.make_ensemble(N)
    ens = wt.ReactorEnsemble(cols, n_zones=n); ens.set_boundary(bc)
    s0 = ens.state
    pH, Cl, T, t = s0.pH, s0.chlorine, s0.temperature, s0.time
    errs = []
    for k in range(steps // every):
        es = ens.step(1.0, n_steps=every)
        pH, Cl, T, t, ost = oracle.ensemble_step(n, ens.constants, bc, 1.0, every, pH, Cl, T, t, nthreads=16)
        assert not es.status.any() and not ost.any()
        errs.append(np.stack([np.abs(es.pH - pH) / np.abs(pH), np.abs(es.chlorine - Cl) / np.abs(Cl),
                              np.abs(es.temperature - T) / np.abs(T)]).reshape(-1))
    ens.close()
    err = np.concatenate(errs)
    assert np.mean(err <= TOL) >= 1 - 1e-5                       # north-star tolerance on all but 1e-5 of the samples
    assert np.mean(err <= 1e-9) >= 0.995
    assert np.percentile(err, 99.99) <= 5e-7
    assert err.max() < 1e-5                                      # everything within the solver's own tolerance


# ---------------------------------------------------------------- pins against the reference itself (g10, g11)
@pytest.mark.parametrize("n", [4, 8, 20])
def test_outlier_reactors_vs_reference(gpu, wt, oracle, n):
    """The reactors of the 10 000 / 12 500-reactor bench ensembles on which GPU and CPU oracle differ by more than
    1e-7 (tools/outlier_scan.py), against 100 steps of the Python reference itself (tests/golden/g10_outliers_n*.npz).
    On these reactors the solve crosses stratification switches with repeated rejections; the bit-faithful CPU
    oracle leaves the 1e-6 band against the reference just the same (test_outlier_reactors_oracle_vs_reference).
    Asserted: the GPU is no worse against the reference than the oracle is, and every sample stays inside the
    solver's own tolerance."""
    from test_oracle_golden import outlier_errors
    g = golden_npz(f"g10_outliers_n{n}.npz")
    R, every, steps = g["reactors"], int(g["every"]), int(g["steps"])
    cols, bc = wt.make_ensemble(int(R.max()) + 1)
    ens = wt.ReactorEnsemble({k: v[R] for k, v in cols.items()}, n_zones=n)
    ens.set_boundary(np.ascontiguousarray(bc[:, R]))
    S = len(R)
    e_gpu = np.zeros(S)
    same_counters = 0
    for k in range(steps // every):
        es = ens.step(1.0, n_steps=every)
        assert not es.status.any()
        snap = g["snaps"][:, k]
        got = np.stack([es.pH, es.chlorine, es.temperature], axis=1)
        e_gpu = np.maximum(e_gpu, np.max(np.abs(got - snap) / np.abs(snap), axis=(1, 2)))
        same_counters += int(np.count_nonzero(np.all(ens.solver_stats()[:, :4] == g["stats"][:, (k + 1) * every - 1, :4], axis=1)))
    ens.close()
    e_orc = np.maximum(outlier_errors(wt, oracle, n, 0), outlier_errors(wt, oracle, n, 1))
    # observed (profiles/r3/parity_report.json, outlier_reactors_vs_reference): GPU max 3.4e-7 / 1.6e-6 / 5.4e-6 for
    # n = 4 / 8 / 20 against the oracle's 7.7e-9 / 1.4e-6 / 4.0e-6; 0 / 1 / 8 reactors beyond 1e-6 against 0 / 1 / 10;
    # the reference's own decision counters at 30/30, 80/80, 475/480 checkpoints
    assert e_gpu.max() < 1e-5                                               # the solver's own tolerance
    assert e_gpu.max() <= max(1.5 * e_orc.max(), 1e-6)                      # no worse than oracle vs reference
    assert (e_gpu > 1e-6).sum() <= (e_orc > 1e-6).sum() + 2
    assert same_counters >= 0.95 * S * (steps // every)                     # the reference's own decision sequence


def _branch(wt, name):
    from test_oracle_golden import branch_case
    return branch_case(wt, name)


@pytest.mark.parametrize("name", ["clamp_cl", "clamp_ph_hi", "clamp_ph_lo", "host_edit", "low_u_n4", "low_u_n8"])
def test_branch_fixtures_vs_reference(gpu, wt, name, caplog):
    """Clamps with their log lines (reactor.py:526-541), host-edited state and clock between steps (:467-472),
    velocity scale <= 1e-6 -> Ri = inf (spatial.py:270-275): the drop-in against the reference's own runs
    (tests/golden/g11_branches.npz), scipy counters included."""
    import logging
    c = _branch(wt, name)
    n = c["n"]
    fields = [str(x) for x in golden_npz("g11_branches.npz")["cfg_fields"]]
    cfgrow = golden_npz("g11_branches.npz")[f"{name}__cfg"]
    kw = {k: (bool(v) if k == "enable_thermal_stratification" else (int(v) if k == "n_zones" else float(v)))
          for k, v in zip(fields, cfgrow)}
    r = wt.IntegratedCSTR(wt.ReactorConfiguration(**kw))
    b = wt.BoundaryConditions(**{k: float(v) for k, v in zip(wt.params.BOUNDARY_FIELDS, c["bc"])})
    if name.startswith("low_u"):
        assert r.transport.superficial_velocity <= 1e-6
    for k in range(c["pre"].shape[0]):
        # the host edits self.state exactly as the reference run did before this step
        r.state.pH, r.state.chlorine, r.state.temperature = c["pre"][k][0].copy(), c["pre"][k][1].copy(), c["pre"][k][2].copy()
        r.state.time = float(c["pre_time"][k])
        with caplog.at_level(logging.WARNING):
            caplog.clear()
            s = r.step(c["dt"], b)
        got = np.stack([s.pH, s.chlorine, s.temperature])
        post = c["traj"][k + 1]
        tol = 1e-7 if (name == "clamp_ph_lo" and k == 0) else 1e-9
        assert np.all(np.abs(got - post) <= tol * np.abs(post) + 1e-300), (name, k)
        assert s.time == c["time"][k] and s.flow_rate == c["flow"][k]
        assert tuple(r._ens.solver_stats()[0][:4]) == tuple(c["stats"][k][:4]), (name, k)
        assert relerr(np.stack([s.H_concentration, s.density, s.chlorine_decay_rate]), c["derived"][k]) < 10 * tol
        msgs = [rec.getMessage() for rec in caplog.records]
        if k == 0 and name == "clamp_cl":
            assert msgs == ["Negative chlorine detected: clipped to 0"] and np.all(s.chlorine == 0.0)
        elif k == 0 and name in ("clamp_ph_hi", "clamp_ph_lo"):
            assert msgs == ["pH out of bounds: clipped to [0, 14]"]
        else:
            assert msgs == []


def test_low_velocity_rhs_vs_reference(gpu, wt):
    g = golden_npz("g11_branches.npz")
    n = 8
    cols = cfg_columns(g["rhs_low_u__cfg"], g["cfg_fields"])
    ens = wt.ReactorEnsemble(cols, n_zones=n)
    assert np.all(ens.constants[wt.params.P_USUP] <= 1e-6)
    ens.set_boundary(np.ascontiguousarray(g["rhs_low_u__bc"].T))
    y = g["rhs_low_u__y"]
    dpH, dCl, dT, fl = ens.derivatives(y[:, :n], y[:, n:2 * n], y[:, 2 * n:])
    assert not fl.any()
    ref = g["rhs_low_u__f"]
    # temperature rows are pure arithmetic: bit-identical to the reference where there is no heat loss (the kernel
    # multiplies by a precomputed U A / (rho cp V), the reference divides), to rounding elsewhere
    no_loss = g["rhs_low_u__bc"][:, 9] == 0
    assert no_loss.sum() > 10 and np.array_equal(dT[no_loss], ref[no_loss, 2 * n:])
    assert np.allclose(dT, ref[:, 2 * n:], rtol=1e-13, atol=1e-16)
    assert np.allclose(dpH, ref[:, :n], rtol=1e-9, atol=1e-18) and np.allclose(dCl, ref[:, n:2 * n], rtol=1e-9, atol=1e-18)
    ens.close()


def test_dropin_surface_and_reference_validators(gpu, wt, capsys):
    """The drop-in carries the reference's sub-objects (reactor.py:229-270), prints its diagnostics report
    (reactor.py:613-645) and passes the reference's own validation suite (core/__init__.py:266-294) on the GPU."""
    r = wt.IntegratedCSTR(wt.ReactorConfiguration(n_zones=5))
    assert isinstance(r.thermo, wt.TemperatureDependentKinetics) and isinstance(r.chemistry, wt.AqueousChemistry)
    assert isinstance(r.transport, wt.TransportModel) and isinstance(r.spatial, wt.SpatialModel) and isinstance(r.buffer, wt.BufferSystem)
    assert r.transport.K_exchange_per_s == r._ens.constants[wt.params.P_KEX, 0]
    assert r.transport.superficial_velocity == r._ens.constants[wt.params.P_USUP, 0] and r.chemistry.Kw == r._ens.constants[wt.params.P_KW, 0]
    assert abs(r.transport.mixing_time_seconds - 46.78) < 0.01 and r.transport.residence_time == 200.0
    for _ in range(3):
        r.step(1.0, wt.BoundaryConditions())
    capsys.readouterr()
    r.print_diagnostics()
    out = capsys.readouterr().out
    for line in ("CSTR PHYSICS DIAGNOSTICS", "Time: 3.0 s", "Residence time: 200.0 min", "Mixing time: 46.8 s", "Total Chlorine:",
                 "pH segregation index:"):
        assert line in out, line
    wt.run_all_validations()
    assert "ALL VALIDATIONS PASSED" in capsys.readouterr().out


def test_bench_as_the_driver_launches_one_rank(gpu):
    """bench.py under the driver's environment for one rank of config 4's shape (RANK / WORLD_SIZE set as
    torch.distributed.run sets them, 12 500 reactors x 8 zones, --steps 20 --warmup 5): RCCL initialisation, the timed
    loop, the device-to-device export and the final all_gather run through the bench's own code path on hardware."""
    import json, os, socket, subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    env = dict(os.environ, RANK="0", LOCAL_RANK="0", WORLD_SIZE="1", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--total-reactors", "12500", "--steps", "20",
                        "--warmup", "5", "--no-cpu-baseline"], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-1500:]
    lines = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    o = lines[0]
    assert o["n_gpus"] == 1 and o["steps"] == 20 and o["warmup"] == 5 and o["scaling"] == "strong"
    assert o["config"]["reactors_total"] == 12500 and o["flagged_reactors"] == 0
    assert o["final_gather_ms"] is not None and o["value"] > 1e8
    assert o["roofline"]["bound"] == "hbm" and 0 < o["roofline"]["frac"] < 1
