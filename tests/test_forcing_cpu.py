"""Per-step boundary schedules on the CPU: the g13 reference fixtures replayed through the C oracle, the synthetic
schedule generator, and the host-side checks of a schedule's shape (creating an ensemble needs a device)."""
import numpy as np
import pytest

from conftest import cfg_columns, golden_npz, relerr


@pytest.mark.parametrize("n", [4, 8, 20])
def test_forced_fixture_trajectory_and_decision_sequence(wt, oracle, n):
    """The reference driven by a new BoundaryConditions every step (tools/gen_golden_forcing.py): the oracle, one
    oracle.step per schedule row, follows its trajectory and takes scipy's decisions (nfev, njev, nlu, accepted steps)
    on every step, as test_trajectory_and_decision_sequence checks for the constant-boundary g3 runs."""
    g = golden_npz(f"g13_forced_n{n}.npz")
    cols = cfg_columns(g["cfg"], g["cfg_fields"])
    par = wt.params.derive_constants(cols, n)[:, 0]
    S, dt = g["schedule"], float(g["dt"])
    traj, stats = g["traj"], g["stats"]
    assert S.shape == (traj.shape[0] - 1, wt.params.NB)
    # the forcing really moves: dosing and heat loss switch both ways, inlet temperature and flow change
    for row in (4, 6, 9):
        on = S[:, row] > 0
        assert on.any() and (~on).any() and np.count_nonzero(on[1:] != on[:-1]) >= 2
    assert len(np.unique(S[:, 0])) >= 3 and S[-1, 3] > S[0, 3]
    assert S[:, 8].min() >= 12.0
    y = traj[0].reshape(-1).copy()
    t = 0.0
    worst = 0.0
    for k in range(S.shape[0]):
        y, t, der, status, st = oracle.step(n, par, S[k], dt, y, t, want_stats=True)
        assert status == 0
        worst = max(worst, relerr(y, traj[k + 1].reshape(-1)))
        assert (st.nfev, st.njev, st.nlu, st.nsteps) == tuple(stats[k][:4]), f"step {k}"
        assert relerr(der.reshape(3, n), g["derived"][k]) < 1e-9
        assert abs(t - g["time"][k]) < 1e-9
    assert worst < 1e-9
    assert np.array_equal(g["flow"], S[:, 0] + S[:, 4] + S[:, 6])


def test_make_boundary_schedule_is_deterministic_in_range_and_switches(wt):
    cols, bc = wt.make_ensemble(2000)
    S = wt.make_boundary_schedule(bc, 30, seed=5)
    assert S.shape == (30, wt.params.NB, 2000) and S.dtype == np.float64 and S.flags["C_CONTIGUOUS"]
    assert np.array_equal(S, wt.make_boundary_schedule(bc, 30, seed=5))
    assert not np.array_equal(S, wt.make_boundary_schedule(bc, 30, seed=6))
    # within the synthetic ranges of make_ensemble
    assert S[:, 0].min() >= 1.6 and S[:, 0].max() <= 12.0
    assert S[:, 1].min() >= 6.5 and S[:, 1].max() <= 8.5
    assert S[:, 2].min() >= 0.0 and S[:, 2].max() <= 1.0
    assert S[:, 3].min() >= 5.0 and S[:, 3].max() <= 35.0
    assert S[:, 4].max() <= 2.0 and S[:, 6].max() <= 1.0 and S[:, 9].max() <= 10.0
    assert np.array_equal(S[:, 5], np.broadcast_to(bc[5], S[:, 5].shape))
    assert np.array_equal(S[:, 7], np.broadcast_to(bc[7], S[:, 7].shape))
    # every step moves the inlet; heat loss only against an ambient of 12 degC or more
    assert np.all(np.any(S[1:, 0:4] != S[:-1, 0:4], axis=1))
    assert np.all(S[:, 8][S[:, 9] > 0] >= 12.0)
    # acid dosing, chlorine dosing and heat loss cross their `> 0` switches in both directions
    for row in (4, 6, 9):
        on = S[:, row] > 0
        assert np.any(on[:-1] & ~on[1:]) and np.any(~on[:-1] & on[1:])
        assert 0.2 < on.mean() < 0.8
        assert np.all(S[:, row][on] > 0.0)


def test_boundary_schedule_block_shapes_and_row_count(wt):
    N, K, NB = 3, 4, wt.params.NB
    S = np.arange(K * NB * N, dtype=np.float32).reshape(K, NB, N)
    blk = wt.boundary_schedule_block(S, K, N)
    assert blk.dtype == np.float64 and blk.flags["C_CONTIGUOUS"] and np.array_equal(blk, S)
    # a sequence of anything boundary_block takes, one item per step
    b0, b1 = wt.BoundaryConditions(), wt.BoundaryConditions(acid_flow_rate=0.5, inlet_temperature=25.0)
    blk = wt.boundary_schedule_block([b0, b1, [b0, b1, b0], {"heat_loss_coefficient": [1.0, 2.0, 3.0]}], K, N)
    assert blk.shape == (K, NB, N)
    assert np.array_equal(blk[0], wt.boundary_block(b0, N)) and np.array_equal(blk[1], wt.boundary_block(b1, N))
    assert np.array_equal(blk[2][:, 1], wt.boundary_block(b1, N)[:, 0])
    assert np.array_equal(blk[3][9], [1.0, 2.0, 3.0])
    with pytest.raises(ValueError, match="rows for n_steps"):
        wt.boundary_schedule_block(S, K + 1, N)
    with pytest.raises(ValueError, match="rows for n_steps"):
        wt.boundary_schedule_block([b0, b1], K, N)
    with pytest.raises(ValueError, match="shape"):
        wt.boundary_schedule_block(S[:, :, :2], K, N)
    with pytest.raises(ValueError, match="shape"):
        wt.boundary_schedule_block(S[0], K, N)
    with pytest.raises(ValueError):
        wt.boundary_schedule_block([b0, [b0, b1], b0, b0], K, N)    # a row with the wrong reactor count
