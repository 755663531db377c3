"""CPU checks of the per-reactor actuator programs: the restatement (actuator_ref.py) against worked answers and the
block of ``actuator_block`` with its validation (the C ABI symbols: test_host_api.py)."""
import importlib
import math

import numpy as np
import pytest

from actuator_ref import (VS_APPLIED, VS_DELIVERED, VS_DEMAND, VS_N_EXEC, VS_N_FAULT, VS_N_RATE, VS_PLAY, VS_POSITION,
                          VS_TRAVEL, ActuatorRef)


@pytest.fixture(scope="module")
def act(native):
    return importlib.import_module("ics-wt-physicsengine_amd.core.actuator")


def _bc(n=1, acid=0.0, chlorine=0.0, inlet=5.0):
    bc = np.zeros((10, n))
    bc[4], bc[6], bc[0] = acid, chlorine, inlet
    return bc


def _run(ref, commands, times, channel=0, other=(0.0, 0.0, 5.0)):
    """Scans with channel ``channel``'s word = commands[k]; returns the positions of that channel after each scan."""
    N = ref.p.shape[2]
    out = []
    for c, t in zip(commands, times):
        w = np.tile(np.asarray(other, dtype=np.float32)[:, None], (1, N))
        w[channel] = c
        ref.scan(w, np.full(N, t))
        out.append(float(ref.st[channel, VS_POSITION, 0]))
    return out


def test_backward_euler_step_response_by_hand(act):
    ref = ActuatorRef(act.actuator_block(1, act.Actuator("acid", tau=20.0)), _bc(), 0.0)
    got = _run(ref, [1.0, 1.0, 1.0], [10.0, 20.0, 30.0])
    # (tau * x + h * u) / (tau + h) with tau 20, h 10, u 1 from x 0: 1/3, then (20/3 + 10)/30 = 5/9, then 19/27
    assert got == pytest.approx([1 / 3, 5 / 9, 19 / 27], rel=1e-15, abs=0)
    assert ref.bc[4, 0] == got[-1] and ref.st[0, VS_APPLIED, 0] == got[-1]
    assert ref.st[0, VS_N_EXEC, 0] == 3 and ref.st[0, VS_N_RATE, 0] == 0


def test_rate_limited_ramp_reaches_its_target_on_time(act):
    rate, h, target = 0.01, 10.0, 0.75
    ref = ActuatorRef(act.actuator_block(1, act.Actuator("acid", rate=rate)), _bc(), 0.0)
    got = _run(ref, [target] * 12, np.arange(1, 13) * h)
    first = got.index(target) + 1
    assert first == math.ceil(target / (rate * h)) == 8
    assert all(x < target for x in got[:7]) and got[7:] == [target] * 5
    assert got[:7] == pytest.approx([0.1 * (k + 1) for k in range(7)], rel=1e-14)
    assert ref.st[0, VS_N_RATE, 0] == 7


@pytest.mark.parametrize("delay", range(9))
def test_delay_shifts_a_step_by_exactly_that_many_scans(act, delay):
    ref = ActuatorRef(act.actuator_block(1, act.Actuator("chlorine", delay=delay)), _bc(chlorine=0.25), 0.0)
    cmd = [0.25] * 3 + [0.75] * 12
    got = _run(ref, cmd, np.arange(1, 16) * 10.0, channel=1)
    assert got == [0.25] * (3 + delay) + [0.75] * (12 - delay)
    assert ref.q[1, :, 0].tolist() == [0.75] * 8
    assert ref.st[1, VS_DEMAND, 0] == 0.75


def test_backlash_absorbs_a_reversal_narrower_than_its_band(act):
    ref = ActuatorRef(act.actuator_block(1, act.Actuator("acid", backlash=0.5)), _bc(), 0.0)
    got = _run(ref, [1.0, 0.9, 0.75, 0.5, 0.5, 1.0], np.arange(1, 7) * 10.0)
    # half-width 0.25: a rise to 1.0 stops at 0.75; the output moves only once the command leaves [0.5, 1.0]
    assert got == [0.75, 0.75, 0.75, 0.75, 0.75, 0.75]
    got = _run(ref, [0.25, 0.25, 1.5], [70.0, 80.0, 90.0])
    assert got == [0.5, 0.5, 1.25]
    assert ref.st[0, VS_PLAY, 0] == 1.25


def test_stuck_holds_and_resumes_from_the_held_position(act):
    ref = ActuatorRef(act.actuator_block(1, act.Actuator("acid", rate=0.025, fault="stuck", t_fault=30.0, t_repair=60.0)),
                      _bc(), 0.0)
    got = _run(ref, [2.0] * 8, np.arange(1, 9) * 10.0)
    # 0.25 per scan; stuck at t = 30, 40, 50 (holds 0.5); from t = 60 on it moves on from 0.5
    assert got == [0.25, 0.5, 0.5, 0.5, 0.5, 0.75, 1.0, 1.25]
    assert ref.st[0, VS_N_FAULT, 0] == 3 and ref.st[0, VS_TRAVEL, 0] == 1.25


def test_fail_to_forces_its_value_inside_the_window(act):
    ref = ActuatorRef(act.actuator_block(1, act.Actuator("chlorine", fault="fail_to", t_fault=20.0, t_repair=40.0,
                                                         fail_value=1.0)), _bc(chlorine=0.25), 0.0)
    got = _run(ref, [0.25] * 5, np.arange(1, 6) * 10.0, channel=1)
    assert got == [0.25, 1.0, 1.0, 0.25, 0.25]
    assert ref.bc[6, 0] == 0.25 and ref.st[1, VS_N_FAULT, 0] == 2 and ref.st[1, VS_TRAVEL, 0] == 1.5


def test_inlet_keeps_its_last_demand_for_insignificant_words(act):
    ref = ActuatorRef(act.actuator_block(2, act.Actuator("inlet", delay=np.array([0, 1]))), _bc(2, inlet=4.0), 0.0)
    rows = []
    for k, word in enumerate([6.0, 0.09375, 0.0, np.nan, -3.0, 25.0, 0.05]):
        w = np.zeros((3, 2), dtype=np.float32)
        w[2] = word
        ref.scan(w, np.full(2, 10.0 * (k + 1)))
        rows.append(ref.bc[0].tolist())
    assert [r[0] for r in rows] == [6.0, 6.0, 6.0, 6.0, 6.0, 20.0, 20.0]
    assert [r[1] for r in rows] == [4.0, 6.0, 6.0, 6.0, 6.0, 6.0, 20.0]
    assert ref.st[2, VS_DEMAND].tolist() == [20.0, 20.0]
    # a lagging valve below 0.1 leaves the row where it was, not at the word the master sent
    ref = ActuatorRef(act.actuator_block(1, act.Actuator("inlet", tau=1000.0)), _bc(inlet=0.0), 0.0)
    w = np.zeros((3, 1), dtype=np.float32)
    w[2] = 10.0
    ref.scan(w, [10.0])
    assert 0 < ref.st[2, VS_POSITION, 0] <= 0.1 and ref.bc[0, 0] == 0.0 and ref.st[2, VS_APPLIED, 0] == 0.0


def test_uneven_scan_intervals(act):
    times = [10.0, 17.0, 67.0, 70.0]
    ref = ActuatorRef(act.actuator_block(1, act.Actuator("acid", tau=10.0)), _bc(acid=0.5), 0.0)
    got = _run(ref, [1.5] * 4, times)
    x, t0, want = 0.5, 0.0, []
    for t in times:
        h = t - t0
        x, t0 = (10.0 * x + h * 1.5) / (10.0 + h), t
        want.append(x)
    assert got == want
    assert ref.t_prev[0] == 70.0


def test_delivered_and_travel(act):
    ref = ActuatorRef(act.actuator_block(1, act.Actuator("acid")), _bc(acid=0.5), 0.0)
    _run(ref, [1.0, 0.25, 0.25, 2.0], [10.0, 20.0, 40.0, 45.0])
    # delivered integrates the applied flow over each interval before the scan changes it
    assert ref.st[0, VS_DELIVERED, 0] == 0.5 * 10 + 1.0 * 10 + 0.25 * 20 + 0.25 * 5
    assert ref.st[0, VS_TRAVEL, 0] == 0.5 + 0.75 + 0.0 + 1.75


def test_pass_through_and_disabled_channels_equal_the_bare_command_path(act):
    N = 50
    rng = np.random.default_rng(1)
    bc = _bc(N, acid=rng.random(N), chlorine=rng.random(N), inlet=rng.uniform(0, 10, N))
    refs = [ActuatorRef(act.actuator_block(N), bc, 0.0),
            ActuatorRef(act.actuator_block(N, act.Actuator("inlet"), act.Actuator("acid"), act.Actuator("chlorine")), bc, 0.0)]
    for k in range(20):
        w = rng.uniform(-1, 25, (3, N)).astype(np.float32)
        w[:, rng.random(N) < 0.1] = np.nan
        w[2, rng.random(N) < 0.3] = 0.05
        for r in refs:
            r.scan(w, np.full(N, 10.0 * (k + 1)))
        assert np.array_equal(refs[0].bc, refs[1].bc), k
    assert not refs[0].st[:, VS_N_EXEC].any() and np.all(refs[1].st[:, VS_N_EXEC] == 20)


def test_stepped_mask_leaves_a_reactor_alone(act):
    ref = ActuatorRef(act.actuator_block(2, act.Actuator("acid", tau=5.0)), _bc(2), 0.0)
    w = np.ones((3, 2), dtype=np.float32)
    ref.scan(w, [10.0, 10.0], stepped=[True, False])
    assert ref.t_prev.tolist() == [10.0, 0.0] and ref.st[0, VS_N_EXEC].tolist() == [1, 0]
    assert ref.bc[4, 1] == 0.0 and ref.bc[0, 1] == 5.0


def test_actuator_block_packing_and_broadcasting(act):
    N = 3
    blk = act.actuator_block(N, act.Actuator("inlet", tau=np.array([1.0, 2.0, 3.0]), delay=2, fault="fail_to",
                                             t_fault=100.0, fail_value=4.0),
                             act.Actuator("acid", rate=0.5, backlash=0.125, fault=np.array(["none", "stuck", "fail_to"]),
                                          t_repair=np.array([np.inf, 50.0, 60.0])))
    assert blk.shape == (3, 9, N) and blk.dtype == np.float64 and blk.flags["C_CONTIGUOUS"]
    assert np.array_equal(blk[0, :, 1], [1, 0.0, 0.5, 0.125, 0, 1, 0.0, 50.0, 0.0])
    assert blk[0, 7, 0] == np.inf and np.array_equal(blk[0, 5], [0, 1, 2])
    assert np.array_equal(blk[2, :, 2], [1, 3.0, np.inf, 0.0, 2, 2, 100.0, np.inf, 4.0])
    off = [0, 0.0, np.inf, 0.0, 0, 0, 0.0, np.inf, 0.0]
    assert np.array_equal(blk[1], np.tile(np.array(off)[:, None], (1, N)))
    assert np.array_equal(act.actuator_block(N), np.tile(np.array(off)[None, :, None], (3, 1, N)))
    assert np.array_equal(act.OFF_ROW, off)


@pytest.mark.parametrize("kw, msg", [
    (dict(channel="steam"), "unknown channel"),
    (dict(fault="jammed"), "unknown fault"),
    (dict(tau=np.nan), "must be finite"),
    (dict(tau=np.inf), "must be finite"),
    (dict(rate=-np.inf), "must be finite"),
    (dict(rate=np.nan), "must be finite"),
    (dict(t_fault=np.inf), "must be finite"),
    (dict(fail_value=np.inf), "must be finite"),
    (dict(tau=-1.0), "tau must be"),
    (dict(rate=0.0), "rate must be"),
    (dict(backlash=-0.1), "backlash must be"),
    (dict(delay=9), "delay must be"),
    (dict(delay=1.5), "delay must be"),
    (dict(delay=-1), "delay must be"),
    (dict(fault=3), "fault must be"),
    (dict(fault=0.5), "fault must be"),
    (dict(t_fault=10.0, t_repair=5.0), "t_repair must be"),
    (dict(fault="fail_to", fail_value=2.5), "fail_value must be in \\[0, limit\\]"),
    (dict(fault="fail_to", fail_value=-0.5), "fail_value must be in \\[0, limit\\]"),
    (dict(channel="chlorine", fault="fail_to", fail_value=1.5), "fail_value must be in \\[0, limit\\]"),
    (dict(channel="inlet", fault="fail_to", fail_value=0.1), "inlet fail_to"),
    (dict(channel="inlet", fault="fail_to", fail_value=21.0), "inlet fail_to"),
])
def test_actuator_block_validation(act, kw, msg):
    args = dict(channel="acid")
    args.update(kw)
    with pytest.raises(ValueError, match=msg):
        act.actuator_block(3, act.Actuator(**args))


def test_actuator_block_count_and_shape_errors(act):
    with pytest.raises(ValueError, match="two actuators on the acid channel"):
        act.actuator_block(3, act.Actuator("acid"), act.Actuator("inlet"), act.Actuator("acid", tau=1.0))
    with pytest.raises(ValueError, match="tau"):
        act.actuator_block(3, act.Actuator("acid", tau=np.ones(4)))
    with pytest.raises(TypeError):
        act.actuator_block(3, {"channel": "acid"})
    # without FAIL_TO the fail value is free; the default 0.0 is valid on every channel
    act.actuator_block(3, act.Actuator("inlet", fail_value=-7.0), act.Actuator("acid", fault="stuck", fail_value=9.0))
    act.actuator_block(3, act.Actuator("inlet", fault="stuck"), act.Actuator("chlorine"))
    # the first failed check is the one named
    with pytest.raises(ValueError, match="tau must be"):
        act.actuator_block(1, act.Actuator("acid", tau=-1.0, rate=-1.0, delay=20))


def test_actuator_state_block_round_trip(act):
    st = np.arange(3 * 9 * 4, dtype=np.float64).reshape(3, 9, 4)
    q = -np.arange(3 * 8 * 4, dtype=np.float64).reshape(3, 8, 4)
    tp = np.array([1.0, 2.0, 3.0, 4.0])
    s = act.ActuatorState.from_block(st, q, tp)
    assert np.array_equal(s.position, st[:, 0]) and np.array_equal(s.n_fault, st[:, 8])
    assert np.array_equal(s.queue, q) and np.array_equal(s.t_prev, tp)
    b, q2, tp2 = s.block()
    assert np.array_equal(b, st) and np.array_equal(q2, q) and np.array_equal(tp2, tp)
