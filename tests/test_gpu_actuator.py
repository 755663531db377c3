"""Per-reactor actuator programs at every PLC scan (include/wtphys.h ``wt_ensemble_actuator_*``): the device's channel
state, queues and boundary rows follow the restatement in actuator_ref.py bit for bit, a pass-through element is
invisible, and a fused call with actuators gives the bits of the host loop it replaces."""
import numpy as np
import pytest

from actuator_ref import VS_DEMAND, VS_N_FAULT, VS_N_RATE, VS_POSITION, ActuatorRef
from alarm_ref import AlarmRef
from conftest import golden_json
from control_ref import ControlRef
from inject_ref import InjectRef
from program_helpers import (DT, K, MASTER, HostScan, acts, assert_all_equal, calls, everything, pi_loops, plant, ref_acts,
                             refused_as_checked, words)

pytestmark = pytest.mark.gpu


def _realistic(wt, N, seed, t_end):
    """Random per-reactor elements on all three channels: lags, rate limits, backlash, delays 0..8 and fault windows
    of both kinds that open and close inside a run of ``t_end`` seconds."""
    rng = np.random.default_rng(seed)
    out = []
    for ch, lim, lo in (("acid", 2.0, 0.0), ("chlorine", 1.0, 0.0), ("inlet", 20.0, 0.2)):
        t_fault = rng.uniform(0, 0.7 * t_end, N)
        out.append(wt.Actuator(
            ch, tau=np.where(rng.random(N) < 0.2, 0.0, rng.uniform(1, 120, N)),
            rate=np.where(rng.random(N) < 0.3, np.inf, lim * 10.0 ** rng.uniform(-4.0, -1.7, N)),
            backlash=np.where(rng.random(N) < 0.5, 0.0, rng.uniform(0, 0.1 * lim, N)),
            delay=rng.integers(0, 9, N), fault=rng.integers(0, 3, N), t_fault=t_fault,
            t_repair=np.where(rng.random(N) < 0.2, np.inf, t_fault + rng.uniform(0, 0.4 * t_end, N)),
            fail_value=rng.uniform(lo, lim, N)))
    return out


def _words(rng, N):
    """Scripted (acid, chlorine, inlet) float32 words: in range, over the limit, negative, NaN, and insignificant
    inlet words."""
    w = np.stack([rng.uniform(-0.5, 2.6, N), rng.uniform(-0.3, 1.3, N), rng.uniform(-2.0, 24.0, N)]).astype(np.float32)
    small = rng.random(N) < 0.3
    w[2, small] = rng.uniform(0, 0.1, small.sum()).astype(np.float32)
    w[rng.random((3, N)) < 0.05] = np.nan
    return w


def test_inert_and_cleared_programs_are_bit_invisible(gpu, wt, native):
    N, n = 1000, 8
    cols, bc = wt.make_ensemble(N, seed=41)
    chlorine, acid = pi_loops(wt, cols)
    off = wt.actuator_block(N, *_realistic(wt, N, 1, K * DT))
    off[:, 0] = 0.0                                          # every channel disabled, the other fields anything valid
    got = []
    for prog in (None, "none", "disabled", "cleared"):
        ens = plant(wt, cols, bc, n)
        ens.set_schedule(0, 7)
        ens.write_commands(*MASTER)
        ens.enable_control(chlorine, acid)
        if prog == "none":
            ens.set_actuators()
        elif prog == "disabled":
            assert native.lib().wt_ensemble_actuator_set(ens._h, native.dptr(off)) == 0
        elif prog == "cleared":
            ens.set_actuators(*_realistic(wt, N, 2, K * DT))
            ens.clear_actuators()
        ens.step(DT, n_steps=K, download=False)
        got.append(everything(ens, programs=("control",)))
        if prog in ("none", "disabled"):
            st = ens.actuator_state()
            assert not st.n_exec.any() and not st.delivered.any() and not st.travel.any()
            assert np.array_equal(st.position, bc[[4, 6, 0]]) and np.array_equal(st.queue[:, 5], bc[[4, 6, 0]])
            _, lt = next(calls(K, K))                        # the loop time after one call of K steps
            assert np.all(st.t_prev == lt)
        ens.close()
    for g, prog in zip(got[1:], ("none", "disabled", "cleared")):
        assert_all_equal(got[0], g, prog)


@pytest.mark.parametrize("n, N", [(4, 1500), (8, 1500), (20, 800), (32, 400)])
def test_pass_through_elements_give_the_bits_of_no_program(gpu, wt, n, N):
    cols, bc = wt.make_ensemble(N, seed=700 + n)
    chlorine, acid = pi_loops(wt, cols, seed=n)
    for interval in (1, 7, 50):
        out = []
        for prog in (False, True):
            ens = plant(wt, cols, bc, n)
            ens.set_schedule(0, interval)
            ens.write_commands(*MASTER)
            ens.enable_control(chlorine, acid)
            if prog:
                ens.set_actuators(wt.Actuator("inlet"), wt.Actuator("acid"), wt.Actuator("chlorine"))
            ens.step(DT, n_steps=K, download=False)
            out.append(everything(ens, programs=("control",)))
            if prog:
                st, b = ens.actuator_state(), ens.boundary()
                assert np.array_equal(st.position, st.demand) and np.array_equal(st.position, st.applied)
                assert np.array_equal(st.position, b[[4, 6, 0]]), (n, interval)
                assert np.all(st.n_exec == -(-K // interval)) and not st.n_rate.any()
            ens.close()
        assert not out[0][5].any()
        assert_all_equal(out[0], out[1], (n, interval))


def _scripted_loop(ens, hs, interval, n_steps, rng):
    """Calls of one scan interval with scripted holding words; after each, the device's actuator state, queues, t_prev
    and rows equal the restatement's (fed with the words after the injection tamper and the alarm trips)."""
    n_calls = 0
    for c in hs.calls(n_steps, interval):
        cmd = _words(rng, ens.n_reactors)
        ens.write_holding(words(cmd))
        ens.step(DT, n_steps=c, download=False)
        v, _, f = ens.sensor_readings()
        hs.scan(v, f, cmd)
        assert_all_equal(ref_acts(hs.act), acts(ens), (interval, n_calls))
        n_calls += 1
    return n_calls


@pytest.mark.parametrize("n", [8, 20])
def test_device_follows_the_restatement_under_scripted_words(gpu, wt, n):
    N, steps = 1000, 150
    cols, bc = wt.make_ensemble(N, seed=31 + n)
    prog = _realistic(wt, N, n, steps * DT)
    block = wt.actuator_block(N, *prog)
    for interval in (1, 7, 50):
        ens = plant(wt, cols, bc, n)
        ens.set_schedule(0, interval)
        ens.set_actuators(*prog)
        ref = ActuatorRef(block, ens.boundary(), np.zeros(N))
        _scripted_loop(ens, HostScan(N, act=ref), interval, steps, np.random.default_rng(interval))
        assert not ens.state.status.any()
        st = ref.st
        assert (st[:, VS_N_RATE] > 0).mean() > 0.05 and (st[:, VS_N_FAULT] > 0).mean() > 0.2, interval
        assert (st[:, VS_POSITION] != st[:, VS_DEMAND]).mean() > 0.3, interval
        ens.close()


def test_tampered_and_tripped_commands_go_through_the_element(gpu, wt):
    N, n, steps = 1000, 8, 150
    cols, bc = wt.make_ensemble(N, seed=5)
    prog = _realistic(wt, N, 77, steps * DT)
    block = wt.actuator_block(N, *prog)
    injections = [wt.Injection("acid_flow_rate", "gain", start=200.0, end=900.0, a=1.7),
                  wt.Injection("inlet_flow_rate", "constant", start=400.0, end=700.0, a=0.05)]
    trip = wt.Alarm("flow_main", "high", -1.0, source="field", on_bad="alarm", action="trip_chlorine",
                    trip_value=np.random.default_rng(3).uniform(0, 1, N))
    for interval in (1, 7, 50):
        ens = plant(wt, cols, bc, n)
        ens.set_schedule(0, interval)
        ens.set_injections(*injections)
        ens.set_alarms(trip)
        ens.set_actuators(*prog)
        ref = ActuatorRef(block, ens.boundary(), np.zeros(N))
        inj, alm = InjectRef(wt.injection_block(N, *injections)), AlarmRef(wt.alarm_block(N, trip), np.zeros(N))
        n_calls = _scripted_loop(ens, HostScan(N, inj=inj, alm=alm, act=ref), interval, steps,
                                 np.random.default_rng(10 + interval))
        st = ens.alarm_state()
        assert np.all(st.n_ovr_chlorine == n_calls - 1)                  # the trip acted at every scan after the first
        ens.close()


def test_end_to_end_equals_a_master_writing_the_applied_flows(gpu, wt):
    """On float32-exact grids (demands on multiples of 2^-6, backlash a power of two) the applied flows are float32
    values: a plant without actuators whose master writes them gets the same bits."""
    N, n, steps, interval = 1000, 8, 200, 5
    cols, bc = wt.make_ensemble(N, seed=88)
    rng = np.random.default_rng(8)
    bc = bc.copy()
    bc[4] = rng.integers(0, 2 * 64 + 1, N) / 64.0
    bc[6] = rng.integers(0, 64 + 1, N) / 64.0
    bc[0] = rng.integers(64, 20 * 64 + 1, N) / 64.0
    t_end = steps * DT
    prog = []
    for ch, lim in (("acid", 2), ("chlorine", 1), ("inlet", 20)):
        t_fault = np.floor(rng.uniform(0, 0.7 * t_end, N))
        prog.append(wt.Actuator(ch, backlash=np.where(rng.random(N) < 0.5, 0.0, 2.0 ** rng.integers(-5, -1, N)),
                                delay=rng.integers(0, 9, N), fault=rng.integers(0, 3, N), t_fault=t_fault,
                                t_repair=t_fault + np.floor(rng.uniform(0, 0.4 * t_end, N)),
                                fail_value=rng.integers(8 if ch == "inlet" else 0, lim * 64 + 1, N) / 64.0))
    block = wt.actuator_block(N, *prog)
    scripted = []
    for _ in range(-(-steps // interval)):
        w = np.stack([rng.integers(-8, 2 * 64 + 24, N), rng.integers(-8, 64 + 16, N),
                      rng.integers(-32, 22 * 64, N)]).astype(np.float64) / 64.0
        small = rng.random(N) < 0.25
        w[2, small] = rng.integers(0, 7, small.sum()) / 64.0
        w = w.astype(np.float32)
        w[rng.random((3, N)) < 0.03] = np.nan
        scripted.append(w)
    ref = ActuatorRef(block, bc, np.zeros(N))
    applied = []
    for (_, lt), w in zip(calls(steps, interval, np.zeros(N)), scripted):
        ref.scan(w, lt)
        applied.append(ref.st[:, 1].astype(np.float32))
        assert np.array_equal(ref.st[:, 1], applied[-1].astype(np.float64))   # the grid keeps them float32-exact
    assert (ref.st[:, VS_N_FAULT] > 0).mean() > 0.3
    out = []
    for act in (True, False):
        ens = plant(wt, cols, bc, n)
        ens.set_schedule(0, interval)
        if act:
            ens.set_actuators(*prog)
        for (c, _), w in zip(calls(steps, interval), scripted if act else applied):
            ens.write_holding(words(w))
            ens.step(DT, n_steps=c, download=False)
        out.append(everything(ens, programs=()))
        if act:
            assert_all_equal(ref_acts(ref), acts(ens), "end to end")
        ens.close()
    assert not out[0][5].any()
    assert_all_equal(out[0], out[1], "end to end")


def test_fused_calls_equal_the_host_loop(gpu, wt, monkeypatch):
    N, n = 2000, 8
    cols, bc = wt.make_ensemble(N, seed=2024)
    chlorine, acid = pi_loops(wt, cols, seed=9)
    prog = _realistic(wt, N, 5, K * DT)
    block, cblock = wt.actuator_block(N, *prog), wt.control_block(N, chlorine, acid)
    refs = {}
    for interval in (1, 7, 50):
        ens = plant(wt, cols, bc, n)
        ens.set_schedule(0, interval)
        ens.write_commands(*MASTER)
        ens.set_actuators(*prog)
        ctl = ControlRef(cblock, np.zeros(N), holding=words(np.array(MASTER)[:, None] * np.ones(N)))
        act = ActuatorRef(block, ens.boundary(), np.zeros(N))
        HostScan(N, ctl=ctl, act=act).run(ens, K, interval)     # PI on the host, actuators on the device
        out = everything(ens, programs=()) + (ctl.st,) + acts(ens)
        assert not out[5].any()
        assert_all_equal(ref_acts(act), acts(ens), ("host loop", interval))
        refs[interval] = out
        ens.close()
    variants = [dict(streams=0, chunk=1), dict(streams=0, chunk=7), dict(streams=0, chunk=50), dict(streams=3, chunk=7),
                dict(streams=0, chunk=50, fused=False), dict(streams=0, chunk=7, tickets=True),
                dict(streams=0, chunk=1, adaptive=True)]
    for v in variants:
        if v.get("tickets"):
            monkeypatch.setenv("WT_Q_TICKETS", "1")            # the long-call split: one item per group and launch
        ens = plant(wt, cols, bc, n)
        ens.set_placement(v.get("adaptive", False))
        ens.set_schedule(v["streams"], v["chunk"])
        if v.get("tickets"):
            assert ens.item_steps(K) < K
        ens.write_commands(*MASTER)
        ens.set_actuators(*prog)
        ens.enable_control(chlorine, acid)
        for c, _ in calls(K, K // 5 if v.get("adaptive") else K):
            ens.step(DT, n_steps=c, fused=v.get("fused", True), download=False)
        if v.get("adaptive"):
            assert ens.schedule()["redeals"] >= 1 and not np.array_equal(ens.placement()[1], np.arange(N))
        got = everything(ens, programs=("control", "actuator"))
        assert_all_equal(refs[1 if not v.get("fused", True) else v["chunk"]], got, v)
        ens.close()
        monkeypatch.delenv("WT_Q_TICKETS", raising=False)


def test_frozen_reactors_get_no_evaluation(gpu, wt):
    # T out of range: the reactor stops stepping, so its elements are not evaluated any more
    g = golden_json("g4_faults.json")["cold_run"]
    cfg = wt.ReactorConfiguration(**g["config"])
    b = wt.BoundaryConditions(**dict(zip(wt.params.BOUNDARY_FIELDS, g["bc"])))
    ens = wt.ReactorEnsemble([cfg, wt.ReactorConfiguration(n_zones=4)])
    ens.set_boundary([b, wt.BoundaryConditions()])
    ens.enable_sensors(seed=1)
    ens.enable_plant_io()
    ens.write_commands([b.acid_flow_rate, 0.0], [b.chlorine_flow_rate, 0.0], [b.inlet_flow_rate, 1.0])
    ens.set_schedule(0, 1)
    ens.set_actuators(wt.Actuator("acid", tau=5.0), wt.Actuator("inlet", delay=2))
    Kc = 60
    es = ens.step(1.0, n_steps=Kc)
    st = ens.actuator_state()
    assert es.status[0] & 1 and es.time[0] < Kc and es.time[1] == Kc
    assert st.t_prev.tolist() == [es.time[0], Kc]
    assert st.n_exec[0].tolist() == [es.time[0], Kc] and st.n_exec[2].tolist() == [es.time[0], Kc]
    assert not st.n_exec[1].any()
    ens.close()
    # a non-finite state: the reactor never steps
    N, n = 64, 4
    cols, bc = wt.make_ensemble(N, seed=6)
    ens = plant(wt, cols, bc, n)
    s = ens.state
    pH = s.pH.copy()
    pH[5] = np.nan
    ens.set_state(pH, s.chlorine, s.temperature)
    ens.set_schedule(0, 3)
    ens.write_commands(*MASTER)
    ens.set_actuators(wt.Actuator("chlorine", tau=30.0, rate=0.01))
    es = ens.step(DT, n_steps=9)
    st = ens.actuator_state()
    assert es.status[5] & 64 and not np.delete(es.status, 5).any()
    assert st.t_prev[5] == 0.0 and st.n_exec[1, 5] == 0 and st.position[1, 5] == bc[6, 5]
    assert np.all(np.delete(st.n_exec[1], 5) == 3) and np.all(np.delete(st.t_prev, 5) == 90.0)
    assert ens.boundary()[6, 5] == bc[6, 5]
    ens.close()


def test_errors_and_lifetime(gpu, wt, native):
    N, n = 256, 4
    cols, bc = wt.make_ensemble(N, seed=12)
    pump = wt.Actuator("chlorine", tau=20.0, rate=0.005, delay=2)
    ens = wt.ReactorEnsemble(cols, n_zones=n)
    ens.set_boundary(bc)
    with pytest.raises(ValueError, match="plant I/O"):
        ens.set_actuators(pump)
    ens.enable_sensors(seed=4)
    with pytest.raises(ValueError, match="plant I/O"):
        ens.set_actuators(pump)
    ens.enable_plant_io()
    with pytest.raises(ValueError, match="no actuator program"):
        ens.actuator_state()
    # the n > 32 kernel carries no actuator section: such an ensemble refuses a program
    for big in (33, 40):
        other = plant(wt, cols, bc, big)
        with pytest.raises(ValueError, match="up to 32 zones"):
            other.set_actuators(pump)
        with pytest.raises(ValueError, match="no actuator program"):
            other.actuator_state()
        other.close()
    with pytest.raises(ValueError, match="two actuators"):
        ens.set_actuators(pump, pump)
    with pytest.raises(ValueError, match="delay must be"):
        ens.set_actuators(wt.Actuator("acid", delay=9))
    good = wt.actuator_block(N, pump, wt.Actuator("inlet", fault="fail_to", fail_value=5.0))
    for ch, row, value in ((0, 0, 2.0), (0, 0, 0.5), (1, 1, -1.0), (1, 1, np.inf), (1, 2, 0.0), (1, 2, -np.inf),
                           (1, 2, np.nan), (1, 3, -0.25), (1, 4, 9.0), (1, 4, 0.5), (1, 5, 3.0), (1, 6, np.inf),
                           (1, 7, -1.0), (2, 8, 0.1), (2, 8, 20.5), (0, 5, 2.0), (0, 8, np.nan)):
        bad = good.copy()
        bad[ch, row, 17] = value
        if (ch, row) == (0, 5):
            bad[0, 8, 17] = 2.5                                  # acid FAIL_TO to 2.5
        assert native.lib().wt_ensemble_actuator_set(ens._h, native.dptr(bad)) == native.WT_E_ARG, (ch, row, value)
        assert refused_as_checked(native, native.WT_PROG_ACTUATOR, bad), (ch, row, value)
    with pytest.raises(ValueError, match="no actuator program"):
        ens.actuator_state()                                     # a refused program leaves none behind
    ens.set_schedule(0, 5)
    ens.write_commands(*MASTER)
    ens.step(DT, n_steps=10, download=False)
    ens.set_actuators(pump)
    st = ens.actuator_state()
    assert np.all(st.t_prev == 100.0) and np.array_equal(st.position[1], np.full(N, float(np.float32(MASTER[1]))))
    ens.step(DT, n_steps=30, download=False)
    st = ens.actuator_state()
    assert np.all(st.n_exec[1] == 6) and not st.n_exec[[0, 2]].any()
    ens.write_commands(0.5, 0.75, 6.0)
    ens.step(DT, n_steps=20, download=False)
    st = ens.actuator_state()
    b = ens.boundary()
    assert np.all(st.demand[1] == 0.75) and np.all(st.position[1] < 0.75) and np.all(b[6] == st.position[1])
    ens.set_actuators(pump, wt.Actuator("acid"))             # set replaces the program and restarts from the rows
    st = ens.actuator_state()
    assert not st.n_exec.any() and np.all(st.t_prev == 600.0) and np.array_equal(st.position[1], b[6])
    assert np.array_equal(st.queue[1], np.tile(b[6], (8, 1)))
    ens.clear_actuators()
    with pytest.raises(ValueError, match="no actuator program"):
        ens.actuator_state()
    ens.clear_actuators()                                    # no effect while none is set
    ens.step(DT, n_steps=5, download=False)                  # the commands reach the plant at once again
    assert np.all(ens.boundary()[6] == 0.75)
    ens.set_actuators(pump)
    ens.close()                                              # destroy with a program set
