"""Per-reactor model predictive controllers at the PLC scans (include/wtphys.h ``wt_ensemble_mpc_*``): a scripted reading
with a known answer, a fused controlled call against the host master it replaces (tests/mpc_ref.py), the controllers
beside tuner, PI, alarm, actuator and injection programs, the lifecycle and the checkpoints.  Shapes: full wavefronts,
five wavefront-groups plus one reactor at n = 8 (row mode), 5 (non-row) and 20, and 33 reactors of 2 zones: 32 scan
lanes in one wavefront and a wavefront with one."""
import numpy as np
import pytest

import mpc_ref as MR
import tune_ref as UR
from actuator_ref import ActuatorRef
from alarm_ref import AlarmRef
from checkpoint_helpers import holding_words
from control_ref import CS_N_EXEC, CS_N_HELD, ControlRef, float32_words
from inject_ref import InjectRef
from program_helpers import (DT, MASTER, HostScan, acts, alarms, assert_all_equal, assert_equal_by_reactor, full_waves,  # noqa: F401
                             commands, plant, plant_state, ragged_size, ref_acts, ref_alarms, words)

pytestmark = pytest.mark.gpu

ZONES = (8, 5, 20, 2)


def ensemble(wt, n, seed=0):
    R, N = (32, 33) if n == 2 else ragged_size(n)
    cols, bc = wt.make_ensemble(N, seed=5200 + n + seed)
    return R, N, cols, bc


def observed(ens):
    """State, readings, boundary, input image and holding image of every reactor."""
    return plant_state(ens) + ens.input_image() + (holding_words(ens),)


def controllers(ens):
    return ens.mpc_state().block(), ens.mpc_prediction()


def exact_loop(wt):
    return wt.DMCLoop("chlorine_outlet", setpoint=1.5, step=[4.0], gain=[0.25], horizon=1, every=1, u0=0.125, out_max=1.0)


@pytest.mark.parametrize("n", ZONES)
def test_scripted_reading_has_the_known_answer(gpu, wt, full_waves, n):
    """An injection program holds the chlorine reading at 1.25.  Setpoint 1.5, step response 4 throughout, a horizon of one
    with gain 0.25: every term is 0.25 * 0.25, every move 0.0625 until the output reaches 1 at the fourteenth execution,
    and the flat prediction rises by 0.25 with every free move.  All numbers are dyadic, in float32 too; nothing here
    comes from the restatement.  An injected value leaves the instrument's fault code alone and a faulted scan holds: the
    answer is asserted for the reactors whose analyser reports no fault at any scan so far (the history says which)."""
    R, N, cols, bc = ensemble(wt, n)
    ens = plant(wt, cols, bc, n, history=60)
    ens.set_schedule(0, 1)
    ens.set_injections(wt.Injection("chlorine_outlet", "constant", start=0.0, end=np.inf, a=1.25))
    ens.set_mpc(chlorine=exact_loop(wt))
    assert ens.info(gpu.WT_INFO_MPC) == 1
    done = 0
    for steps in (10, 50):
        ens.step(DT, n_steps=steps, download=False)
        done += steps
        k = done - 1                                            # index of the last execution
        st, pred = ens.mpc_state(), ens.mpc_prediction()
        _, _, fault, filled = ens.sensor_history()
        assert np.all(filled == done)
        clean = ~fault[:done, 3].astype(bool).any(axis=0)
        print("n", n, "steps", done, "clean", int(clean.sum()), "of", N)
        assert clean.sum() >= N - 4 and clean[:R].any() and clean[-1:].any()
        c = type(st.chlorine)(*(row[clean] for row in st.block()[0]))
        assert not c.n_held.any() and st.chlorine.n_held[~clean].all()
        ones = np.ones(int(clean.sum()))
        outputs = np.minimum(1.0, 0.125 + 0.0625 * (np.arange(done) + 1.0))
        top = 1.5 + 0.25 * min(k, 13)
        for name, want in (("phase", 1.0), ("output", outputs[k]), ("count", 0.0), ("bias", 1.25 - (1.5 + 0.25 * min(k - 1, 13))),
                           ("move", 0.0625 if k <= 13 else 0.0), ("t_exec", DT * done), ("ise", 0.0625 * DT * k), ("iae", 0.25 * DT * k),
                           ("dose", float(np.sum(outputs[1:] * DT))), ("n_exec", float(done)), ("n_sat", float(max(0, k + 1 - 14))),
                           ("n_rate", 0.0), ("n_skipped", 0.0)):
            assert_equal_by_reactor((want * ones,), (getattr(c, name),), (name, done), R)
        assert_equal_by_reactor((top * np.ones((64, len(ones))),), (pred[0][:, clean],), ("prediction", done), R)
        assert not st.block()[1].any() and not pred[1].any()
        hr = holding_words(ens)
        assert np.array_equal(hr[clean, 2:4], np.broadcast_to(float32_words(outputs[k]), (len(ones), 2))) and not hr[:, [0, 1, 4, 5]].any()
        assert np.array_equal(ens.boundary()[6, clean], outputs[k - 1] * ones)   # what the scan before wrote has reached the plant
    ens.close()


def mixed_controllers(wt, cols):
    """Per-reactor controllers that between them reach every branch.  Chlorine loop on the outlet analyser: period 1, 3
    or 7 scans by r mod 3, horizon 1, 17 or 64 by (r // 3) mod 3 -- the gains are those of the CPU test's order check, so
    the p = 64 reactors tell a tree from a left-to-right sum --, moves unlimited or limited to 0.004 by r mod 2 (a limit
    in force erases the last bits of the sum, so the p = 64 reactors have none), start times staggered over five scans.  Acid loop on the outlet pH probe, whose 1800 s warm-up outlasts the run: it stays
    waiting, held at every scan it owns."""
    cl0 = np.asarray(cols["initial_chlorine"])
    r = np.arange(len(cl0))
    every = np.choose(r % 3, [1.0, 3.0, 7.0])
    horizon = np.choose((r // 3) % 3, [1.0, 17.0, 64.0])
    step = np.stack([wt.fopdt_step(2.0, 60.0, 30.0, DT * e) for e in every], axis=1)
    chlorine = wt.DMCLoop("chlorine_outlet", cl0 + 0.3, step, MR.order_gains(), horizon=horizon, every=every, u0=0.2,
                          du_max=np.where((r % 2 == 0) | (horizon == 64), np.inf, 0.004), t_start=100.0 + 20.0 * (r % 5))
    acid = wt.DMCLoop("pH_outlet", 7.2, -wt.fopdt_step(0.5, 100.0, 20.0, 2 * DT), -MR.order_gains(), every=2, u0=0.3, t_start=50.0)
    return chlorine, acid


class WithShadow(MR.LoopOwners):
    """The controllers alone, and beside them a restatement that adds its terms left to right on the same readings."""

    def __init__(self, mpc, shadow):
        super().__init__(None, mpc)
        self.shadow = shadow

    def scan(self, values, faults, t_now, stepped=None):
        super().scan(values, faults, t_now, stepped)
        self.shadow.scan(values, faults, t_now, stepped)


@pytest.mark.parametrize("n", ZONES)
def test_fused_controlled_call_equals_the_host_master(gpu, wt, full_waves, n):
    """The host master: calls of one step, the words of the restatement written before each, its scan after each.  Two
    reactors never step (a non-finite state) and one stops at step 40 (a zone above 100 degC), on both sides.  An
    injection program on both sides drops the chlorine reading out (NaN) during [100, 130), which holds the loops that
    are entitled by then while they wait, and during [300, 340), which holds running loops: their predictions shift."""
    STEPS, STOP_AT = 100, 40
    R, N, cols, bc = ensemble(wt, n, seed=1)
    chlorine, acid = mixed_controllers(wt, cols)
    blocks = wt.mpc_block(N, chlorine, acid)
    never, stopped = np.array([1, min(R + 2, N - 2)]), np.array([4])
    script = [wt.Injection("chlorine_outlet", "dropout", start=a, end=b) for a, b in ((100.0, 130.0), (300.0, 340.0))]

    def start(ens):
        ens.set_placement(False)
        ens.set_schedule(0, 1)
        ens.set_injections(*script)
        s = ens.state
        pH = s.pH.copy()
        pH[never, 0] = np.nan
        ens.set_state(pH, s.chlorine, s.temperature)

    def stop(ens):
        s = ens.state
        T = s.temperature.copy()
        T[stopped, 0] = 150.0
        ens.set_state(s.pH, s.chlorine, T)

    twin = plant(wt, cols, bc, n)
    start(twin)
    ref, shadow = MR.MpcRef(*blocks), MR.MpcRef(*blocks, total=MR.sequential_sum)
    hs = HostScan(N, tun=WithShadow(ref, shadow), inj=InjectRef(wt.injection_block(N, *script)))
    t_before, done = np.zeros(N), 0
    for c in hs.calls(STEPS, 1):
        if done == STOP_AT:
            stop(twin)
        w = hs.holding()
        twin.write_holding(w)
        twin.step(DT, n_steps=c, download=False)
        done += c
        t_now = twin.state.time
        stepped = t_now != t_before
        t_before = t_now
        v, _, f = twin.sensor_readings()
        hs.scan(v, f, commands(w), stepped)
    want = plant_state(twin) + twin.input_image() + (ref.holding,)
    twin.close()
    ens = plant(wt, cols, bc, n)
    start(ens)
    ens.set_mpc(chlorine, acid)
    ens.step(DT, n_steps=STOP_AT, download=False)
    stop(ens)
    ens.step(DT, n_steps=STEPS - STOP_AT, download=False)
    assert_equal_by_reactor(want, observed(ens), ("plant", n), R)
    assert_equal_by_reactor((ref.st, ref.pred), controllers(ens), ("controllers", n), R)
    assert_all_equal(blocks, ens.mpc_params(), "params")
    es = ens.state
    ens.close()
    # every branch was reached
    took = np.full(N, float(STEPS))
    took[never], took[stopped] = 0.0, float(STOP_AT)
    assert np.array_equal(es.time, took * DT)
    c, a = ref.st[0], ref.st[1]
    r = np.arange(N)
    through = took == STEPS
    print("n", n, "n_exec by period", [c[MR.MS_N_EXEC][through & (r % 3 == g)].tolist()[:4] for g in range(3)],
          "n_rate", c[MR.MS_N_RATE][:6].tolist(), "n_sat max", c[MR.MS_N_SAT].max(), "held", c[MR.MS_N_HELD][:6].tolist(),
          "acid held", a[MR.MS_N_HELD][:4].tolist())
    assert not ref.st[:, :, never].any() and not ref.pred[:, :, never].any()
    assert np.all(c[MR.MS_N_EXEC][stopped] > 0) and np.all(c[MR.MS_T_EXEC][stopped] <= STOP_AT * DT)
    # (an analyser of the plant may be in fault for much of a run: its loop is held, so these count reactors)
    for g in range(3):                                          # periods and horizons
        assert (through & (r % 3 == g) & (c[MR.MS_N_EXEC] >= 8)).sum() >= 3
        assert (through & ((r // 3) % 3 == g) & (c[MR.MS_N_EXEC] >= 8)).any()
    assert np.median(c[MR.MS_N_EXEC][through & (r % 3 == 0)]) > 3 * np.median(c[MR.MS_N_EXEC][through & (r % 3 == 2)])
    limited = through & np.isfinite(blocks[0][0, MR.M_DU_MAX])
    assert np.array_equal(np.isfinite(blocks[0][0, MR.M_DU_MAX]), (r % 2 == 1) & (blocks[0][0, MR.M_HORIZON] != 64))
    assert (c[MR.MS_N_RATE][limited] > 0).sum() >= 3          # (a horizon of 1 asks for moves below the limit)
    assert not c[MR.MS_N_RATE][~limited].any()
    # a loop of period 1 is held at the four scans of the second drop-out while it runs, and at the scans of the first
    # one from its t_start on while it waits: three of them for t_start 100, one for 120, none from 140 on
    each = through & (r % 3 == 0)
    assert np.all(c[MR.MS_N_HELD][each] >= 4) and len(np.unique(c[MR.MS_N_HELD][each])) >= 3, "the staggered starts fell on one scan"
    assert np.all(c[MR.MS_N_HELD][each & (r % 5 == 0)] >= 7) and np.all(c[MR.MS_N_EXEC][each & (r % 5 == 0)] <= STEPS - 12 - 4)
    assert np.all(a[MR.MS_PHASE] == MR.WAITING) and np.all(a[MR.MS_N_HELD][through] > 50) and not a[MR.MS_N_EXEC].any() and not ref.pred[1].any()
    assert not ref.holding[:, [0, 1, 4, 5]].any()               # a waiting loop writes no word
    p64 = through & (blocks[0][0, MR.M_HORIZON] == 64)
    shows = ((shadow.pred[0] != ref.pred[0]).any(axis=0) | (shadow.st[0] != ref.st[0]).any(axis=0)) & p64
    print("the order of the sum shows in", int(shows.sum()), "of", int(p64.sum()), "reactors with a horizon of 64")
    assert p64.sum() >= 3 and shows.any(), "the order of the sum does not show"


@pytest.mark.parametrize("n", ZONES)
def test_controllers_beside_the_other_programs(gpu, wt, full_waves, n):
    """Tuner, controller, PI, alarm, actuator and injection programs together.  Device: all in one fused call.  Host master:
    tuner, controller and PI in HostScan, alarms and actuators on the twin's device with their restatements following.
    An injection program on both sides scripts the chlorine reading -- 0.25 below the setpoint, and 0.25 above it during
    [200, 300) and [400, 500) -- so that outcomes do not hang on the plant's noise: every relay starts at 100 s, switches up
    at the first scans from 300 s and 500 s and finishes there with its one cycle.  The controllers of the even reactors
    are entitled to the loop from the start and count the scans the relay had it (n_skipped); those of the odd reactors
    start at 550 s, after the experiment.  From then on the chlorine PI stands still; the acid PI carries on."""
    R, N, cols, bc = ensemble(wt, n, seed=2)
    cl0 = np.asarray(cols["initial_chlorine"])
    r = np.arange(N)
    here = cl0 + 0.5
    tune = wt.RelayTune("chlorine_outlet", setpoint=here, amplitude=0.1, bias=0.3, start=100.0, settle=0, cycles=1)
    dmc = wt.DMCLoop.from_fopdt("chlorine_outlet", here, 2.0, 60.0, 30.0, DT, horizon=48, move_penalty=0.5, u0=0.3,
                                t_start=np.where(r % 2 == 0, 0.0, 550.0), du_max=0.05)
    pi_cl = wt.PILoop("chlorine_outlet", setpoint=here, kp=0.3, ki=1e-3, bias=np.where(r % 3 == 0, 0.2, 0.3))
    pi_ac = wt.PILoop("pH_outlet", setpoint=7.2, kp=0.4, ki=5e-4, direction=-1, bias=0.1)
    alarm = [wt.Alarm("chlorine_outlet", "low", cl0 - 0.05, deadband=0.02, source="field"),
             wt.Alarm("pH_outlet", "high", 7.25, on_delay=50.0, action="trip_acid", trip_value=0.8)]
    actuators = [wt.Actuator("chlorine", tau=40.0, rate=0.05, delay=3), wt.Actuator("acid", delay=2, rate=0.01)]
    script = [wt.Injection("chlorine_outlet", "constant", start=0.0, end=np.inf, a=here - 0.25)] + \
             [wt.Injection("chlorine_outlet", "constant", start=a, end=a + 100.0, a=here + 0.25) for a in (200.0, 400.0)]
    tblock, cblock, mblocks = wt.tune_block(N, tune), wt.control_block(N, pi_cl, pi_ac), wt.mpc_block(N, dmc)

    def programs(ens):
        ens.set_schedule(0, 1)
        ens.write_commands(*MASTER)
        ens.set_injections(*script)
        ens.set_alarms(*alarm)
        ens.set_actuators(*actuators)

    K1, K2 = 60, 30
    twin = plant(wt, cols, bc, n)
    programs(twin)
    ctl = ControlRef(cblock, np.zeros(N), holding=words(np.array(MASTER)[:, None] * np.ones(N)))
    tun = UR.TuneRef(tblock, ctl=ctl)
    ref = MR.MpcRef(*mblocks, words=ctl)
    alm, act = AlarmRef(wt.alarm_block(N, *alarm), np.zeros(N)), ActuatorRef(wt.actuator_block(N, *actuators), twin.boundary(), np.zeros(N))
    hs = HostScan(N, ctl=ctl, tun=MR.LoopOwners(tun, ref), inj=InjectRef(wt.injection_block(N, *script)), alm=alm, act=act)
    ens = plant(wt, cols, bc, n)
    programs(ens)
    ens.enable_control(pi_cl, pi_ac)
    ens.set_tuners(tune)
    ens.set_mpc(chlorine=dmc)

    def compare(stage):
        assert not twin.state.status.any()
        assert_equal_by_reactor(plant_state(twin) + twin.input_image() + (ctl.holding,), observed(ens), ("plant", stage), R)
        assert_equal_by_reactor(ref_alarms(alm) + ref_acts(act), alarms(ens) + acts(ens), ("alarm, actuator", stage), R)
        assert_equal_by_reactor((ctl.st, tun.st, ref.st, ref.pred),
                                (ens.control_state().block(), ens.tuner_state().block()) + controllers(ens), ("control, tuner, mpc", stage), R)
        assert_all_equal(ref_alarms(alm) + ref_acts(act), alarms(twin) + acts(twin), ("twin", stage))

    hs.run(twin, K1, 1)
    ens.step(DT, n_steps=K1, download=False)
    compare("taken over")
    ts, ms, cs = ens.tuner_state().chlorine, ens.mpc_state().chlorine, ens.control_state().block()
    print("n", n, "tuner phases", np.bincount(ts.phase.astype(int), minlength=4), "n_skipped", np.unique(ms.n_skipped), "n_exec", np.unique(ms.n_exec),
          "n_held", np.unique(ms.n_held))
    done = (ts.phase == UR.DONE) & (ts.n_held == 0) & (ms.n_held == 0)     # (a faulted scan may move a switch by a scan)
    assert done.sum() >= N - 6 and np.all(ts.t_done[done] == 500.0) and np.all(ts.t_begin[done] == 100.0)
    even = r % 2 == 0
    owned_by_relay = (ts.t_done - ts.t_begin) / DT + 1.0        # scans, the finishing one included
    assert np.array_equal(ms.n_skipped[even & done], owned_by_relay[even & done]) and not ms.n_skipped[~even].any()
    # before the relay (10 ... 90 s) and from 510 s on; from 550 s on
    assert np.all(ms.n_exec[even & done] == 19) and np.all(ms.n_exec[~even & done] == 6)
    hs.run(twin, K2, 1)
    ens.step(DT, n_steps=K2, download=False)
    compare("after")
    after = ens.control_state().block()
    assert np.array_equal(after[0][:, done], cs[0][:, done])    # the chlorine PI stands still
    assert np.all((after[1, CS_N_EXEC] + after[1, CS_N_HELD]) - (cs[1, CS_N_EXEC] + cs[1, CS_N_HELD]) == K2)
    last = ens.mpc_state().chlorine
    assert np.all((last.n_exec + last.n_held)[done] == (ms.n_exec + ms.n_held)[done] + K2) and np.all(last.n_exec[done] >= ms.n_exec[done] + K2 - 4)
    ens.close(); twin.close()


def test_lifecycle(gpu, wt, full_waves):
    L = gpu.lib()
    n = 8
    R, N, cols, bc = ensemble(wt, n, seed=3)
    loop = exact_loop(wt)
    blocks = wt.mpc_block(N, loop)
    ens = wt.ReactorEnsemble(cols, n_zones=n)
    ens.set_boundary(bc)
    assert ens.info(gpu.WT_INFO_MPC) == 0
    ens.enable_sensors(seed=4)                                  # the sensor suite alone is not what a controller needs
    assert L.wt_ensemble_mpc_set(ens._h, *(gpu.dptr(b) for b in blocks)) == gpu.WT_E_STATE
    assert L.wt_last_error().decode() == "model predictive controllers act on the plant I/O scan: enable plant I/O first"
    with pytest.raises(ValueError, match="plant I/O"):
        ens.set_mpc(loop)
    ens.enable_plant_io()
    ens.set_schedule(0, 1)
    ens.clear_mpc()                                             # no effect while none is set
    for call in (ens.mpc_state, ens.mpc_prediction, ens.mpc_params, ens.reset_mpc):
        with pytest.raises(ValueError, match="no model predictive controller is set"):
            call()
    bad = blocks[0].copy()
    bad[0, MR.M_HORIZON, N - 1] = 65
    assert L.wt_ensemble_mpc_set(ens._h, gpu.dptr(bad), gpu.dptr(blocks[1]), gpu.dptr(blocks[2])) == gpu.WT_E_ARG
    msg = L.wt_last_error()
    assert L.wt_mpc_check(N, gpu.dptr(bad), gpu.dptr(blocks[1]), gpu.dptr(blocks[2])) == gpu.WT_E_ARG and L.wt_last_error() == msg
    assert msg.decode() == f"horizon must be an integer in 1..64 (loop 0, reactor {N - 1})" and ens.info(gpu.WT_INFO_MPC) == 0
    ens.set_injections(wt.Injection("chlorine_outlet", "constant", start=0.0, end=np.inf, a=1.25))
    pi = wt.PILoop("chlorine_outlet", setpoint=1.5, kp=0.3, ki=1e-3, bias=0.2)
    ens.enable_control(pi)
    enabled = ens.control_state().block()
    ens.set_mpc(loop)
    assert ens.info(gpu.WT_INFO_MPC) == 1 and not ens.mpc_state().block().any() and not ens.mpc_prediction().any()
    assert_all_equal(blocks, ens.mpc_params(), "params")
    only = np.empty_like(blocks[2])
    gpu.check(L.wt_ensemble_mpc_params(ens._h, None, None, gpu.dptr(only)))
    assert np.array_equal(only, blocks[2])
    ens.step(DT, n_steps=30, download=False)
    first = ens.mpc_state().chlorine
    assert np.all(first.n_exec + first.n_held == 30) and (first.n_exec == 30).any()
    assert np.array_equal(ens.control_state().block(), enabled)             # the PI stood still all along
    hr = holding_words(ens)
    assert np.array_equal(hr[:, 2:4], float32_words(first.output))
    # reset: waiting again, state and prediction zeroed, the words kept; the next valid scan starts afresh from u0
    ens.reset_mpc()
    assert not ens.mpc_state().block().any() and not ens.mpc_prediction().any() and np.array_equal(holding_words(ens), hr)
    ens.step(DT, n_steps=1, download=False)
    again = ens.mpc_state().chlorine
    ran = again.n_exec == 1
    assert ran.sum() >= N - 4 and np.all(again.output[ran] == 0.1875) and np.all(again.t_exec[ran] == 31 * DT) and np.all(again.phase[ran] == 1)
    assert np.all(ens.mpc_prediction()[0][:, ran] == 1.5)
    # set over controllers in force replaces them and starts afresh as well
    ens.set_mpc(loop)
    assert not ens.mpc_state().block().any()
    ens.step(DT, n_steps=3, download=False)
    # clear: the switch is off, the words stay, and the PI resumes
    hr = holding_words(ens)
    ens.clear_mpc()
    assert ens.info(gpu.WT_INFO_MPC) == 0 and np.array_equal(holding_words(ens), hr)
    with pytest.raises(ValueError, match="no model predictive controller is set"):
        ens.mpc_state()
    ens.step(DT, n_steps=5, download=False)
    cs = ens.control_state().chlorine
    assert np.all(cs.n_exec + cs.n_held == 5) and (cs.n_exec == 5).any()
    pi_ran = cs.n_exec > 0
    assert np.array_equal(holding_words(ens)[pi_ran, 2:4], float32_words(cs.output[pi_ran]))
    ens.close()
    # 40 zones: the n > 32 kernel carries no program
    cfg = wt.ReactorConfiguration(n_zones=40)
    big = wt.ReactorEnsemble([cfg, cfg]); big.set_boundary(wt.BoundaryConditions())
    big.enable_sensors(seed=3); big.enable_plant_io()
    small = wt.mpc_block(2, loop)
    assert L.wt_ensemble_mpc_set(big._h, *(gpu.dptr(b) for b in small)) == gpu.WT_E_STATE
    assert L.wt_last_error().decode() == "model predictive controllers run in the kernels for up to 32 zones"
    assert big.info(gpu.WT_INFO_MPC) == 0
    big.close()


def test_checkpoints_carry_the_controllers(gpu, wt, full_waves):
    """Mid-run: the restored handle, the clone and a mark / rewind each continue with the bits of the handle that was
    never saved, controller state, prediction, parameters and model included."""
    n = 5
    R, N, cols, bc = ensemble(wt, n, seed=4)
    chlorine, acid = mixed_controllers(wt, cols)
    acid.sensor = "chlorine_inlet"                              # an instrument that is up: both loops run
    acid.setpoint = np.asarray(cols["initial_chlorine"]) - 0.2

    def fresh():
        ens = plant(wt, cols, bc, n)
        ens.set_schedule(0, 1)
        ens.set_mpc(chlorine, acid)
        return ens

    def full(ens):
        return observed(ens) + controllers(ens) + tuple(ens.mpc_params())

    SAVE, REST = 45, 35
    never = fresh(); never.step(DT, n_steps=SAVE, download=False); never.step(DT, n_steps=REST, download=False)
    want = full(never); never.close()
    a = fresh(); a.step(DT, n_steps=SAVE, download=False)
    mid = controllers(a)
    assert (mid[0][:, MR.MS_N_EXEC] > 0).any(axis=1).all() and (mid[0][:, MR.MS_COUNT] > 0).any() and mid[1].any()
    blob = a.checkpoint()
    bare = wt.ReactorEnsemble(cols, n_zones=n); bare.set_boundary(bc)
    no_io = bare.checkpoint()
    b = plant(wt, cols, bc, n, seed=1); b.restore(blob)
    c = a.clone()
    a.mark()
    for name, ens in (("original", a), ("restored", b), ("clone", c)):
        assert ens.info(gpu.WT_INFO_MPC) == 1
        ens.step(DT, n_steps=REST, download=False)
        assert_equal_by_reactor(want, full(ens), name, R)
    a.rewind()
    assert_all_equal(mid, controllers(a), "rewound state")
    a.step(DT, n_steps=REST, download=False)
    assert_equal_by_reactor(want, full(a), "rewound", R)
    assert (want[-5][:, MR.MS_N_EXEC] > mid[0][:, MR.MS_N_EXEC]).any()
    # a blob taken without plant I/O takes the controllers away
    b.restore(no_io)
    assert b.info(gpu.WT_INFO_MPC) == 0 and b.info(gpu.WT_INFO_PLANT_IO) == 0
    b.enable_sensors(seed=2); b.enable_plant_io()
    assert b.info(gpu.WT_INFO_MPC) == 0
    with pytest.raises(ValueError, match="no model predictive controller is set"):
        b.mpc_state()
    for ens in (a, b, c, bare):
        ens.close()


@pytest.mark.parametrize("n", ZONES)
def test_disabled_controllers_change_nothing(gpu, wt, full_waves, n):
    """Controllers whose loops are all off against none, beside a running PI program."""
    R, N, cols, bc = ensemble(wt, n, seed=5)
    pi = wt.PILoop("chlorine_outlet", setpoint=np.asarray(cols["initial_chlorine"]) + 2.0, kp=0.3, ki=1e-3, bias=0.2)
    off = exact_loop(wt)
    off.enable = 0
    out = []
    for controlled in (False, True):
        ens = plant(wt, cols, bc, n)
        ens.set_schedule(0, 1)
        ens.enable_control(pi)
        if controlled:
            ens.set_mpc(off, wt.DMCLoop("pH_outlet", 7.2, [-1.0], [-0.1], enable=0))
        ens.step(DT, n_steps=60, download=False)
        out.append(observed(ens) + (ens.control_state().block(),))
        if controlled:
            assert not ens.mpc_state().block().any() and not ens.mpc_prediction().any()
        ens.close()
    assert_equal_by_reactor(out[0], out[1], "disabled controllers", R)
