"""Per-reactor relay autotune programs at the PLC scans (include/wtphys.h ``wt_ensemble_tune_*``): a scripted limit
cycle with a known answer, a fused tuned call against the host master it replaces (tests/tune_ref.py), the hand-over
to the PI programs, the lifecycle and the checkpoints.  Shapes: full wavefronts, five wavefront-groups plus one reactor,
at n = 8 (row mode), 5 (non-row) and 20."""
import numpy as np
import pytest

import tune_ref as UR
from actuator_ref import ActuatorRef
from alarm_ref import AlarmRef
from checkpoint_helpers import holding_words
from inject_ref import InjectRef
from control_ref import CS_INTEGRAL, CS_N_EXEC, CS_N_HELD, CS_OUTPUT, C_KI, C_KP, ControlRef, float32_words
from program_helpers import (DT, K, MASTER, HostScan, acts, alarms, assert_all_equal, assert_equal_by_reactor, full_waves,  # noqa: F401
                             plant, plant_state, ragged_size, ref_acts, ref_alarms, words)

pytestmark = pytest.mark.gpu

ZONES = (8, 5, 20)


def ensemble(wt, n, seed=0):
    R, N = ragged_size(n)
    cols, bc = wt.make_ensemble(N, seed=4100 + n + seed)
    return R, N, cols, bc


def observed(ens):
    """State, readings, boundary, input image and holding image of every reactor."""
    return plant_state(ens) + ens.input_image() + (holding_words(ens),)


def operating_point(wt, cols, bc, n, seed=11):
    """The outlet chlorine reading of every reactor at 100 s, past the analyser's warm-up: where a commissioning engineer
    puts the setpoint of a relay test.  (The analysers carry a start-up offset: the reading is not the state.)"""
    ens = plant(wt, cols, bc, n, seed=seed)
    ens.step(DT, n_steps=10, download=False)
    v = ens.sensor_readings()[0][3].astype(np.float64)
    ens.close()
    return np.where(np.isfinite(v), v, np.nanmedian(v))


def mixed_tuners(wt, cols, setpoint, commission=False):
    """Per-reactor experiments that between them reach every outcome within K steps.  Chlorine loop, by reactor mod 4:
    0 and 3 -- no hysteresis on the noisy outlet reading around its operating point: the relay chatters and finishes (3: with
    its own start time, a scan apart from its neighbours'); 1 -- a hysteresis no reading exceeds: never switches and
    times out; 2 -- a start beyond the run: still waiting at the end.  Acid loop on the outlet pH probe, whose 1800 s
    warm-up gives held scans, started at staggered times."""
    cl0 = np.asarray(cols["initial_chlorine"])
    N = len(cl0)
    r = np.arange(N)
    chlorine = wt.RelayTune("chlorine_outlet", setpoint=setpoint, amplitude=np.where(r % 2 == 0, 0.2, 0.1), bias=0.3,
                            hysteresis=np.where(r % 4 == 1, 50.0, 0.0),
                            start=np.select([r % 4 == 2, r % 4 == 3], [10 * K * DT, 100.0 + 10.0 * r], 0.0),
                            timeout=np.where(r % 4 == 1, 1000.0 + 10.0 * r, np.inf), settle=0, cycles=np.where(r % 8 == 0, 1, 2),
                            rule="tyreus_luyben_pi", commission=(r % 4 == 0) if commission else False)
    acid = wt.RelayTune("pH_outlet", setpoint=7.2, amplitude=0.25, bias=0.5, direction=-1, hysteresis=0.0,
                        start=1500.0 + 20.0 * (r % 7), timeout=np.where(r % 3 == 0, 700.0, np.inf), settle=0, cycles=2,
                        rule=(0.3, 1.5))
    return chlorine, acid


@pytest.mark.parametrize("interval", [1, 3])
@pytest.mark.parametrize("n", ZONES)
def test_scripted_limit_cycle_has_the_known_answer(gpu, wt, full_waves, n, interval):
    """An injection program scripts the chlorine reading: 1.25, and 1.75 in three windows of 60 s every 120 s (times the
    scan interval).  Around the setpoint 1.5 that is an error of +-0.25 with a period of 120 s: the relay starts +1 at the
    first scan, goes down at 60, up at 120 (the first up-switch marks time), and the up-switches at 240 and 360 close
    the two measured cycles.  Nothing here comes from the restatement.  An injected value leaves the instrument's fault
    code alone, and a faulted scan holds: the answer is asserted for the reactors whose DPD analyser reports no fault at
    any scan of the run (the sensor history says which), all but a few."""
    R, N, cols, bc = ensemble(wt, n)
    s = float(interval)
    steps = 40 * interval
    ens = plant(wt, cols, bc, n, history=steps)
    ens.set_schedule(0, interval)
    ens.set_injections(wt.Injection("chlorine_outlet", "constant", start=0.0, end=np.inf, a=1.25),
                       *(wt.Injection("chlorine_outlet", "constant", start=a * s, end=(a + 60.0) * s, a=1.75) for a in (60.0, 180.0, 300.0)))
    ens.set_tuners(chlorine=wt.RelayTune("chlorine_outlet", setpoint=1.5, amplitude=0.25, bias=0.5, hysteresis=0.0, settle=0,
                                         cycles=2))
    assert ens.info(gpu.WT_INFO_TUNE) == 1
    ens.step(DT, n_steps=steps, download=False)
    st = ens.tuner_state()
    _, _, fault, filled = ens.sensor_history()
    assert np.all(filled == steps)
    clean = ~fault[interval - 1::interval, 3].astype(bool).any(axis=0)
    assert clean.sum() >= N - 4 and clean[:R].any() and clean[-R - 1:].any()
    c = type(st.chlorine)(*(row[clean] for row in st.block()[0]))
    assert not c.n_held.any() and st.chlorine.n_held[~clean].all()
    ones = np.ones(int(clean.sum()))
    for name, want in (("phase", 2.0), ("t_begin", 10.0 * s), ("t_done", 360.0 * s), ("period", 120.0 * s), ("amplitude", 0.25),
                       ("n_up", 3.0), ("n_cycles", 2.0), ("n_exec", 36.0), ("relay", 1.0), ("output", 0.5), ("t_up", 360.0 * s),
                       ("sum_period", 240.0 * s), ("sum_amp", 0.5), ("commissioned", 0.0)):
        assert_equal_by_reactor((want * ones,), (getattr(c, name),), name, R)
    ku = (4.0 * 0.25) / (3.141592653589793 * np.sqrt(0.25 * 0.25 - 0.0 * 0.0))
    kp = 0.45 * ku
    ki = kp / ((1.0 / 1.2) * (120.0 * s))
    assert_equal_by_reactor((ku * ones, kp * ones, ki * ones), (c.ku, c.kp, c.ki), "gains", R)
    assert not st.acid.phase.any() and not st.block()[1].any()
    hr = holding_words(ens)
    assert np.array_equal(hr[clean, 2:4], np.broadcast_to(float32_words(0.5), (len(ones), 2))) and not hr[:, [0, 1, 4, 5]].any()
    assert np.array_equal(ens.boundary()[6, clean], 0.5 * ones)        # the centre output reached the plant
    ens.close()


@pytest.mark.parametrize("n, interval", [(8, 1), (5, 7), (20, 3)])
def test_fused_tuned_call_equals_the_host_master(gpu, wt, full_waves, n, interval):
    R, N, cols, bc = ensemble(wt, n)
    chlorine, acid = mixed_tuners(wt, cols, operating_point(wt, cols, bc, n))
    block = wt.tune_block(N, chlorine, acid)
    twin = plant(wt, cols, bc, n)
    twin.set_schedule(0, interval)
    ref = UR.TuneRef(block)
    HostScan(N, tun=ref, emulated=True).run(twin, K, interval)
    want = plant_state(twin) + twin.input_image() + (ref.holding,)
    twin.close()
    ens = plant(wt, cols, bc, n)
    ens.set_schedule(0, interval)
    ens.set_tuners(chlorine, acid)
    ens.step(DT, n_steps=K, download=False)
    assert not want[5].any()
    assert_equal_by_reactor(want, observed(ens), ("plant", n, interval), R)
    got = ens.tuner_state().block()
    assert_equal_by_reactor((ref.st,), (got,), ("tuner state", n, interval), R)
    assert np.array_equal(ens.tuner_params(), block)
    ens.close()
    # the parameters must keep covering every outcome
    c, a = ref.st[0], ref.st[1]
    r = np.arange(N)
    print("chlorine phases", np.bincount(c[UR.US_PHASE].astype(int), minlength=4), "by group", [np.bincount(c[UR.US_PHASE][r % 4 == g].astype(int), minlength=4).tolist() for g in range(4)],
          "max n_up", c[UR.US_N_UP].max(), "acid phases", np.bincount(a[UR.US_PHASE].astype(int), minlength=4), "held", a[UR.US_N_HELD].max())
    assert (c[UR.US_PHASE] == UR.DONE).any() and (c[UR.US_PHASE][r % 4 == 3] == UR.DONE).any(), "no chlorine experiment finished"
    assert (c[UR.US_PHASE][r % 4 == 1] == UR.FAILED).all() and (c[UR.US_N_UP][r % 4 == 1] == 0).all(), "no time-out"
    assert (c[UR.US_PHASE][r % 4 == 2] == UR.WAITING).all(), "no experiment still waiting"
    assert len(np.unique(c[UR.US_T_BEGIN][r % 4 == 3])) > 3, "the staggered starts fell on one scan"
    assert (a[UR.US_N_HELD] > 0).any() and (a[UR.US_N_EXEC] > 0).any(), "no held scan on the warming pH probe"
    assert (c[UR.US_N_UP] >= 2).any() and (c[UR.US_KU][c[UR.US_PHASE] == UR.DONE] > 0).all()


@pytest.mark.parametrize("n, interval", [(8, 1), (5, 7), (20, 3)])
def test_tuner_beside_the_control_program(gpu, wt, full_waves, n, interval):
    """Tuner, PI, alarm and actuator programs together.  Device: all four in one fused call.  Host master: tuner and PI
    in HostScan (a TuneRef, then the ControlRef it commissions), alarms and actuators on the twin's device with their restatements
    following.  An injection program on both sides scripts the chlorine reading the tuner and the PI see -- 0.25 below
    the setpoint, and 0.25 above it during [600, 900), [1200, 1500) and [1800, 2100) -- so that which experiments finish
    does not hang on the plant's noise: every relay that runs switches up at the first scans from 900, 1500 and 2100 s,
    which closes one cycle by 1500 s and two by 2100 s (plus a scan interval), well inside the 3000 s of the run.  The
    commands still reach the plant through the alarm trips and the actuators."""
    R, N, cols, bc = ensemble(wt, n, seed=1)
    cl0 = np.asarray(cols["initial_chlorine"])
    r = np.arange(N)
    here = operating_point(wt, cols, bc, n)
    chlorine, acid = mixed_tuners(wt, cols, here, commission=True)
    acid.enable = 0                                         # the acid PI loop runs on, untuned
    pi_cl = wt.PILoop("chlorine_outlet", setpoint=here, kp=0.3, ki=1e-3, bias=np.where(r % 3 == 0, 0.2, 0.3),
                      enable=np.where(r % 16 == 8, 0, 1))
    pi_ac = wt.PILoop("pH_outlet", setpoint=7.2, kp=0.4, ki=5e-4, direction=-1, bias=0.1)
    alarm = [wt.Alarm("chlorine_outlet", "low", cl0 - 0.05, deadband=0.02, source="field"),
             wt.Alarm("pH_outlet", "high", 7.25, on_delay=50.0, action="trip_acid", trip_value=0.8)]
    actuators = [wt.Actuator("chlorine", tau=40.0, rate=0.05, delay=3), wt.Actuator("acid", delay=2, rate=0.01)]
    script = [wt.Injection("chlorine_outlet", "constant", start=0.0, end=np.inf, a=here - 0.25)] + \
             [wt.Injection("chlorine_outlet", "constant", start=a, end=a + 300.0, a=here + 0.25) for a in (600.0, 1200.0, 1800.0)]
    tblock, cblock = wt.tune_block(N, chlorine, acid), wt.control_block(N, pi_cl, pi_ac)

    def programs(ens):
        ens.set_schedule(0, interval)
        ens.write_commands(*MASTER)
        ens.set_injections(*script)
        ens.set_alarms(*alarm)
        ens.set_actuators(*actuators)

    K1, K2 = 60, K - 60                                     # a look inside the experiments, then the rest
    twin = plant(wt, cols, bc, n)
    programs(twin)
    ctl = ControlRef(cblock, np.zeros(N), holding=words(np.array(MASTER)[:, None] * np.ones(N)))
    enabled = ctl.st.copy()
    ref = UR.TuneRef(tblock, ctl=ctl)
    alm, act = AlarmRef(wt.alarm_block(N, *alarm), np.zeros(N)), ActuatorRef(wt.actuator_block(N, *actuators), twin.boundary(), np.zeros(N))
    hs = HostScan(N, ctl=ctl, tun=ref, inj=InjectRef(wt.injection_block(N, *script)), alm=alm, act=act)
    ens = plant(wt, cols, bc, n)
    programs(ens)
    ens.enable_control(pi_cl, pi_ac)
    ens.set_tuners(chlorine, acid)

    def compare(stage):
        assert not twin.state.status.any()
        assert_equal_by_reactor(plant_state(twin) + twin.input_image() + (ref.holding,), observed(ens), ("plant", stage), R)
        assert_equal_by_reactor(ref_alarms(alm) + ref_acts(act), alarms(ens) + acts(ens), ("alarm, actuator", stage), R)
        assert_equal_by_reactor((ctl.st, ref.st), (ens.control_state().block(), ens.tuner_state().block()), ("control, tuner", stage), R)
        assert_all_equal(ref_alarms(alm) + ref_acts(act), alarms(twin) + acts(twin), ("twin", stage))

    hs.run(twin, K1, interval)
    ens.step(DT, n_steps=K1, download=False)
    compare("inside")
    # while a tuner runs its PI loop stands still (t_prev is not part of the state block); the other loop runs on
    cs, ts = ens.control_state().block(), ens.tuner_state().block()
    running = ts[0, UR.US_PHASE] == UR.RUNNING
    since_enable = running & (ts[0, UR.US_T_BEGIN] == (10.0 if interval == 1 else DT * interval))
    assert since_enable.sum() >= 3
    assert np.array_equal(cs[0][:, since_enable], enabled[0][:, since_enable])
    scans = len(list(HostScan(N).calls(K1, interval)))
    assert np.all(cs[1, CS_N_EXEC] + cs[1, CS_N_HELD] == scans)
    waiting = ts[0, UR.US_PHASE] == UR.WAITING                # not started yet: the PI loop runs
    pi_on = cblock[0, 0] == 1
    assert (waiting & pi_on).any() and np.all((cs[0, CS_N_EXEC] + cs[0, CS_N_HELD])[waiting & pi_on] == scans)
    hs.run(twin, K2, interval)
    ens.step(DT, n_steps=K2, download=False)
    compare("after")
    ts = ens.tuner_state()
    com = ts.chlorine.commissioned == 1
    done = ts.chlorine.phase == UR.DONE
    print("commissioned", int(com.sum()), "done", int(done.sum()), "phases", np.bincount(ts.chlorine.phase.astype(int), minlength=4))
    assert com.any(), "no experiment commissioned its loop"
    assert (done & ~com & (tblock[0, UR.U_COMMISSION] == 0)).any(), "no experiment finished without commissioning"
    assert not (com & ~pi_on).any() and np.all(com <= ((tblock[0, UR.U_COMMISSION] == 1) & done))
    params = np.empty_like(cblock)
    gpu.check(gpu.lib().wt_ensemble_program_params(ens._h, gpu.WT_PROG_CONTROL, gpu.dptr(params)))
    assert np.array_equal(params, ctl.p)
    assert np.array_equal(params[0, C_KP, com], ts.chlorine.kp[com]) and np.array_equal(params[0, C_KI, com], ts.chlorine.ki[com])
    assert np.array_equal(params[0, C_KP, ~com], cblock[0, C_KP, ~com])
    # retune_control reads the records in force: the commissioned loop keeps its gains and its state
    before = ens.control_state().block()
    new_acid = wt.PILoop("pH_outlet", setpoint=7.1, kp=0.2, ki=1e-4, direction=-1, bias=0.1)
    ens.retune_control(acid=new_acid)
    kept = ctl.p.copy()
    kept[1] = wt.control_block(N, None, new_acid)[1]
    ctl.retune(kept)
    assert np.array_equal(ens.control_state().block(), before)
    gpu.check(gpu.lib().wt_ensemble_program_params(ens._h, gpu.WT_PROG_CONTROL, gpu.dptr(params)))
    assert np.array_equal(params, kept)
    tail = 4 * interval
    hs.run(twin, tail, interval)
    ens.step(DT, n_steps=tail, download=False)
    compare("retuned")
    ens.close(); twin.close()


def test_lifecycle(gpu, wt, full_waves):
    L = gpu.lib()
    n = 8
    R, N, cols, bc = ensemble(wt, n, seed=2)
    here = operating_point(wt, cols, bc, n, seed=4)
    tune = wt.RelayTune("chlorine_outlet", setpoint=here, amplitude=0.2, bias=0.3, settle=0, cycles=1, commission=True)
    blk = wt.tune_block(N, tune)
    ens = wt.ReactorEnsemble(cols, n_zones=n)
    ens.set_boundary(bc)
    assert ens.info(gpu.WT_INFO_TUNE) == 0
    ens.enable_sensors(seed=4)                              # the sensor suite alone is not what a tuner needs
    assert L.wt_ensemble_tune_set(ens._h, gpu.dptr(blk)) == gpu.WT_E_STATE
    assert L.wt_last_error().decode() == "tuners act on the plant I/O scan: enable plant I/O first"
    with pytest.raises(ValueError, match="plant I/O"):
        ens.set_tuners(tune)
    ens.enable_plant_io()
    ens.set_schedule(0, 1)
    ens.clear_tuners()                                      # no effect while none is set
    bad = blk.copy()
    bad[0, UR.U_CYCLES, N - 1] = 0
    assert L.wt_ensemble_tune_set(ens._h, gpu.dptr(bad)) == gpu.WT_E_ARG
    msg = L.wt_last_error()
    assert L.wt_tune_check(N, gpu.dptr(bad)) == gpu.WT_E_ARG and L.wt_last_error() == msg
    assert ens.info(gpu.WT_INFO_TUNE) == 0
    pi = wt.PILoop("chlorine_outlet", setpoint=here, kp=0.3, ki=1e-3, bias=0.2)
    ens.enable_control(pi)
    ens.set_tuners(tune)
    assert ens.info(gpu.WT_INFO_TUNE) == 1 and not ens.tuner_state().block().any()
    ens.step(DT, n_steps=K, download=False)
    first = ens.tuner_state()
    com = first.chlorine.commissioned == 1
    assert com.any() and np.array_equal(com, first.chlorine.phase == UR.DONE)
    gains = np.empty((2, 9, N))
    gpu.check(L.wt_ensemble_program_params(ens._h, gpu.WT_PROG_CONTROL, gpu.dptr(gains)))
    assert np.array_equal(gains[0, C_KP, com], first.chlorine.kp[com])
    # disable_control leaves the tuner running: a reset experiment runs again, commissions nothing, and owns its words
    ens.disable_control()
    assert ens.info(gpu.WT_INFO_TUNE) == 1
    ens.reset_tuners()
    assert not ens.tuner_state().block().any()
    ens.step(DT, n_steps=1, download=False)
    again = ens.tuner_state().chlorine
    assert np.all(again.phase == UR.RUNNING) and np.all(again.t_begin == (K + 1) * DT)   # t_start has passed: at the next scan
    hr = holding_words(ens)
    assert np.array_equal(hr[:, 2:4], float32_words(again.output))
    ens.step(DT, n_steps=K, download=False)
    again = ens.tuner_state().chlorine
    assert np.all(again.n_exec + again.n_held > 1) and not again.commissioned.any()     # the control program is off
    # reset leaves the PI gains: enable the PI again with the commissioned records, reset the tuners, look
    ens.enable_control(pi)
    ens.retune_control(chlorine=wt.PILoop("chlorine_outlet", setpoint=1.0, kp=first.chlorine.kp.clip(0.1, 5.0), ki=1e-3, bias=0.2))
    kp = np.empty((2, 9, N))
    gpu.check(L.wt_ensemble_program_params(ens._h, gpu.WT_PROG_CONTROL, gpu.dptr(kp)))
    ens.reset_tuners()
    gpu.check(L.wt_ensemble_program_params(ens._h, gpu.WT_PROG_CONTROL, gpu.dptr(gains)))
    assert np.array_equal(gains, kp)
    # clear: the switch is off, the holding words stay as they are, nothing tunes any more
    ens.step(DT, n_steps=3, download=False)
    ens.disable_control()
    hr = holding_words(ens)
    ens.clear_tuners()
    assert ens.info(gpu.WT_INFO_TUNE) == 0 and np.array_equal(holding_words(ens), hr)
    with pytest.raises(ValueError, match="no tune program is set"):
        ens.tuner_state()
    ens.step(DT, n_steps=5, download=False)
    assert np.array_equal(holding_words(ens), hr)
    ens.close()
    # n = 33: the n > 32 kernel carries no program
    cfg = wt.ReactorConfiguration(n_zones=33)
    big = wt.ReactorEnsemble([cfg, cfg]); big.set_boundary(wt.BoundaryConditions())
    big.enable_sensors(seed=3); big.enable_plant_io()
    small = wt.tune_block(2, wt.RelayTune("chlorine_outlet", 1.5, 0.25, 0.5))
    assert L.wt_ensemble_tune_set(big._h, gpu.dptr(small)) == gpu.WT_E_STATE
    assert big.info(gpu.WT_INFO_TUNE) == 0
    big.close()


def test_checkpoints_carry_the_program(gpu, wt, full_waves):
    """Mid-experiment: the restored handle, the clone and a mark / rewind each continue with the bits of the handle that
    was never saved, tuner state and commissioned PI records included."""
    n, interval = 5, 3
    R, N, cols, bc = ensemble(wt, n, seed=3)
    here = operating_point(wt, cols, bc, n)
    chlorine, acid = mixed_tuners(wt, cols, here, commission=True)
    pi = wt.PILoop("chlorine_outlet", setpoint=here, kp=0.3, ki=1e-3, bias=0.2)

    def fresh():
        ens = plant(wt, cols, bc, n)
        ens.set_schedule(0, interval)
        ens.enable_control(pi)
        ens.set_tuners(chlorine, acid)
        return ens

    def full(ens):
        params = np.empty((2, 9, N))
        gpu.check(gpu.lib().wt_ensemble_program_params(ens._h, gpu.WT_PROG_CONTROL, gpu.dptr(params)))
        return observed(ens) + (ens.tuner_state().block(), ens.tuner_params(), ens.control_state().block(), params)

    SAVE, REST = 95, K - 95                                  # off a scan boundary, experiments running
    never = fresh(); never.step(DT, n_steps=SAVE, download=False); never.step(DT, n_steps=REST, download=False)
    want = full(never); never.close()
    a = fresh(); a.step(DT, n_steps=SAVE, download=False)
    mid = a.tuner_state().block()
    assert (mid[:, UR.US_PHASE] == UR.RUNNING).any() and (mid[0, UR.US_N_EXEC] > 0).any()
    blob = a.checkpoint()
    bare = wt.ReactorEnsemble(cols, n_zones=n); bare.set_boundary(bc)
    no_io = bare.checkpoint()
    b = plant(wt, cols, bc, n, seed=1); b.restore(blob)
    c = a.clone()
    a.mark()
    for name, ens in (("original", a), ("restored", b), ("clone", c)):
        assert ens.info(gpu.WT_INFO_TUNE) == 1
        ens.step(DT, n_steps=REST, download=False)
        assert_equal_by_reactor(want, full(ens), name, R)
    a.rewind()
    assert np.array_equal(a.tuner_state().block(), mid)
    a.step(DT, n_steps=REST, download=False)
    assert_equal_by_reactor(want, full(a), "rewound", R)
    assert (want[-4][0, UR.US_COMMISSIONED] == 1).any()
    # a blob taken without plant I/O takes the tune program away
    b.restore(no_io)
    assert b.info(gpu.WT_INFO_TUNE) == 0 and b.info(gpu.WT_INFO_PLANT_IO) == 0
    b.enable_sensors(seed=2); b.enable_plant_io()
    assert b.info(gpu.WT_INFO_TUNE) == 0
    with pytest.raises(ValueError, match="no tune program is set"):
        b.tuner_state()
    for ens in (a, b, c, bare):
        ens.close()


@pytest.mark.parametrize("n", ZONES)
def test_disabled_tuners_change_nothing(gpu, wt, full_waves, n):
    """A tune program whose loops are all off against no tune program, beside a running PI program."""
    R, N, cols, bc = ensemble(wt, n, seed=4)
    pi = wt.PILoop("chlorine_outlet", setpoint=np.asarray(cols["initial_chlorine"]) + 2.0, kp=0.3, ki=1e-3, bias=0.2)
    off = wt.RelayTune("chlorine_outlet", 1.5, 0.25, 0.5, enable=0)
    out = []
    for tuned in (False, True):
        ens = plant(wt, cols, bc, n)
        ens.set_schedule(0, 7)
        ens.enable_control(pi)
        if tuned:
            ens.set_tuners(off, wt.RelayTune("pH_outlet", 7.2, 0.25, 0.5, enable=0))
        ens.step(DT, n_steps=100, download=False)
        out.append(observed(ens) + (ens.control_state().block(),))
        if tuned:
            assert not ens.tuner_state().block().any()
        ens.close()
    assert_equal_by_reactor(out[0], out[1], "disabled tuners", R)
