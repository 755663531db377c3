"""The installation of the fused sensor suite (``set_installation``): every reactor's own sample lines and instrument
installation, against the oracle with the same installation (tests/install_ref.py, which tests/test_install_cpu.py
holds to the reference's own sensor classes).

The method of test_gpu_sensor_edges.py, whose helpers this file uses: the suite is enabled at t = 0, the clock moved on
by the 1 800 s of the pH warm-up, and the oracle suite of every reactor is fed the device's own recorded per-step state
(one fused call under ``record(1, steps)``), rounded to fp32, at the device's fp64 times.  Bounds: values within
|dv| / (1 + |v|) < 2e-5; NaN and 0.0 positions, statuses and faults equal at every read; the fp64 ageing accumulators
of ``sensor_health()`` to rtol 1e-6 / atol 1e-9.  Shapes: 32, 8, 3 and 1 reactors per wavefront, the last on the
n > 32 kernel.

Observed on an MI355X: max |dv| / (1 + |v|) 4.9e-7 over all tests of this file (delays 4.9e-7, branches 4.9e-7, bubbles
3.6e-7, ageing 2.2e-7, mid-run change 4.7e-7, mixed 3.0e-7); statuses, faults, NaN and 0.0 positions equal at every
read; the ageing accumulators at most 1e-10 of their tolerance; the bubble windows hold 11 to 126 sensors NaN for good
and 8 to 11 flowmeter dropouts."""
import numpy as np
import pytest

import install_ref as IR
import sensor_oracle as SO
import test_gpu_sensor_edges as E
from program_helpers import full_waves, everything, pi_loops  # noqa: F401  (full_waves is a fixture)

# full_waves: 64 // n reactors in every wavefront, as a large ensemble is packed, so that the sensor lanes of a pass
# belong to 32, 8, 3 and 1 reactors (a small ensemble is otherwise spread out, down to one reactor per wavefront)
pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("full_waves")]
SHAPES = [(2, 33), (8, 9), (20, 4), (40, 3)]
F = {k: i for i, k in enumerate(IR.PARAM_ROWS)}
# (volume mL, flow mL/min) of a line by its delay: 90 s, 0 s (no flow), 12 s, 50 s, 9.96 s
LINES = [(750.0, 500.0), (250.0, 0.0), (100.0, 500.0), (250.0, 300.0), (83.0, 500.0)]
assert [SO.SampleLine(v, f).transport_delay_s for v, f in LINES] == [90.0, 0.0, 12.0, 50.0, 9.96]


def suites_of(plant, base, block, seed=E.SEED):
    cols = plant[0]
    return [IR.InstalledSuite(float(cols["flow_rate"][r]), float(cols["initial_chlorine"][r]), float(cols["temperature"][r]), 0.0,
                              seed, base + r, block[:, r]) for r in range(block.shape[1])]


def compare(label, dev, ref):
    """E.compare, and the positions of 0.0 (the flowmeter's dropouts) equal as well."""
    worst = E.compare(label, dev, ref)
    assert np.array_equal(dev[0] == 0.0, ref[0] == 0.0), label
    return worst


def run(wt, n, plant, base, inst, calls, one_step=False, seed=E.SEED):
    """E.run_calls with an installation set before the first read (None: no call at all)."""
    steps = sum(k for k, _ in calls)
    ens = E.open_warm(wt, n, plant, base, steps, seed=seed)
    if inst is not None:
        ens.set_installation(inst)
    for k, dt in calls:
        for _ in range(k if one_step else 1):
            ens.step(dt, n_steps=1 if one_step else k, download=False)
    traj = ens.trajectory()
    assert len(traj) == steps and not traj.status.any()
    return ens, traj, E.history_of(ens, steps)


def calm_plant(wt, n, N):
    """The plant of test_gpu_sensor_edges.py::test_long_horizon_ageing for every reactor, which steps of 3 600 s do not
    trouble: the default configuration at pH 7.2 under chlorine dosing and a warm inlet; the reactors differ in their
    chlorine so that no two analysers read alike."""
    cfg = wt.ReactorConfiguration(n_zones=n, initial_pH=7.2)
    cols = {k: np.full(N, float(getattr(cfg, k))) for k in ("initial_pH", "initial_chlorine", "temperature", "flow_rate", "alkalinity", "total_carbonate")}
    cols["initial_chlorine"] = cols["initial_chlorine"] + 0.05 * np.arange(N)
    bc = wt.boundary_block(wt.BoundaryConditions(inlet_flow_rate=5.0, inlet_pH=7.5, chlorine_flow_rate=0.3, inlet_temperature=24.0), N)
    rep = lambda k: np.repeat(cols[k][:, None], n, axis=1)
    return cols, bc, (rep("initial_pH"), rep("initial_chlorine"), rep("temperature"))


def health(ens):
    return tuple(ens.sensor_health().values())


def delays_installation(wt, N):
    """Every reactor its own pair of lines, different on the two lines; reactor 0 has the 90 s inlet line."""
    r = np.arange(N)
    lin, lout = np.array(LINES)[r % 5], np.array(LINES)[(r + 1 + r // 5) % 5]
    return wt.Installation(inlet_line_volume_mL=lin[:, 0], inlet_line_flow_mL_min=lin[:, 1],
                           outlet_line_volume_mL=lout[:, 0], outlet_line_flow_mL_min=lout[:, 1])


def branches_installation(wt, N):
    """r % 3 == 0: all three thresholds exactly (no branch); 1: all three just beyond; 2: one just beyond, in turn."""
    r = np.arange(N)
    one = (r % 3 == 2) * (1 + (r // 3) % 3)                                # 1 stagnant, 2 grounding, 3 vibration
    beyond = r % 3 == 1
    return wt.Installation(flow_velocity=np.where(beyond | (one == 1), 0.09, 0.1), grounding_quality=np.where(beyond | (one == 2), 0.79, 0.8),
                           pipe_vibration_g=np.where(beyond | (one == 3), 0.21, 0.2))


def mixed_installation(wt, N):
    """Delays, all four effects on two reactors of three (bubbles at 1/128 per read), another ambient temperature."""
    r = np.arange(N)
    d = delays_installation(wt, N)
    d.flow_velocity = np.where(r % 3 == 0, 0.5, 0.05)
    d.air_bubble_frequency = np.where(r % 3 == 0, 0.0, 0.46875)
    d.grounding_quality = np.where(r % 3 == 0, 0.9, 0.4)
    d.pipe_vibration_g = np.where(r % 3 == 0, 0.1, 0.5)
    d.ambient_temperature = 18.0 + r
    return d


# ---------------------------------------------------------------- 1. defaults change nothing
@pytest.mark.parametrize("n,N", SHAPES)
def test_defaults_change_nothing(gpu, wt, n, N):
    """No call at all, ``set_installation(Installation())``, and a non-default installation cleared before the first
    read: the same bits over the whole run -- history, last readings, sensor_health() -- at dt = 0.8 s, where the line's
    winner hangs on the last bits of t - delay."""
    plant = E.moving_plant(wt, n, N)
    calls = [(30, 0.8)]
    ens, traj, ref = run(wt, n, plant, 0, None, calls)
    assert ens.info(gpu.WT_INFO_INSTALL) == 0 and np.array_equal(ens.installation(), wt.installation_block(N))
    ref_health = health(ens)
    ens.close()
    ens, _, dev = run(wt, n, plant, 0, wt.Installation(), calls)
    assert ens.info(gpu.WT_INFO_INSTALL) == 1 and np.array_equal(ens.installation(), wt.installation_block(N))
    assert E.same_bits(dev, ref) and E.same_bits(health(ens), ref_health)
    ens.close()
    ens = E.open_warm(wt, n, plant, 0, 30)
    ens.set_installation(mixed_installation(wt, N))
    assert ens.info(gpu.WT_INFO_INSTALL) == 1 and not np.array_equal(ens.installation(), wt.installation_block(N))
    ens.clear_installation()
    assert ens.info(gpu.WT_INFO_INSTALL) == 0 and np.array_equal(ens.installation(), wt.installation_block(N))
    ens.step(0.8, n_steps=30, download=False)
    assert E.same_bits(E.history_of(ens, 30), ref) and E.same_bits(health(ens), ref_health)
    assert np.array_equal(ens.trajectory().pH, traj.pH)
    ens.close()


# ---------------------------------------------------------------- 2. per-reactor delays
@pytest.mark.parametrize("n,N", SHAPES)
@pytest.mark.parametrize("dt,steps", [(0.5, 70), (0.8, 60), (1.0, 40), (7.5, 30)])
def test_per_reactor_delays(gpu, wt, n, N, dt, steps):
    """Every reactor its own pair of delays out of 90, 0, 12, 50 and 9.96 s.  0.5 s: the line's 100 entries (two pushes
    per read) span 25 s and wrap after 50 reads, so the 90 s, 50 s and, after the wrap, no other line takes the oldest
    entry held; 0.8 s: 12 / 0.8 = 15 and 50 / 0.8 = 62.5, an exact hit and a tie that the last bits of t - delay
    settle; 7.5 s: 90 s is twelve reads back, 9.96 and 12 s between two timestamps.  A delay of 0 returns the line's
    first entry at t: to the RTD that is the pH electrode's sample, as in the reference."""
    plant = E.moving_plant(wt, n, N)
    inst = delays_installation(wt, N)
    block = wt.installation_block(N, inst)
    ens, traj, dev = run(wt, n, plant, 0, inst, [(steps, dt)])
    assert np.array_equal(ens.installation(), block)
    ens.close()
    suites = suites_of(plant, 0, block)
    assert [s.lines[0].transport_delay_s for s in suites[:3]] == [90.0, 0.0, 12.0]
    ref = E.oracle_reads(suites, traj)
    if dt == 0.5:
        assert steps * 2 > 100 and 100 * dt / 2 < 90.0               # (the ring has wrapped and is shorter than the delay)
    compare(f"delays n = {n} N = {N} dt = {dt}", dev, ref)


# ---------------------------------------------------------------- 3. each installation branch, and the thresholds
@pytest.mark.parametrize("n,N", SHAPES)
def test_branches_and_thresholds(gpu, wt, n, N):
    """A reactor at exactly 0.1 m/s, 0.8 and 0.2 g reads bit for bit what the same reactor reads without an
    installation; just beyond (0.09, 0.79, 0.21; all three, or one in turn) it differs and matches the oracle."""
    plant = E.moving_plant(wt, n, N)
    inst = branches_installation(wt, N)
    block = wt.installation_block(N, inst)
    ens, traj, dev = run(wt, n, plant, 0, inst, [(36, 1.0)])
    ens.close()
    ens0, traj0, dev0 = run(wt, n, plant, 0, None, [(36, 1.0)])
    ens0.close()
    assert np.array_equal(traj.pH, traj0.pH)
    at = np.arange(N) % 3 == 0
    assert all(np.array_equal(a[:, :, at], b[:, :, at], equal_nan=True) for a, b in zip(dev, dev0))
    for r in np.nonzero(~at)[0]:
        assert not np.array_equal(dev[0][:, :, r], dev0[0][:, :, r], equal_nan=True), r
    ref = E.oracle_reads(suites_of(plant, 0, block), traj)
    compare(f"branches n = {n} N = {N}", dev, ref)


# ---------------------------------------------------------------- 4. bubbles
# reactor_base by shape: the first multiple of N at which the oracle, under the plant's initial values as constant
# taps, counts at least eight flowmeter dropouts in the window (a reactor has about one before its flowmeter meets a
# bubble of its own).  The test counts again on the oracle's run over the device's trajectory.
BUBBLE_BASE = {(2, 33): 0, (8, 9): 180, (20, 4): 180, (40, 3): 180}
BUBBLE_READS = 120


def bubbles_installation(wt, N):
    return wt.Installation(air_bubble_frequency=np.array([0.0, 0.46875, 3.75])[np.arange(N) % 3])


@pytest.mark.parametrize("n,N", SHAPES)
def test_bubbles(gpu, wt, n, N):
    """Bubble frequencies 0, 0.46875 and 3.75 per minute (0, 1/128 and 1/16 per read) by reactor.  A hit makes the sensor
    NaN for good (the reference's lag keeps it) while it goes on drawing; the flowmeter's own draw drops single reads
    to 0.0.  The onset read of every NaN sensor and every dropout equal the oracle's (the NaN and 0.0 patterns are
    compared at every read)."""
    plant = E.quiet_plant(wt, n, N)
    base = BUBBLE_BASE[(n, N)]
    inst = bubbles_installation(wt, N)
    block = wt.installation_block(N, inst)
    ens, traj, dev = run(wt, n, plant, base, inst, [(BUBBLE_READS, 1.0)])
    suites = suites_of(plant, base, block)
    ref = E.oracle_reads(suites, traj)
    ov = ref[0]
    gone = np.isnan(ov[-1]) & (block[F["air_bubble_frequency"]] > 0)[None, :]
    dropouts = int((ov[:, SO.S_FLOW] == 0.0).sum())
    print(f"bubbles n = {n} N = {N}: {int(gone.sum())} sensors NaN for good, {dropouts} flowmeter dropouts, {int(np.isfinite(ov[-1]).sum())} sensors alive at the end")
    assert gone.sum() >= 5 and dropouts >= 5 and np.isfinite(ov[-1]).any()
    assert np.isfinite(ov[-1][:, np.arange(N) % 3 == 0]).any()
    for i, r in zip(*np.nonzero(gone)):                                  # NaN from its onset to the end
        onset = int(np.argmax(np.isnan(ov[:, i, r])))
        assert np.isnan(ov[onset:, i, r]).all() and np.isnan(dev[0][onset:, i, r]).all() and (onset == 0 or np.isfinite(dev[0][onset - 1, i, r]))
    compare(f"bubbles n = {n} N = {N}", dev, ref)
    E.compare_health(f"bubbles n = {n} N = {N}", ens, suites)
    ens.close()


# ---------------------------------------------------------------- 5. stagnant ageing and ambient temperature
@pytest.mark.parametrize("n,N", SHAPES)
def test_stagnant_ageing_and_ambient(gpu, wt, n, N):
    """Eight steps of 3 600 s: odd reactors at 0.05 m/s age their pH electrodes at (bio + 100 * 0.0001) per day and
    their amperometric cell at 0.05 per day, even ones at the suite's rates; every reactor has its own ambient
    temperature, which moves the RTDs against a run without an installation in the direction of 30 degC - ambient."""
    plant = calm_plant(wt, n, N)
    r = np.arange(N)
    ambient = np.where(r == 0, 30.0, 5.0 + 9.0 * r)
    inst = wt.Installation(flow_velocity=np.where(r % 2 == 1, 0.05, 0.5), ambient_temperature=ambient)
    block = wt.installation_block(N, inst)
    calls = [(8, 3600.0)]
    ens, traj, dev = run(wt, n, plant, 0, inst, calls)
    suites = suites_of(plant, 0, block)
    ref = E.oracle_reads(suites, traj)
    compare(f"ageing n = {n} N = {N}", dev, ref)
    E.compare_health(f"ageing n = {n} N = {N}", ens, suites)
    h = ens.sensor_health()
    ens.close()
    alive = np.isfinite(ref[0][-1])
    for i, fast, slow in ((SO.S_CL_IN, 0.05, 0.01), (SO.S_PH_IN, 0.011, 0.002)):
        per_day = h["slow0"][i] / (7 * 3600.0 / 86400.0)
        ok = alive[i]
        assert ok[1::2].any() and ok[0::2].any()
        assert np.allclose(per_day[1::2][ok[1::2]], fast, rtol=1e-9) and np.allclose(per_day[0::2][ok[0::2]], slow, rtol=1e-9)
    ens0, _, dev0 = run(wt, n, plant, 0, None, calls)
    ens0.close()
    for i in (SO.S_T_IN, SO.S_T_OUT):
        d = dev[0][-1, i] - dev0[0][-1, i]
        ok = np.isfinite(d) & (r % 2 == 0) & (r > 0)                     # (an even reactor differs from the plain run in its ambient only)
        assert d[0] == 0.0 or not np.isfinite(d[0])                      # (reactor 0: 0.5 m/s and 30 degC, the suite's build)
        assert ok.any()
        assert np.all(np.sign(d[ok]) == np.sign(30.0 - ambient[ok])) and np.all(np.abs(d[ok]) >= 0.009 * np.abs(30.0 - ambient[ok]))


# ---------------------------------------------------------------- 6. a mid-run change
@pytest.mark.parametrize("n,N", SHAPES)
def test_mid_run_change(gpu, wt, n, N):
    """The inlet line goes 12 s -> 50 s -> 0 s and the outlet line 12 s -> 0 s -> 50 s between calls; the oracle's lines
    get ``transport_delay_s`` assigned at the same reads and keep their buffers.  The move to 50 s takes the target
    back behind the device's cursor."""
    plant = E.moving_plant(wt, n, N)
    line = lambda i: dict(zip(("volume", "flow"), LINES[i]))
    def installation(a, b):
        return wt.Installation(inlet_line_volume_mL=LINES[a][0], inlet_line_flow_mL_min=LINES[a][1],
                               outlet_line_volume_mL=LINES[b][0], outlet_line_flow_mL_min=LINES[b][1], ambient_temperature=25.0)
    phases = [(30, (2, 2)), (40, (3, 1)), (30, (1, 3))]
    steps = sum(k for k, _ in phases)
    ens = E.open_warm(wt, n, plant, 0, steps)
    for k, (a, b) in phases:
        ens.set_installation(installation(a, b))
        ens.step(1.0, n_steps=k, download=False)
    traj = ens.trajectory()
    assert len(traj) == steps and not traj.status.any()
    dev = E.history_of(ens, steps)
    ens.close()
    suites = suites_of(plant, 0, wt.installation_block(N, installation(2, 2)))
    parts, first = [], 0
    for k, (a, b) in phases:
        for s in suites:
            s.set_delays(SO.SampleLine(*LINES[a]).transport_delay_s, SO.SampleLine(*LINES[b]).transport_delay_s)
        window = type(traj)(*(getattr(traj, f)[first:first + k] for f in ("time", "pH", "chlorine", "temperature", "flow_rate", "status")))
        parts.append(E.oracle_reads(suites, window))
        first += k
    ref = tuple(np.concatenate([p[j] for p in parts]) for j in range(3))
    compare(f"mid-run change n = {n} N = {N}", dev, ref)


# ---------------------------------------------------------------- 7. invariances
@pytest.mark.parametrize("n,N", SHAPES)
def test_one_fused_call_equals_one_step_calls(gpu, wt, n, N):
    plant = E.moving_plant(wt, n, N)
    inst = mixed_installation(wt, N)
    a, ta, da = run(wt, n, plant, 0, inst, [(40, 0.8)])
    b, tb, db = run(wt, n, plant, 0, inst, [(40, 0.8)], one_step=True)
    assert E.same_bits(da, db) and E.same_bits(health(a), health(b)) and np.array_equal(ta.pH, tb.pH)
    assert np.isnan(da[0][-1]).any() and np.isfinite(da[0][-1]).any()
    ref = E.oracle_reads(suites_of(plant, 0, wt.installation_block(N, inst)), ta)
    compare(f"mixed n = {n} N = {N}", da, ref)
    a.close(); b.close()


@pytest.mark.parametrize("n,N", [(8, 9), (40, 3)])
def test_plant_io_with_bubbles_fused_equals_chunked(gpu, wt, n, N):
    """Plant I/O with both PI loops under bubbles at 1/16 per read on every reactor: one fused call of K scans equals K
    one-scan calls, bitwise.  The NaN of a bubbled pH_outlet or chlorine_outlet reaches the scan: the input image shows
    it as the reference's ``safe_value`` does, as 0.0, and the loop on it holds -- its held count goes up at every scan
    from then on and its output stays."""
    cols, bc, (pH, Cl, T) = E.quiet_plant(wt, n, N)
    K = 40

    def open_():
        ens = wt.ReactorEnsemble(cols, n_zones=n)
        ens.set_boundary(bc)
        ens.enable_sensors(seed=E.SEED, history=K)
        ens.set_state(pH, Cl, T, np.array(ens.state.time) + E.WARM)
        ens.enable_plant_io()
        ens.set_schedule(chunk_steps=1)
        ens.set_installation(wt.Installation(air_bubble_frequency=3.75))
        chlorine, acid = pi_loops(wt, cols)
        ens.enable_control(chlorine=chlorine, acid=acid)
        return ens

    a = open_()
    a.step(1.0, n_steps=K, download=False)
    b = open_()
    held, out = [], []
    for _ in range(K):
        b.step(1.0, n_steps=1, download=False)
        st = b.control_state()
        held.append(np.stack([st.chlorine.n_held, st.acid.n_held])); out.append(np.stack([st.chlorine.output, st.acid.output]))
    ea, eb = everything(a, programs=("control",)), everything(b, programs=("control",))
    for i, (x, y) in enumerate(zip(ea, eb)):
        assert np.array_equal(x, y, equal_nan=True), i
    assert E.same_bits(E.history_of(a, K), E.history_of(b, K))
    hv = E.history_of(a, K)[0][:, [SO.S_CL_OUT, SO.S_PH_OUT]]           # (read, loop, reactor)
    dead = np.isnan(hv[-1])
    assert dead.sum() >= 5
    image = a.input_image()[0]
    regs = wt.ReactorEnsemble.INPUT_REGISTERS
    for l, name in enumerate(("chlorine_outlet", "pH_outlet")):
        shown = wt.ReactorEnsemble.decode_float32(image[:, regs[name]:regs[name] + 2])
        assert np.all(shown[dead[l]] == 0.0) and np.all(shown[~dead[l]] != 0.0), name     # safe_value (__main__.py:166-224): NaN -> 0.0
    held, out = np.array(held), np.array(out)
    for l, r in zip(*np.nonzero(dead)):
        onset = max(1, int(np.argmax(np.isnan(hv[:, l, r]))))
        assert np.isnan(hv[onset:, l, r]).all()
        assert np.all(np.diff(held[onset - 1:, l, r]) == 1) and np.all(out[onset:, l, r] == out[onset - 1, l, r]), (l, r)
    a.close(); b.close()


@pytest.mark.parametrize("n,N", SHAPES)
def test_checkpoint_clone_and_rewind_carry_the_installation(gpu, wt, n, N):
    plant = E.moving_plant(wt, n, N)
    inst = mixed_installation(wt, N)
    block = wt.installation_block(N, inst)
    whole, _, ref = run(wt, n, plant, 0, inst, [(20, 0.8), (20, 0.8)])
    ref_health = health(whole)
    whole.close()
    ens = E.open_warm(wt, n, plant, 0, 40)
    ens.set_installation(inst)
    ens.step(0.8, n_steps=20, download=False)
    blob = ens.checkpoint()
    twin = ens.clone()
    ens.mark()
    ens.clear_installation()
    ens.step(0.8, n_steps=3, download=False)
    ens.rewind()
    fresh = E.open_warm(wt, n, plant, 0, 40)
    assert fresh.info(gpu.WT_INFO_INSTALL) == 0
    fresh.restore(blob)
    for h in (ens, twin, fresh):
        assert h.info(gpu.WT_INFO_INSTALL) == 1 and np.array_equal(h.installation(), block)
        h.step(0.8, n_steps=20, download=False)
        assert E.same_bits(E.history_of(h, 40), ref) and E.same_bits(health(h), ref_health)
        assert np.array_equal(h.installation(), block)
        h.close()


def test_info_and_refusals(gpu, wt):
    cols, bc = wt.make_ensemble(4)
    ens = wt.ReactorEnsemble(cols, n_zones=5)
    ens.set_boundary(bc)
    assert ens.info(gpu.WT_INFO_INSTALL) == 0
    import ctypes
    blk = wt.installation_block(4)
    for refused in (lambda: ens.set_installation(wt.Installation()), ens.installation):
        with pytest.raises(ValueError) as ei:
            refused()
        assert str(ei.value) == "the sensor suite is not enabled (wt_ensemble_sensors_enable)"     # the service program's words
    assert gpu.lib().wt_ensemble_install_set(ens._h, gpu.dptr(blk)) == gpu.WT_E_STATE
    assert gpu.lib().wt_ensemble_install_set(ens._h, None) == gpu.WT_E_ARG and gpu.lib().wt_ensemble_install_get(ens._h, None) == gpu.WT_E_ARG
    assert gpu.lib().wt_ensemble_install_clear(ctypes.c_void_p()) == gpu.WT_E_ARG
    ens.clear_installation()
    ens.enable_sensors(seed=1)
    assert ens.info(gpu.WT_INFO_INSTALL) == 0
    ens.set_installation(wt.Installation(flow_velocity=0.05))
    assert ens.info(gpu.WT_INFO_INSTALL) == 1 and np.all(ens.installation()[F["flow_velocity"]] == 0.05)
    with pytest.raises(ValueError, match=r"inlet_line_volume_mL and flow give a delay of 91 s or more.*\(reactor 3\)"):
        ens.set_installation(wt.Installation(inlet_line_volume_mL=np.array([250.0, 250.0, 757.5, 758.4])))
    assert ens.info(gpu.WT_INFO_INSTALL) == 1 and np.all(ens.installation()[F["flow_velocity"]] == 0.05)     # a refused block changes nothing
    ens.clear_installation()
    assert ens.info(gpu.WT_INFO_INSTALL) == 0 and np.array_equal(ens.installation(), wt.installation_block(4))
    with pytest.raises(gpu.WtError) as ei:
        ens.info(99)
    assert ei.value.code == gpu.WT_E_ARG
    assert set(vars(ens)) == set(vars(wt.ReactorEnsemble(cols, n_zones=5)))
    ens.close()
