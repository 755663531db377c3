"""NEXT-2 / NEXT-3 on the GPU: the per-reactor Modbus register image and the command path against
oracle/plc_oracle.py (pinned by the reference's encoder / register map, tests/golden/g8_modbus.json)."""
import numpy as np
import pytest

from program_helpers import SENSOR_NS, equals_spread, packing, ragged_size  # noqa: F401  (packing: a fixture)

pytestmark = pytest.mark.gpu
# The tests of this module at N = 2048, 1024, 512 and 64 run spread: two, one and one reactors of eight zones per wavefront
# on a card with 1 024 wavefront slots, and 64 wavefronts of one four-zone reactor.  The ``_packed`` tests run the same
# bodies with full wavefronts: five wavefronts of 64 // n reactors and a lone one at every zone
# count of SENSOR_NS, every reactor compared, and the packed images and boundaries equal the spread run's bit for bit.


def _ensemble(wt, N, n=8, seed=99, base=0, packing=None):
    cols, bc = wt.make_ensemble(N)
    ens = wt.ReactorEnsemble(cols, n_zones=n)
    if packing is not None:
        packing.place(ens)
    ens.set_boundary(bc)
    ens.enable_sensors(seed=seed, reactor_base=base)
    ens.enable_plant_io()
    return ens, cols, bc


def test_input_image_vs_oracle(gpu, wt):
    """Image after 400 scans of one step (pH still warming up -> 0.0, ~6 % of sensors faulted) equals the
    oracle's update_modbus_inputs applied to the device's own readings, word for word."""
    N = 2048
    input_image_vs_oracle(wt, N, 8, 400, lambda f: list(range(0, N, 37)) + list(np.nonzero(f.any(axis=0))[0][:40]))


IMAGE_BASE, IMAGE_SCANS = 520, 60      # with this module's seed the stream of reactor 522 puts a fault code on pH_outlet within 60 reads


@pytest.mark.parametrize("n", SENSOR_NS)
@pytest.mark.parametrize("packing", ["packed"], indirect=True)
def test_input_image_vs_oracle_packed(gpu, wt, monkeypatch, n, packing):
    """Full wavefronts: the scan lane of slot ``sl`` packs the readings the sensor lanes left for that slot, whichever
    pass they ran in.  60 scans of one step, reactors 520 ... of the sensor streams (so that a fault code is in the
    image: asserted, as is a NaN reading), every reactor against the oracle, and the image, its flags and the readings
    equal to the spread run's."""
    R, N = ragged_size(n)
    run = lambda p: input_image_vs_oracle(wt, N, n, IMAGE_SCANS, lambda f: list(range(N)), p, IMAGE_BASE)
    equals_spread(monkeypatch, packing, ("input image", n), n, run(packing), run)


def input_image_vs_oracle(wt, N, n, scans, reactors, packing=None, base=0):
    """``scans`` scans of one step; the image of ``reactors(fault codes)`` against the oracle.  Returns the image, its
    flags and the readings, reactor last."""
    import plc_oracle as PO
    ens, cols, bc = _ensemble(wt, N, n=n, base=base, packing=packing)
    ens.set_schedule(2, 1)
    ens.step(1.0, n_steps=scans)
    v, s, f = ens.sensor_readings()
    img, ok = ens.input_image()
    assert ok.all() and f.any() and np.isnan(v).any()
    for r in reactors(f):
        io = PO.PlantIO()
        assert io.update_inputs([float(x) for x in v[:, r]], [int(x) for x in f[:, r]], scans - 1.0)   # sim_time lags one dt
        ir, di = ens.input_blocks(r, img)
        assert ir == io.ir[:200] and di == io.di[:100], r
    if packing is not None:
        packing.check(ens)
    ens.close()
    return img.T, np.asarray(ok).T, v, s, f


def test_scan_interval_and_time_register(gpu, wt):
    """chunked scans publish the last step of the launch; simulation_time = (steps - 1) * dt accumulated."""
    import plc_oracle as PO
    N = 512
    ens, cols, bc = _ensemble(wt, N)
    ens.set_schedule(1, 25)
    ens.step(0.5, n_steps=60)                     # launches of 25, 25, 10 steps
    img, ok = ens.input_image()
    t = 0.0
    for _ in range(59):
        t += 0.5
    assert np.all(wt.ReactorEnsemble.decode_float32(img[:, 16:18]) == np.float32(t))
    v, s, f = ens.sensor_readings()
    io = PO.PlantIO(); io.update_inputs([float(x) for x in v[:, 5]], [int(x) for x in f[:, 5]], t)
    assert ens.input_blocks(5, img)[0] == io.ir[:200]
    ens.close()


def test_command_path_vs_oracle(gpu, wt):
    """Holding image -> boundary conditions: validate_flow_rate clamps, NaN -> 0, inlet only if > 0.1;
    acts from the scan after the write; untouched reactors keep their boundary."""
    command_path_vs_oracle(wt, 1024, 8)


@pytest.mark.parametrize("n", SENSOR_NS)
@pytest.mark.parametrize("packing", ["packed"], indirect=True)
def test_command_path_vs_oracle_packed(gpu, wt, monkeypatch, n, packing):
    """Full wavefronts: five of 64 // n reactors and a lone one; the first half of the reactors is written (the
    non-finite, negative and out-of-range commands at the head of the list among them, in neighbouring scan lanes), the
    other half keeps its boundary.  The bounds on how many rows change and how many reactors are dosed are the 1 024-reactor
    test's, scaled to N.  The boundary after the scan and the state after the dosed run equal the spread run's."""
    R, N = ragged_size(n)
    run = lambda p: command_path_vs_oracle(wt, N, n, p)
    equals_spread(monkeypatch, packing, ("command path", n), n, run(packing), run)


def command_path_vs_oracle(wt, N, n, packing=None):
    """Returns the boundary after the scan that applied the commands and the inlet-zone pH after the dosed run."""
    import plc_oracle as PO
    ens, cols, bc = _ensemble(wt, N, n=n, packing=packing)
    ens.set_schedule(1, 1)
    ens.step(1.0, n_steps=2)
    assert np.array_equal(ens.boundary()[[0, 4, 6]], np.stack([bc[0], np.zeros(N), np.zeros(N)]))   # zeros in the registers: dosing off
    rng = np.random.default_rng(5)
    special = np.array([np.nan, np.inf, -np.inf, -1.0, 0.0, 0.1, 0.100001, 0.05, 2.0, 2.5, 1.0, 1.5, 20.0, 25.0, 1e30, -1e30, 1e-40])
    half = N // 2
    if half >= special.size:
        acid = np.concatenate([special, rng.uniform(-0.5, 3.0, N - special.size)])
        chl = np.concatenate([special[::-1], rng.uniform(-0.5, 1.5, N - special.size)])
        inlet = np.concatenate([np.roll(special, 5), rng.uniform(-1.0, 25.0, N - special.size)])
    else:
        # fewer written reactors than special values: every second reactor takes one, from ``n`` values into the list on
        # (so that the small ensembles of different zone counts share the list out), the others a random command
        def mixed(values, lo, hi):
            out = rng.uniform(lo, hi, N)
            out[::2] = np.resize(np.roll(values, -n), out[::2].size)
            return out
        acid, chl, inlet = mixed(special, -0.5, 3.0), mixed(special[::-1], -0.5, 1.5), mixed(np.roll(special, 5), -1.0, 25.0)
    ens.write_commands(acid[:half], chl[:half], inlet[:half], first_reactor=0)
    before = ens.boundary()
    assert np.array_equal(before[[0, 4, 6]], np.stack([bc[0], np.zeros(N), np.zeros(N)]))           # not yet: no scan since the write
    ens.step(1.0, n_steps=1)
    after = ens.boundary()
    exp = np.array(bc, copy=True); exp[4] = 0.0; exp[6] = 0.0
    for r in range(half):
        io = PO.PlantIO()
        io.write_holding("acid_flow_rate", float(acid[r])); io.write_holding("chlorine_flow_rate", float(chl[r])); io.write_holding("inlet_flow_rate", float(inlet[r]))
        col = list(exp[:, r]); PO.apply_boundary_conditions(col, io.read_commands()); exp[:, r] = col
    assert np.array_equal(after, exp)
    assert (after[0, :half] != bc[0, :half]).sum() > 300 * half / 512 and np.array_equal(after[:, half:], exp[:, half:])
    # and the physics sees it: dosing acid lowers the inlet-zone pH relative to an undosed twin
    ens.step(1.0, n_steps=120)
    twin, _, _ = _ensemble(wt, N, n=n, packing=packing)
    twin.set_schedule(1, 1); twin.step(1.0, n_steps=123)
    dosed = np.nonzero(after[4, :half] > 0.5)[0]
    pH = ens.state.pH
    assert dosed.size > 50 * half / 512 and np.all(pH[dosed, 0] < twin.state.pH[dosed, 0] - 1e-3)
    if packing is not None:
        packing.check(ens); packing.check(twin)
    ens.close(); twin.close()
    return after, pH[:, 0]


def test_closed_loop_vs_reference_order(gpu, wt):
    """A host-side proportional controller closes the loop through the images every step; the same
    loop run with the oracle's PlantIO on the device's readings produces the same boundary history."""
    closed_loop_vs_reference_order(wt)


@pytest.mark.parametrize("packing", ["packed"], indirect=True)
def test_closed_loop_vs_reference_order_packed(gpu, wt, monkeypatch, packing):
    """64 reactors of four zones as four full wavefronts of sixteen (two sensor passes each); the boundary history
    equals the spread run's (64 wavefronts of one reactor)."""
    run = lambda p: closed_loop_vs_reference_order(wt, p)
    equals_spread(monkeypatch, packing, "closed loop", 4, run(packing), run)


def closed_loop_vs_reference_order(wt, packing=None):
    """Returns the boundary after every step, reactor last."""
    import plc_oracle as PO
    N = 64
    ens, cols, bc = _ensemble(wt, N, n=4, packing=packing)
    history = []
    ens.set_schedule(1, 1)
    ios = [PO.PlantIO() for _ in range(N)]
    exp = np.array(bc, copy=True)
    for k in range(90):
        ens.step(1.0, n_steps=1, fused=False)
        v, s, f = ens.sensor_readings()
        img, _ = ens.input_image()
        for r in range(N):                                   # reference order: update inputs, then read commands
            ios[r].update_inputs([float(x) for x in v[:, r]], [int(x) for x in f[:, r]], float(k))
            col = list(exp[:, r]); PO.apply_boundary_conditions(col, ios[r].read_commands()); exp[:, r] = col
        assert np.array_equal(ens.boundary(), exp), k
        history.append(exp.copy())
        assert all(ens.input_blocks(r, img)[0] == ios[r].ir[:200] for r in (0, 17, 63))
        # the "PLC": chlorine dosing proportional to the shortfall of the outlet DPD reading (register 8-9) from 1.5 mg/L
        cl_out = wt.ReactorEnsemble.decode_float32(img[:, 8:10]).astype(np.float64)
        cmd_cl = np.clip(0.4 * (1.5 - cl_out), -0.2, 1.3)
        cmd_in = np.where(np.arange(N) % 3 == 0, 6.0 + 0.01 * k, 0.0)
        ens.write_commands(np.full(N, 0.05), cmd_cl, cmd_in)
        for r in range(N):
            ios[r].write_holding("acid_flow_rate", 0.05); ios[r].write_holding("chlorine_flow_rate", float(cmd_cl[r])); ios[r].write_holding("inlet_flow_rate", float(cmd_in[r]))
    assert ens.boundary()[6].max() > 0.1
    if packing is not None:
        packing.check(ens)
    ens.close()
    return (np.array(history),)


def test_set_boundary_wins_over_earlier_commands(gpu, wt):
    """With plant I/O on, every PLC scan rewrites boundary rows 0 / 4 / 6 on the device; a later ``set_boundary`` with
    the very block the host sent before must still be uploaded (the host's copy is no longer what the device holds)."""
    cols, bc = wt.make_ensemble(64)
    ens = wt.ReactorEnsemble(cols, n_zones=4)
    ens.set_boundary(bc)
    ens.enable_sensors(seed=5); ens.enable_plant_io()
    ens.write_commands(1.5, 0.75, 9.0)
    ens.step(1.0, n_steps=3)
    assert np.allclose(ens.boundary()[[4, 6, 0]], np.array([[1.5], [0.75], [9.0]]))
    for _ in range(2):                       # the first and every later identical call restore the host's rows
        ens.write_commands(0.0, 0.0, 0.0)    # (0 inlet command = "leave the inlet alone", so nothing overrides it again)
        ens.set_boundary(bc)
        assert np.array_equal(ens.boundary(), bc)
        ens.write_commands(1.5, 0.75, 9.0)
        ens.step(1.0, n_steps=2)
        assert np.allclose(ens.boundary()[[4, 6, 0]], np.array([[1.5], [0.75], [9.0]]))
    ens.close()
