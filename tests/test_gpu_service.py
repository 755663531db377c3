"""The sensor service program on the GPU: the fused call against the host loop it replaces (bit for bit), against the
restatement of the reference's maintenance methods (tests/service_ref.py) at the golden scenarios, next to plant I/O,
through checkpoints, and its refusals.

Packing: ensembles this small are spread by the library, a wavefront per reactor on a card
with more wavefront slots than reactors.  The fused-against-host-loop test and the test beside plant I/O therefore run
twice, spread under the ids they always had and packed (WT_FULL_WAVES, identity placement: reactor r is slot r % R of
wavefront-group r // R); "reactors per wavefront" and the number of sensor passes describe the packed cases.  The
golden-scenario test holds one reactor per ensemble and stays as it is."""
import numpy as np
import pytest

from conftest import golden_npz

import sensor_oracle as SO
import service_ref as SR
from program_helpers import both_packings, equals_spread, packing, spread_only  # noqa: F401  (packing: a fixture)
from test_service_cpu import block_of, deal

pytestmark = pytest.mark.gpu
DT, STEPS = 30.0, 80
SHAPES = [(2, 70), (5, 27), (8, 19), (20, 7), (32, 5)]
# packed only: two full wavefronts and a lone reactor at the zone counts SHAPES leaves out, so that the packed cases reach
# every program-carrying instantiation and every pass structure of the suite (tests/test_sensor_passes.py)
PACKED_SHAPES = [(3, 43), (4, 33), (6, 21), (12, 11), (16, 9)]


def ensemble(wt, n, N, seed=0x5E41CE, history=STEPS, packing=None):
    cols, bc = wt.make_ensemble(N)
    ens = wt.ReactorEnsemble(cols, n_zones=n)
    if packing is not None:
        packing.place(ens)
    ens.set_boundary(bc)
    ens.enable_sensors(seed=seed, history=history)
    return ens


def mixed_program(wt, N, phase=0, together=False):
    """Four slots with per-reactor arrays: reactors four apart take different actions with different references in the
    same step, direct neighbours in different steps (the timed slots are staggered by ``r % 4`` and ``r % 3`` read
    intervals); with ``together`` slot 2 falls due in every reactor at the same read, so that neighbouring reactors
    (neighbouring lanes of a sensor's run in a packed wavefront) apply five different actions to two sensors in one
    step.  Slots 0 and 1 of every fifth reactor hit the DPD sensor in the
    same step (replace first, then trim); slot 2 works on the pH electrodes once they are warm (1 800 s); slot 3 is a
    work order on the flowmeter's DRIFT_WARNING with per-reactor delays.  ``phase`` moves every per-reactor pattern on
    by that many reactors."""
    r = np.arange(N) + phase
    return (wt.Service("chlorine_outlet", np.where(r % 5 == 0, "replace_reagent", "calibrate"), at=300.0 + 30.0 * (r % 4), every=600.0,
                       ref=0.5 + 0.01 * r, ref_mode=np.array(["constant", "sample", "trim"])[r % 3]),
            wt.Service(np.array([3, 2, 6, 5, 4])[r % 5], "calibrate", at=300.0 + 30.0 * (r % 4), every=np.where(r % 2 == 0, 450.0, 0.0),
                       count=3, ref=0.02 * (r % 7), ref_mode=np.array(["trim", "sample"])[r % 2]),
            wt.Service(r % 2, np.array(["rinse", "two_point", "acid_clean", "pepsin_clean", "calibrate"])[r % 5], at=1860.0 + (0.0 if together else 30.0) * (r % 3),
                       ref=7.0, ref2=4.0),
            wt.Service("flow_main", "calibrate", on_status="drift_warning", delay=60.0 * (r % 3), ref_mode="trim", count=2))


def host_loop(ens, prog, steps, dt=DT):
    """What the fused call replaces: one-step calls, the restatement deciding after each read, service_sensors applying."""
    N = ens.n_reactors
    before = np.array(ens.state.time)
    log = []                                                  # per step: what fell due in every reactor
    for _ in range(steps):
        es = ens.step(dt, n_steps=1)
        status = ens.sensor_readings()[1]
        # (a reactor whose step raised takes no reading and gets no service)
        due = [prog.after_read(r, float(es.time[r]), status[:, r]) if es.time[r] > before[r] else [] for r in range(N)]
        before = np.array(es.time)
        log.append(due)
        for k in range(prog.slots):                           # slot order; the reactors of a slot do not interact
            groups = {}
            for r in range(N):
                for d in due[r]:
                    if d[0] == k:
                        groups.setdefault(d[1:4], []).append((r, d[4], d[5]))
            for (sensor, action, mode), members in groups.items():
                mask = np.zeros(N, dtype=bool); ref = np.zeros(N); ref2 = np.zeros(N)
                for r, a, b in members:
                    mask[r], ref[r], ref2[r] = True, a, b
                ens.service_sensors(sensor, action, ref=ref, ref2=ref2, ref_mode=mode, mask=mask)
    return log


def snapshot(ens):
    hv, hs, hf, nf = ens.sensor_history()
    health = ens.sensor_health()
    return dict(hv=hv, hs=hs, hf=hf, nf=nf, readings=ens.sensor_readings(), health=np.stack([health[k] for k in sorted(health)]),
                state=np.stack([ens.state.pH, ens.state.chlorine, ens.state.temperature]))


def by_reactor(snap, *more):
    """The arrays of a ``snapshot`` and ``more`` (reactor last already), each with the reactor on its last axis."""
    return ((snap["hv"], snap["hs"], snap["hf"], snap["nf"]) + tuple(np.asarray(v) for v in snap["readings"])
            + (snap["health"], np.moveaxis(snap["state"], 1, -1)) + tuple(more))


def same(a, b):
    for k in a:
        x, y = (a[k], b[k]) if k != "readings" else (np.stack([np.asarray(v, dtype=np.float64) for v in a[k]]),
                                                     np.stack([np.asarray(v, dtype=np.float64) for v in b[k]]))
        if not np.array_equal(x, y, equal_nan=True):
            return k
    return None


@both_packings("n,N", SHAPES, packed=SHAPES + PACKED_SHAPES)
def test_fused_equals_host_loop(gpu, wt, monkeypatch, n, N, packing):
    """Packed: 32, 12, 8, 3 and 2 reactors per wavefront (SHAPES) and 21, 16, 10, 5 and 4 (PACKED_SHAPES), a partial last
    wavefront, one to four sensor passes, at n = 3, 5 and 6 with a pass boundary inside a sensor's run.  Spread: the
    library's own dealing, a wavefront per reactor where the card has more wavefront slots than the ensemble reactors,
    one sensor pass.  80 steps of 30 s, so the pH electrodes warm up inside the run.  One call under set_schedule(1, 7)
    (slot state crosses item boundaries), one under the default schedule, and the host loop of 80 one-step calls (its
    ``service_sensors`` is a kernel of one thread per reactor, whatever the packing): the same bits everywhere, and the
    packed snapshot and service state equal the spread run's."""
    R = 64 // n
    # The packed cases' program: slot 2 due in all reactors at one read (neighbours otherwise never act in the same
    # step), and the per-reactor patterns moved on until one of the reactors that hit the DPD sensor twice in a step --
    # every fifth -- sits in a slot other than the first (with 5, 3 or 2 to a wavefront and this few reactors none does
    # unmoved).  The spread cases keep the program they always had; a packed case makes its own spread run.
    phase = next(p for p in range(5) if any((r + p) % 5 == 0 and r % R for r in range(N))) if packing.packed else 0
    program = lambda: mixed_program(wt, N, phase, together=packing.packed)
    runs = {}
    for name in ("items", "queue", "host"):
        ens = ensemble(wt, n, N, packing=packing)
        slots = program()
        if name == "host":
            prog = SR.ServiceProgram(wt.service_block(N, *slots))
            log = host_loop(ens, prog, STEPS)
        else:
            if name == "items":
                ens.set_schedule(1, 7)
            ens.set_services(*slots)
            assert ens.info(gpu.WT_INFO_SERVICE) == 1
            assert np.array_equal(ens.service_params(), wt.service_block(N, *slots))
            ens.step(DT, n_steps=STEPS)
            runs[name + "_state"] = ens.service_state().block()
        runs[name] = snapshot(ens)
        packing.check(ens)
        ens.close()
    assert np.all(runs["host"]["nf"] == STEPS)
    assert same(runs["items"], runs["host"]) is None and same(runs["queue"], runs["host"]) is None
    for name in ("items_state", "queue_state"):
        assert np.array_equal(runs[name], prog.state, equal_nan=True), name
    # the program did what it was written for: every slot served, two slots of one sensor in one step among them
    assert np.all(prog.state[:, SR.VS_N_DONE].sum(axis=1) > 0)
    both = prog.params[0, SR.V_T_FIRST] == prog.params[1, SR.V_T_FIRST]
    assert np.any(both & (prog.params[1, SR.V_SENSOR] == 3))
    base = ensemble(wt, n, N, packing=packing); base.step(DT, n_steps=STEPS)
    assert same(snapshot(base), runs["host"]) in ("hv", "hs")          # and it changed the readings
    base.close()
    if packing.packed:
        # in some step two neighbouring slots of one wavefront applied different actions, and a reactor in a slot other
        # than the first had program slots 0 and 1 hit the DPD sensor together (on the restatement's record)
        acts = lambda due: {d[2] for d in due}
        assert any(due[r] and due[r + 1] and acts(due[r]) != acts(due[r + 1]) for due in log for r in range(N - 1) if r // R == (r + 1) // R)
        assert any({(d[0], d[1]) for d in due[r]} >= {(0, 3), (1, 3)} for due in log for r in range(N) if r % R)

    def twin(p):                                              # (the spread run of a packed-only shape or a moved program)
        ens = ensemble(wt, n, N, packing=p)
        ens.set_services(*program())
        ens.step(DT, n_steps=STEPS)
        got = by_reactor(snapshot(ens), ens.service_state().block())
        p.check(ens)
        ens.close()
        return got
    equals_spread(monkeypatch, packing, ("service", n, N, packing.name), n, by_reactor(runs["queue"], runs["queue_state"]), twin)


CASE_SETUP = {"short8": (dict(n_zones=8, flow_rate=8.0, initial_chlorine=2.0),
                         dict(inlet_flow_rate=6.0, chlorine_flow_rate=0.2, inlet_temperature=22.0)),
              "long5": (dict(n_zones=5, initial_pH=7.2), dict(inlet_flow_rate=5.0, inlet_pH=7.5, chlorine_flow_rate=0.3))}


@pytest.mark.parametrize("case", list(CASE_SETUP))
def test_device_against_the_restatement_at_the_golden_scenarios(gpu, wt, case):
    """g14_service_short8 and _long5 (tools/gen_golden_service.py): a case's slots dealt to programs of at most four, a
    sensor's slots together; each program runs on one reactor with one-step calls, the restatement is fed the device's
    own fp32-rounded state as in test_gpu_sensors.py::test_suite_with_physics_vs_oracle.  NaN pattern, status and fault
    streams equal; values within 2e-5 of 1 + |v| (the fp32 signal path); the services at the golden file's steps; the
    slot state exactly.  The flowmeter after its trim: NORMAL, the mean of its reads within 2 % of the true flow (one
    read carries the instrument's noise, 0.75 % of this flow per sigma: see test_service_cpu.py)."""
    g = golden_npz(f"g14_service_{case}.npz")
    cfg_kw, bc_kw = CASE_SETUP[case]
    seed, rid, dt, steps = int(g["seed"]), int(g["reactor"]), float(g["dt"]), g["taps"].shape[0]
    f32 = lambda x: float(np.float32(x))
    programs = deal(g["slots"])
    assert len(programs) == 2
    for rows, sensors in programs:
        cfg = wt.ReactorConfiguration(**cfg_kw)
        ens = wt.ReactorEnsemble([cfg])
        ens.set_boundary(wt.BoundaryConditions(**bc_kw))
        ens.set_schedule(1, 1)
        ens.enable_sensors(seed=seed, reactor_base=rid, history=steps)
        blk = block_of(rows)
        ens._program_call(gpu.lib().wt_ensemble_service_set, gpu.dptr(blk))
        suite = SR.ServicedSuite(cfg.flow_rate, cfg.initial_chlorine, cfg.temperature, 0.0, seed, rid)
        prog = SR.ServiceProgram(blk)
        ov = np.empty((steps, 7)); os_ = np.empty((steps, 7), dtype=np.uint8); of = np.empty((steps, 7), dtype=np.uint8)
        flow = np.empty(steps)
        done = []
        for k in range(steps):
            es = ens.step(dt, n_steps=1)
            taps = [f32(es.pH[0, 0]), f32(es.pH[0, -1]), f32(es.chlorine[0, 0]), f32(es.chlorine[0, -1]), f32(es.temperature[0, 0]),
                    f32(es.temperature[0, -1]), f32(es.flow_rate[0])]
            t = float(es.time[0])
            ov[k], os_[k], of[k] = suite.read_all({0: taps[0], -1: taps[1]}, {0: taps[2], -1: taps[3]}, {0: taps[4], -1: taps[5]}, taps[6], t)
            flow[k] = taps[6]
            for _, i, action, mode, ref, ref2 in prog.after_read(0, t, os_[k]):
                SR.apply(suite, i, action, t, mode, ref, ref2, taps)
                done.append((k, i, action))
        hv, hs, hf, nf = ens.sensor_history()
        assert nf[0] == steps
        hv, hs, hf = hv[:, :, 0], hs[:, :, 0], hf[:, :, 0]
        assert np.array_equal(np.isnan(hv), np.isnan(ov))
        ok = ~np.isnan(ov)
        err = np.max(np.abs(hv[ok] - ov[ok]) / (1.0 + np.abs(ov[ok])))
        print(f"{case} sensors {sorted(sensors)}: max |dv| / (1 + |v|) = {err:.3e}")
        assert err < 2e-5
        assert np.array_equal(hs, os_) and np.array_equal(hf, of)
        mine = g["services"][np.isin(g["services"][:, 1], sorted(sensors))]
        assert np.array_equal(np.array(done, dtype=np.float64), mine[:, :3])
        assert np.array_equal(ens.service_state().block()[:, :, 0], prog.state[:, :, 0], equal_nan=True)
        dev, ref = ens.sensor_health(), SR.health(suite)
        assert np.array_equal(dev["cal_time"][:, 0], ref[:, 1]) and np.array_equal(dev["power_on"][:, 0], ref[:, 2])
        assert np.allclose(dev["cal_offset"][:, 0], ref[:, 0], rtol=0, atol=2e-5 * (1 + np.abs(ref[:, 0]).max()))
        assert np.allclose(np.stack([dev["slow0"], dev["slow1"], dev["slow2"]])[:, :, 0].T, ref[:, 3:6], rtol=1e-6, atol=1e-9)
        if 4 in sensors:
            step = int(mine[mine[:, 1] == 4][0, 0])
            assert np.all(hs[step + 30:, 4] == SO.ST_NORMAL) and np.all(hs[step - 5:step + 1, 4] == SO.ST_DRIFT_WARNING)
            assert abs(np.mean(hv[step + 30:, 4] / flow[step + 30:]) - 1.0) < 0.02
        ens.close()


def test_a_program_changes_nothing_before_its_first_service(gpu, wt, monkeypatch):
    """The spread case of ``changes_nothing_before_its_first_service`` (19 reactors: the library deals them a wavefront
    each on a card with more wavefront slots than that)."""
    changes_nothing_before_its_first_service(wt, monkeypatch, spread_only(monkeypatch))


@pytest.mark.parametrize("packing", ["packed"], indirect=True)
def test_a_program_changes_nothing_before_its_first_service_packed(gpu, wt, monkeypatch, packing):
    """Two full wavefronts of eight reactors and one of three: the scan lanes read the serviced instruments of their
    neighbours' slots.  What the serviced run leaves equals the spread run's, bit for bit."""
    changes_nothing_before_its_first_service(wt, monkeypatch, packing)


def changes_nothing_before_its_first_service(wt, monkeypatch, packing):
    """Plant I/O with a PI loop on chlorine_outlet; the program's first service is the DPD calibration after the read at
    t = 600 s (step 20 of 30 s).  After 20 steps every image word, command, PI state and reading equals the run without
    the program, bit for bit; ten steps later the loop has seen the serviced instrument."""
    n, N = 8, 19
    out = run_beside_plant_io(wt, n, N, packing)
    # (the service follows the read of step 20: the instrument's calibration fields already differ, nothing read so far does)
    health = out["serviced", "before"].pop("health"), out["plain", "before"].pop("health")
    assert not np.array_equal(health[0], health[1], equal_nan=True)
    assert same(out["plain", "before"], out["serviced", "before"]) is None
    after = same(out["plain", "after"], out["serviced", "after"])
    assert after is not None
    assert not np.array_equal(out["plain", "after"]["ctl"], out["serviced", "after"]["ctl"], equal_nan=True)
    left = lambda o: by_reactor(o["serviced", "after"], o["serviced", "after"]["img"].T, o["serviced", "after"]["ok"].T,
                                o["serviced", "after"]["bc"], o["serviced", "after"]["ctl"])
    equals_spread(monkeypatch, packing, "service beside plant I/O", n, left(out), lambda p: left(run_beside_plant_io(wt, n, N, p)))


def run_beside_plant_io(wt, n, N, packing):
    out = {}
    for name in ("plain", "serviced"):
        ens = ensemble(wt, n, N, history=40, packing=packing)
        ens.enable_plant_io()
        ens.set_schedule(0, 5)
        ens.enable_control(chlorine=wt.PILoop("chlorine_outlet", setpoint=1.5, kp=0.05, ki=0.001, bias=0.2, out_max=1.0))
        if name == "serviced":
            ens.set_services(wt.Service("chlorine_outlet", "calibrate", at=600.0, ref_mode="trim"),
                             wt.Service("flow_main", "calibrate", at=690.0, ref_mode="trim"))
        for stage, steps in (("before", 20), ("after", 10)):
            ens.step(DT, n_steps=steps)
            img, ok = ens.input_image()
            out[name, stage] = dict(img=img, ok=ok, bc=ens.boundary(), ctl=ens.control_state().block(), **snapshot(ens))
        packing.check(ens)
        ens.close()
    return out


def test_checkpoints_carry_the_program(gpu, wt):
    """30 steps, checkpoint; the restored handle, the clone and a mark / rewind each continue for 50 steps with the bits
    of the handle that was never saved, service_state() and sensor_health() included.  reset_services re-arms,
    clear_services stops."""
    n, N = 5, 27
    def fresh():
        ens = ensemble(wt, n, N)
        ens.set_services(*mixed_program(wt, N))
        return ens
    def full(ens):
        return dict(svc=ens.service_state().block(), **snapshot(ens))
    never = fresh(); never.step(DT, n_steps=30); never.step(DT, n_steps=50)
    want = full(never); never.close()
    a = fresh(); a.step(DT, n_steps=30)
    blob = a.checkpoint()
    b = ensemble(wt, n, N, seed=1, history=3); b.restore(blob)
    c = a.clone()
    a.mark()
    for ens in (a, b, c):
        ens.step(DT, n_steps=50)
        assert same(full(ens), want) is None
    a.rewind(); a.step(DT, n_steps=50)
    assert same(full(a), want) is None
    assert b.info(gpu.WT_INFO_SERVICE) == 1 and np.array_equal(b.service_params(), a.service_params())
    # reset: the set-time state; the timed slots fall due again at the next read
    done = a.service_state().n_done
    a.reset_services()
    st = a.service_state()
    assert not st.n_done.any() and np.isnan(st.t_last).all() and np.isnan(st.t_seen).all()
    assert np.array_equal(st.t_due, a.service_params()[:, SR.V_T_FIRST])
    a.step(DT, n_steps=1)
    assert np.all(a.service_state().n_done[0] == 1) and done[0].min() >= 1
    # clear: the switch is off, the sensors keep what was done to them and are not touched again
    health = a.sensor_health()
    a.clear_services()
    assert a.info(gpu.WT_INFO_SERVICE) == 0
    with pytest.raises(ValueError, match="no service program is set"):
        a.service_state()
    a.step(DT, n_steps=25)
    after = a.sensor_health()
    assert np.array_equal(after["cal_time"], health["cal_time"]) and np.array_equal(after["cal_offset"], health["cal_offset"])
    # a blob of the parent's layout is another library's
    bad = bytearray(blob); bad[32] ^= 1
    with pytest.raises(ValueError, match="layout fingerprint"):
        b.restore(bytes(bad))
    for ens in (a, b, c):
        ens.close()


def test_refusals_on_a_device(gpu, wt):
    """set_services before enable_sensors; n = 33: the program is refused, the immediate service works and matches the
    restatement; enabling the sensors again (after a restore of a blob without them) starts without a program."""
    L = gpu.lib()
    cols, bc = wt.make_ensemble(4)
    ens = wt.ReactorEnsemble(cols, n_zones=8); ens.set_boundary(bc)
    blk = wt.service_block(4, wt.Service("chlorine_outlet", "calibrate", at=60.0))
    assert L.wt_ensemble_service_set(ens._h, gpu.dptr(blk)) == gpu.WT_E_STATE
    for call in (lambda: ens.service_sensors("pH_inlet", "rinse"), ens.sensor_health):
        with pytest.raises(ValueError, match="sensor suite is not enabled"):
            call()
    bare = ens.checkpoint()
    ens.enable_sensors(seed=5)
    assert ens.info(gpu.WT_INFO_SERVICE) == 0
    ens.clear_services()                                   # no effect while none is set
    ens.set_services(wt.Service("chlorine_outlet", "calibrate", at=60.0))
    assert ens.info(gpu.WT_INFO_SERVICE) == 1
    with pytest.raises(ValueError, match="only the amperometric"):
        ens.service_sensors("chlorine_outlet", "replace_membrane")
    with pytest.raises(ValueError, match="ref and ref2 must be finite"):
        ens.service_sensors("chlorine_outlet", "calibrate", ref=np.nan)
    ens.restore(bare)                                      # the suite goes, and the program with it
    assert ens.info(gpu.WT_INFO_SERVICE) == 0
    ens.enable_sensors(seed=5)
    assert ens.info(gpu.WT_INFO_SERVICE) == 0
    ens.close()
    # n = 33: the n > 32 kernel carries no program; the immediate service is a kernel of its own
    seed = 77
    cfg = wt.ReactorConfiguration(n_zones=33)
    big = wt.ReactorEnsemble([cfg, cfg]); big.set_boundary(wt.BoundaryConditions())
    big.enable_sensors(seed=seed, history=8)
    blk = wt.service_block(2, wt.Service("chlorine_outlet", "calibrate", at=60.0))
    assert L.wt_ensemble_service_set(big._h, gpu.dptr(blk)) == gpu.WT_E_STATE
    suite = SR.ServicedSuite(cfg.flow_rate, cfg.initial_chlorine, cfg.temperature, 0.0, seed, 1)
    f32 = lambda x: float(np.float32(x))
    ov = np.empty((8, 7))
    for k in range(8):
        es = big.step(DT, n_steps=1)
        taps = [f32(es.pH[1, 0]), f32(es.pH[1, -1]), f32(es.chlorine[1, 0]), f32(es.chlorine[1, -1]), f32(es.temperature[1, 0]),
                f32(es.temperature[1, -1]), f32(es.flow_rate[1])]
        t = float(es.time[1])
        ov[k] = suite.read_all({0: taps[0], -1: taps[1]}, {0: taps[2], -1: taps[3]}, {0: taps[4], -1: taps[5]}, taps[6], t)[0]
        if k == 3:                                         # reactor 1 alone: the flowmeter trimmed, the DPD reagent replaced
            big.service_sensors("flow_main", "calibrate", ref_mode="trim", mask=[False, True])
            big.service_sensors(3, SR.REPLACE_REAGENT, mask=np.array([False, True]))
            SR.apply(suite, 4, SR.CALIBRATE, t, SR.REF_TRIM, 0.0, 0.0, taps)
            SR.apply(suite, 3, SR.REPLACE_REAGENT, t)
    hv = big.sensor_history()[0][:, :, 1]
    assert np.array_equal(np.isnan(hv), np.isnan(ov))
    ok = ~np.isnan(ov)
    assert np.max(np.abs(hv[ok] - ov[ok]) / (1.0 + np.abs(ov[ok]))) < 2e-5
    health = big.sensor_health()
    assert health["cal_time"][4, 1] == 4 * DT and health["cal_time"][4, 0] == 0.0 and health["slow0"][3, 1] > health["slow0"][3, 0]
    assert np.allclose(SR.health(suite)[:, :6], np.stack([health[k][:, 1] for k in ("cal_offset", "cal_time", "power_on", "slow0", "slow1", "slow2")]).T,
                       rtol=1e-6, atol=1e-4)
    big.close()
