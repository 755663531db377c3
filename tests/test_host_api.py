"""Host-side logic that needs no GPU: dataclasses mirror the reference's API,
SoA packing, synthetic generator, the shared library exports its C ABI and
refuses to compute without a device."""
import ctypes as C
import dataclasses
import os
import re
import sys

import numpy as np
import pytest

from conftest import ROOT, golden_json


def test_dataclass_defaults_match_reference(wt):
    # reactor.py:61-89, :169-186 defaults (values recorded in SURVEY.md Appendix A)
    cfg = wt.ReactorConfiguration()
    assert (cfg.volume, cfg.height, cfg.diameter, cfg.n_zones) == (1000.0, 2.0, 0.798, 5)
    assert (cfg.flow_rate, cfg.impeller_speed, cfg.impeller_diameter, cfg.power_number) == (5.0, 60.0, 0.3, 5.0)
    assert (cfg.initial_pH, cfg.alkalinity, cfg.total_carbonate, cfg.initial_chlorine, cfg.temperature) == (7.0, 100.0, 2.0, 2.0, 20.0)
    assert cfg.enable_thermal_stratification is True
    b = wt.BoundaryConditions()
    assert [getattr(b, k) for k in wt.params.BOUNDARY_FIELDS] == [5.0, 7.5, 0.0, 20.0, 0.0, 0.1, 0.0, 50.0, 20.0, 0.0]
    assert [f.name for f in dataclasses.fields(b)] == list(wt.params.BOUNDARY_FIELDS)
    s = wt.ReactorState()
    assert s.pH.shape == (5,) and np.all(s.H_concentration == 10 ** (-s.pH))
    assert np.all(s.density == 998.2) and np.all(s.chlorine_decay_rate == 0.0001)
    assert set(s.state_dict()) >= {"time", "pH", "chlorine", "temperature", "flow_rate", "H_concentration"}
    assert wt.PhysicsEngine is wt.IntegratedCSTR


def test_config_validate_errors(wt):
    g = golden_json("g4_faults.json")
    with pytest.raises(ValueError, match="Volume mismatch"):
        wt.ReactorConfiguration(volume=500.0).validate()
    assert g["volume_mismatch"] == "ValueError"
    with pytest.raises(AssertionError):
        wt.ReactorConfiguration(temperature=45.0).validate()
    with pytest.raises(AssertionError):
        wt.ReactorConfiguration(initial_chlorine=11.0).validate()
    wt.ReactorConfiguration().validate()


def test_boundary_block_packing(wt):
    bb = wt.boundary_block(wt.BoundaryConditions(acid_flow_rate=0.5), 3)
    assert bb.shape == (10, 3) and np.all(bb[4] == 0.5) and np.all(bb[0] == 5.0)
    seq = [wt.BoundaryConditions(inlet_pH=6.0 + i) for i in range(3)]
    assert np.array_equal(wt.boundary_block(seq, 3)[1], [6.0, 7.0, 8.0])
    d = wt.boundary_block({"inlet_temperature": np.array([1.0, 2.0, 3.0])}, 3)
    assert np.array_equal(d[3], [1.0, 2.0, 3.0]) and np.all(d[7] == 50.0)
    with pytest.raises(ValueError):
        wt.boundary_block(seq, 4)
    with pytest.raises(ValueError):
        wt.boundary_block(np.zeros((9, 3)), 3)


def test_synthetic_ensemble_is_prefix_stable_and_in_range(wt):
    c1, b1 = wt.make_ensemble(64)
    c2, b2 = wt.make_ensemble(1000)
    for k in c1:
        assert np.array_equal(c1[k], c2[k][:64])
    assert np.array_equal(b1, b2[:, :64])
    c3, b3 = wt.make_ensemble(100, start=900)
    assert np.array_equal(b3, b2[:, 900:])
    assert c2["initial_pH"].min() >= 6.5 and c2["initial_pH"].max() <= 8.5
    assert c2["temperature"].min() >= 10 and c2["temperature"].max() <= 30
    assert np.all((b2[4] == 0) | ((b2[4] > 0) & (b2[4] <= 2)))
    assert 0.35 < np.mean(b2[4] == 0) < 0.65 and 0.6 < np.mean(b2[9] == 0) < 0.9
    assert np.all(b2[0] <= 12.0) and np.all(b2[0] >= 1.6)


def test_shard_bounds_cover_everything(wt):
    for N in (1, 7, 100, 100000):
        for W in (1, 2, 3, 8):
            spans = [wt.shard_bounds(N, W, r) for r in range(W)]
            assert spans[0][0] == 0 and spans[-1][1] == N
            assert all(spans[i][1] == spans[i + 1][0] for i in range(W - 1))
            sizes = [hi - lo for lo, hi in spans]
            assert max(sizes) - min(sizes) <= 1
    with pytest.raises(ValueError):
        wt.shard_bounds(10, 2, 2)


def test_library_exports_every_declared_symbol(native):
    """Every function declared in include/wtphys.h is exported by libwtphys.so."""
    hdr = open(os.path.join(ROOT, "include", "wtphys.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    names = sorted(set(re.findall(r"\b(wt_[a-z_0-9]+)\s*\(", hdr)))
    assert len(names) >= 20
    lib = C.CDLL(native.LIB_PATH)
    for name in names:
        assert hasattr(lib, name), f"{name} not exported"
    assert lib.wt_abi_version() == 1


def test_binding_table_is_the_header(native):
    """``_native.SIGNATURES`` binds exactly the functions include/wtphys.h declares, each once: the table is a dict
    display, so a name written twice would silently keep its last entry -- the source is read for that."""
    hdr = open(os.path.join(ROOT, "include", "wtphys.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(wt_[a-z_0-9]+)\s*\(", hdr))
    assert set(native.SIGNATURES) == declared
    src = open(native.__file__).read()
    table = src[src.index("SIGNATURES = {"):src.index("\n}\n", src.index("SIGNATURES = {"))]
    keys = re.findall(r'^\s*"(wt_[a-z_0-9]+)":', table, flags=re.M)
    assert sorted(keys) == sorted(declared), "a name bound twice, or an entry the regex does not see"
    # nothing binds a function outside the table
    assert not re.findall(r"\.(?:argtypes|restype)\s*=", src.replace("fn.argtypes, fn.restype = ", ""))
    L = native.lib()
    for name, sig in native.SIGNATURES.items():
        argtypes, restype = sig if isinstance(sig, tuple) else (sig, C.c_int)
        fn = getattr(L, name)
        assert list(fn.argtypes) == list(argtypes) and fn.restype is restype, name


def test_program_check_without_a_device(native, wt):
    """wt_program_check runs the checks of each scan program's set call on the host: the off blocks pass, a bad block
    gets the set call's message (the builder raises it as a ValueError), a malformed call is refused."""
    L, N = native.lib(), 3
    off = {native.WT_PROG_CONTROL: wt.control_block(N), native.WT_PROG_INJECT: wt.injection_block(N),
           native.WT_PROG_ALARM: wt.alarm_block(N), native.WT_PROG_ACTUATOR: wt.actuator_block(N)}
    for program, blk in off.items():
        assert L.wt_program_check(program, native.dptr(blk), N) == native.WT_OK, program
    blk = off[native.WT_PROG_CONTROL]
    for program, params, n in ((4, blk, N), (-1, blk, N), (native.WT_PROG_CONTROL, None, N),
                               (native.WT_PROG_CONTROL, blk, 0)):
        assert L.wt_program_check(program, native.dptr(params), n) == native.WT_E_ARG, (program, n)
    # a bad block per program: (program, a valid block, {(slot, row): value} that spoils it, message, builder call)
    cases = (
        (native.WT_PROG_CONTROL, wt.control_block(N, chlorine=wt.PILoop(3, 1.0)), {(0, 2): 0.0},
         "direction must be +1 or -1", lambda: wt.control_block(N, chlorine=wt.PILoop(3, 1.0, direction=0))),
        (native.WT_PROG_INJECT, wt.injection_block(N, wt.Injection(3, "bias")), {(0, 2): 50.0, (0, 3): 40.0},
         "start must not exceed end", lambda: wt.injection_block(N, wt.Injection(3, "bias", start=50.0, end=40.0))),
        (native.WT_PROG_INJECT, wt.injection_block(N, wt.Injection(3, "bias")), {(0, 3): -np.inf},
         "injection parameters must be finite (end may be +inf)",
         lambda: wt.injection_block(N, wt.Injection(3, "bias", end=-np.inf))),
        (native.WT_PROG_ALARM, wt.alarm_block(N, wt.Alarm(3, "high", 1.0, action="trip_chlorine")), {(0, 9): 1.5},
         "a trip_chlorine slot's trip_value must be in [0, 1]",
         lambda: wt.alarm_block(N, wt.Alarm(3, "high", 1.0, action="trip_chlorine", trip_value=1.5))),
        (native.WT_PROG_ACTUATOR, wt.actuator_block(N, wt.Actuator("inlet")), {(2, 4): 9.0},
         "delay must be an integer in 0..8", lambda: wt.actuator_block(N, wt.Actuator("inlet", delay=9))),
    )
    for program, good, spoil, msg, build in cases:
        assert L.wt_program_check(program, native.dptr(good), N) == native.WT_OK, msg
        bad = good.copy()
        for (slot, row), value in spoil.items():
            bad[slot, row] = value
        assert L.wt_program_check(program, native.dptr(bad), N) == native.WT_E_ARG, msg
        assert L.wt_last_error().decode() == msg
        with pytest.raises(ValueError) as ei:
            build()
        assert str(ei.value) == msg
    # several bad fields in different reactors: the first failing check of the first bad reactor is the one named
    bad = off[native.WT_PROG_ACTUATOR].copy()
    bad[0, 4, 0], bad[0, 1, 1] = 9.0, -1.0
    assert L.wt_program_check(native.WT_PROG_ACTUATOR, native.dptr(bad), N) == native.WT_E_ARG
    assert L.wt_last_error() == b"delay must be an integer in 0..8"
    # the service and tune programs: wt_service_check and wt_tune_check are the same check under their own names
    for program, named, good, (slot, row), msg in (
            (native.WT_PROG_SERVICE, L.wt_service_check, wt.service_block(N, wt.Service("chlorine_outlet", "calibrate", at=60.0)),
             (0, 5), "period must be 0 (once) or at least 0.001 s"),
            (native.WT_PROG_TUNE, L.wt_tune_check, wt.tune_block(N, acid=wt.RelayTune("pH_outlet", 7.2, 0.5, 1.5)),
             (1, 5), "bias - amplitude must be >= 0 and bias + amplitude at most the loop's command limit (1.0 chlorine, 2.0 acid)")):
        bad = good.copy()
        bad[slot, row, N - 1] = 1e-4 if program == native.WT_PROG_SERVICE else 0.75
        for blk, code, text in ((good, native.WT_OK, None), (np.zeros_like(good), native.WT_OK, None), (bad, native.WT_E_ARG, msg)):
            for check in (lambda: L.wt_program_check(program, native.dptr(blk), N), lambda: named(N, native.dptr(blk))):
                assert check() == code, (program, text)
                assert text is None or L.wt_last_error().decode() == text
        assert L.wt_program_check(program, native.dptr(good), 0) == named(0, native.dptr(good)) == native.WT_E_ARG
        assert L.wt_last_error() == b"n_reactors must be >= 1"
        assert named(0, None) == native.WT_E_ARG and L.wt_last_error() == b"n_reactors must be >= 1"   # their own order
        assert named(N, None) == native.WT_E_ARG and L.wt_last_error() == b"NULL argument"             # and their own text
    assert L.wt_program_check(native.WT_PROG_TUNE + 1, native.dptr(off[native.WT_PROG_CONTROL]), N) == native.WT_E_ARG
    assert L.wt_last_error() == b"unknown program"


def test_no_silent_cpu_fallback(native, wt):
    """Without a HIP device the product path must fail loudly."""
    if native.device_count() > 0:
        pytest.skip("a GPU is visible; the loud-failure path is for GPU-less hosts")
    with pytest.raises(native.WtError) as ei:
        wt.ReactorEnsemble([wt.ReactorConfiguration(n_zones=4)])
    assert ei.value.code == native.WT_E_NOGPU
    with pytest.raises(native.WtError):
        wt.solve_pH(100.0, 2.0, 20.0)


def test_product_package_never_imports_oracle():
    pkg = os.path.join(ROOT, "ics-wt-physicsengine_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".hpp", ".h", ".cpp")):
                text = open(os.path.join(dirpath, f)).read()
                assert "wt_oracle" not in text and "libwtoracle" not in text, f


# the names wt_simulator.core exports (/root/reference/src/wt_simulator/core/__init__.py:238-263)
REFERENCE_CORE_EXPORTS = ("IntegratedCSTR", "ReactorConfiguration", "ReactorState", "BoundaryConditions",
                          "TemperatureDependentKinetics", "ArrheniusParameters", "AqueousChemistry", "BufferSystem",
                          "TransportModel", "GeometryParameters", "FlowParameters", "SpatialModel", "StratificationParameters",
                          "validate_thermodynamics", "validate_chemistry", "validate_transport", "validate_spatial",
                          "validate_integrated_reactor")


def test_import_surface_covers_the_reference_export_list(wt):
    for name in REFERENCE_CORE_EXPORTS + ("run_all_validations",):
        assert hasattr(wt, name) and name in wt.core.__all__, name


def test_physics_subobjects_reproduce_reference_constants(wt):
    """TransportModel / AqueousChemistry / TemperatureDependentKinetics / SpatialModel as host-side holders of the
    init-time constants: bit-identical to what the reference's objects held (tests/golden/g1_constants.json)."""
    g = golden_json("g1_constants.json")
    for e in g["configs"]:
        c = e["config"]
        tm = wt.TransportModel(wt.GeometryParameters(c["volume"], c["height"], c["diameter"], c["n_zones"]),
                               wt.FlowParameters(c["flow_rate"], c["turbulent_intensity"], c["recirculation_ratio"],
                                                 c["impeller_speed"], c["impeller_diameter"], c["power_number"]), c["temperature"])
        assert tm.K_exchange_per_s == e["K_exchange_per_s"] == tm.K_matrix[0, 1]
        assert tm.superficial_velocity == e["superficial_velocity"] and tm.D_effective == e["D_effective"]
        ch = wt.AqueousChemistry(wt.BufferSystem(c["alkalinity"], c["total_carbonate"], c["temperature"]))
        assert (ch.Kw, ch.Ka1, ch.Ka2, ch.Ka_HOCl) == (e["Kw"], e["Ka1"], e["Ka2"], e["Ka_HOCl"])
    th = wt.TemperatureDependentKinetics()
    assert all(th.chlorine_decay_rate(float(T)) == v for T, v in g["k_decay"].items())
    sp = wt.SpatialModel(5, 2.0)
    assert all(sp.calculate_water_density(float(T)) == v for T, v in g["density"].items())
    ch = wt.AqueousChemistry(wt.BufferSystem(100.0, 2.0, 20.0))
    assert ch.buffering_capacity(7.2) == g["beta_7p2"] and ch.pH_dependent_chlorine_decay_factor(7.2) == g["decay_factor_7p2"]
    with pytest.raises(ValueError, match="outside liquid water range"):
        th.chlorine_decay_rate(100.5)


def test_reference_validators_that_need_no_gpu(wt, capsys):
    wt.validate_thermodynamics(); wt.validate_transport(); wt.validate_spatial()
    out = capsys.readouterr().out
    assert out.count("validations passed") == 3


def _build_c_client(tmp_path):
    import os, subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    csrc = os.path.join(root, "ics-wt-physicsengine_amd", "csrc")
    exe = str(tmp_path / "abi_client")
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(root, "include"),
                    os.path.join(root, "tests", "c_abi", "abi_client.c"), "-L", csrc, "-lwtphys", f"-Wl,-rpath,{csrc}", "-o", exe],
                   check=True)
    return exe


def test_boundary_is_plain_c(tmp_path):
    """include/wtphys.h is valid strict C99 and a C program that drives the whole step path through it links against
    csrc/libwtphys.so (no C++ or torch types in the signatures) -- the shape a cgo / JNI / FFI binding has."""
    import subprocess
    exe = _build_c_client(tmp_path)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 1 and "usage" in r.stderr



def test_known_answers_of_the_physics_relations(wt):
    """The reference's own known answers (thermodynamics.py:403-417, transport.py:536-554, chemistry.py:545-546,
    spatial.py:561-565) and the fixture values of g1_constants.json, through the column-wise routines of ``params``
    that the classes and the ensemble's constant block share -- scalars and arrays give the same numbers."""
    g = golden_json("g1_constants.json")
    P = wt.params
    temps = np.array([float(t) for t in g["k_decay"]])
    assert np.array_equal(P.arrhenius(temps, 1e-4, 45000.0), np.array(list(g["k_decay"].values())))
    assert P.arrhenius(20.0, 1e-4, 45000.0) == 1e-4                            # the reference rate at the reference temperature
    assert abs(P.water_ionization_constant(25.0) / 1e-14 - 1) < 1e-6 and P.carbonate_pKa(25.0, 1) == 6.35
    dens = np.array([float(t) for t in g["density"]])
    assert np.array_equal(P.water_density(dens), np.array(list(g["density"].values())))
    assert P.water_density(4.0) == 999.97 and P.water_density(8.0) < P.water_density(8.0001)      # the 8 degC jump
    with pytest.raises(ValueError, match=r"Temperature -0\.5°C outside liquid water range \[0\.0, 100\.0\]°C"):
        P.kelvin(np.array([3.0, -0.5, 120.0]))                                  # the first offender is named
    # carbonate fractions sum to one, buffer capacity / decay factor at the fixture point
    eq = P.equilibrium_constants(np.array([20.0]))
    H = P._pow10_neg(np.array([6.0, 7.2, 8.4, 10.3]))
    assert np.allclose(sum(P.carbonate_fractions(H, eq["Ka1"], eq["Ka2"])), 1.0, rtol=0, atol=1e-15)
    assert P.buffer_capacity(H, eq["Kw"], eq["Ka1"], eq["Ka2"], 2.0 / 1000.0)[1] == g["beta_7p2"]
    assert P.chlorine_decay_factor(H, eq["Ka_HOCl"])[1] == g["decay_factor_7p2"]
    # exchange operator: zero row sums except the outlet sink, negative semi-definite, K_ex of the fixture configurations
    for e in g["configs"]:
        c = e["config"]
        cols = {k: np.array([float(c[k])]) for k in ("volume", "height", "diameter", "flow_rate", "impeller_speed",
                                                       "impeller_diameter", "power_number", "temperature")}
        t = P.transport_columns(cols, c["n_zones"])
        assert t["K_exchange_per_s"][0] == e["K_exchange_per_s"] and t["superficial_velocity"][0] == e["superficial_velocity"]
        K = P.exchange_matrix(t["K_exchange_per_s"][0], t["Q_per_V"][0], c["n_zones"])
        rows = K.sum(axis=1)
        assert np.abs(rows[:-1]).max() < 1e-12 and abs(rows[-1] + t["Q_per_V"][0]) < 1e-12
        assert np.linalg.eigvalsh((K + K.T) / 2).max() <= 1e-10
    # stratification: warm water on top is stable (Ri > 0), suppression only where Ri exceeds the critical value
    rho = P.water_density(np.array([17.0, 19.0, 21.0, 23.0, 25.0]))
    ri = P.interface_richardson(rho, 0.4, 0.01)
    assert (ri < 0).all() and (P.interface_richardson(rho[::-1], 0.4, 0.01) > 0).all()
    assert np.array_equal(P.suppression_factors(rho[::-1], 0.4, 0.01), np.full(4, 0.5)) and np.isinf(P.interface_richardson(rho, 0.4, 1e-7)).all()
    cv, seg = P.mixing_quality(np.array([[2.0, 2.0, 2.0], [1.0, 2.0, 3.0], [0.0, 0.0, 0.0]]))
    assert cv[0] == 0 and seg[0] == 0 and 0 < seg[1] < 1 and cv[2] == 0


def test_host_modules_are_not_transliterations():
    """Statement overlap of the host-side physics modules with the reference's core/*.py (docstrings and comments
    dropped on both sides, one statement per line): class / field / method names are the drop-in contract, the bodies
    are this build's own.  The reference's statements are held as digests (tests/golden/g12_reference_core_statements.json,
    oracle/gen_golden_overlap.py), so the check needs no reference sources."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import overlap_check as oc
    from gen_golden_overlap import digest
    known = set(golden_json("g12_reference_core_statements.json")["digests"])
    assert len(known) > 500
    for name in ("physics.py", "chemistry.py", "params.py"):
        lines = oc.normalised_lines(os.path.join(ROOT, "ics-wt-physicsengine_amd", "core", name))
        share = sum(digest(l) in known for l in lines) / len(lines)
        assert share < 0.25, (name, share)


# per scan program: its C entry points (besides wt_program_check), the header constants and values tests rely on, its
# device source, its package exports and its ReactorEnsemble methods
PROGRAMS = {
    "control": (("wt_ensemble_control_enable", "wt_ensemble_control_retune", "wt_ensemble_control_get",
                 "wt_ensemble_control_disable"),
                (r"#define WT_CTL_LOOPS 2\b", r"WT_PROG_CONTROL = 0\b", r"WT_NC = 9\b", r"WT_NCS = 8\b"),
                "wt_ctl.hpp", ("PILoop", "ControlState", "LoopState", "control_block"),
                ("enable_control", "retune_control", "disable_control", "control_state")),
    "inject": (("wt_ensemble_inject_set", "wt_ensemble_inject_get", "wt_ensemble_inject_clear"),
               (r"#define WT_INJ_SLOTS 4\b", r"WT_NI = 6\b", r"WT_NIS = 4\b", r"WT_INJ_CMD_ACID = 7\b",
                r"WT_INJ_CMD_INLET = 9\b", r"WT_INJ_FAULT = 7\b", r"WT_PROG_INJECT = 1\b"),
               "wt_inj.hpp", ("Injection", "InjectionState", "injection_block"),
               ("set_injections", "injection_state", "clear_injections")),
    "alarm": (("wt_ensemble_alarm_set", "wt_ensemble_alarm_get", "wt_ensemble_alarm_reset", "wt_ensemble_alarm_words",
               "wt_ensemble_alarm_device", "wt_ensemble_alarm_clear"),
              (r"#define WT_ALM_SLOTS 4\b", r"WT_PROG_ALARM = 2\b", r"WT_NA = 10\b", r"WT_NAS = 8\b", r"WT_NAR = 6\b",
               r"WT_A_TRIP_VALUE = 9\b", r"WT_AS_N_BAD = 7\b", r"WT_AR_N_OVR_CHLORINE = 5\b",
               r"WT_ALM_TRIP_CHLORINE = 2\b"),
              "wt_alm.hpp", ("Alarm", "AlarmState", "alarm_block"),
              ("set_alarms", "alarm_state", "alarm_words", "reset_alarms", "clear_alarms")),
    "actuator": (("wt_ensemble_actuator_set", "wt_ensemble_actuator_get", "wt_ensemble_actuator_clear"),
                 (r"#define WT_ACT_CHANNELS 3\b", r"#define WT_ACT_MAX_DELAY 8\b", r"WT_NV = 9\b", r"WT_NVS = 9\b",
                  r"WT_V_FAIL_VALUE = 8\b", r"WT_VS_N_FAULT = 8\b", r"WT_ACT_FAIL_TO = 2\b", r"WT_ACT_INLET = 2\b",
                  r"WT_PROG_ACTUATOR = 3\b"),
                 "wt_act.hpp", ("Actuator", "ActuatorState", "actuator_block"),
                 ("set_actuators", "actuator_state", "clear_actuators")),
    "disturb": (("wt_ensemble_disturb_set", "wt_ensemble_disturb_get", "wt_ensemble_disturb_history",
                 "wt_ensemble_disturb_clear"),
                (r"WT_DST_SLOTS\b", r"WT_DST_OFF\b", r"WT_DST_STEP\b", r"WT_DST_RAMP\b", r"WT_DST_SINE\b",
                 r"WT_DST_OU\b", r"WT_ND\b", r"WT_NDS\b", r"WT_PROG_DISTURB = 4\b"),
                "wt_dst.hpp", ("Disturbance", "DisturbanceState", "disturbance_block"),
                ("set_disturbances", "disturbance_state", "disturbance_history", "clear_disturbances")),
    "score": (("wt_ensemble_score_set", "wt_ensemble_score_get", "wt_ensemble_score_curve", "wt_ensemble_score_reset",
               "wt_ensemble_score_clear"),
              (r"#define WT_SCR_SLOTS 4\b", r"#define WT_SCR_MAX_BINS 32\b", r"WT_SCR_BAND = 1\b", r"WT_SP_T_END = 7\b",
               r"WT_NSP = 8\b", r"WT_SS_RUN_MAX = 14\b", r"WT_NSS = 15\b", r"WT_PROG_SCORE = 5\b"),
              "wt_scr.hpp", ("Score", "ScoreState", "ScoreCurve", "score_block"),
              ("set_scores", "score_state", "score_curve", "reset_scores", "clear_scores")),
    "detect": (("wt_ensemble_detect_set", "wt_ensemble_detect_get", "wt_ensemble_detect_reset", "wt_ensemble_detect_clear"),
               (r"#define WT_DET_SLOTS 4\b", r"WT_DET_FLATLINE = 3\b", r"WT_NK = 12\b", r"WT_NKS = 16\b",
                r"WT_KR_LABEL_END = 1\b", r"WT_NKR = 2\b", r"WT_PROG_DETECT = 6\b"),
               "wt_det.hpp", ("Detector", "DetectorState", "detector_block"),
               ("set_detectors", "detector_state", "reset_detectors", "clear_detectors")),
    "trend": (("wt_ensemble_trend_set", "wt_ensemble_trend_get", "wt_ensemble_trend_data", "wt_ensemble_trend_reset",
               "wt_ensemble_trend_clear"),
              (r"#define WT_TRD_SLOTS 8\b", r"WT_TRD_DETECT = 11\b", r"WT_T_T_END = 5\b", r"WT_NT = 6\b", r"WT_TS_LAST = 3\b",
               r"WT_NTS = 4\b", r"WT_PROG_TREND = 7\b"),
              "wt_trd.hpp", ("Trend", "TrendState", "TrendData", "trend_block"),
              ("set_trends", "trend_state", "trend_data", "reset_trends", "clear_trends")),
    "service": (("wt_ensemble_service_set", "wt_ensemble_service_get", "wt_ensemble_service_params", "wt_ensemble_service_reset",
                 "wt_ensemble_service_clear", "wt_service_check"),
                (r"#define WT_SVC_SLOTS 4\b", r"WT_SVC_REPLACE_REAGENT = 6\b", r"WT_SV_REF2 = 11\b", r"WT_NSV = 12\b",
                 r"WT_NSVS = 4\b", r"WT_INFO_SERVICE = 22\b", r"WT_PROG_SERVICE = 8\b"),
                "wt_svc.hpp", ("Service", "ServiceState", "service_block"),
                ("set_services", "service_state", "service_params", "reset_services", "clear_services")),
    "tune": (("wt_ensemble_tune_set", "wt_ensemble_tune_get", "wt_ensemble_tune_params", "wt_ensemble_tune_reset",
              "wt_ensemble_tune_clear", "wt_tune_check"),
             (r"#define WT_TUN_LOOPS 2\b", r"WT_TUN_COMMISSION = 13\b", r"WT_NU = 14\b", r"WT_TUNS_COMMISSIONED = 19\b",
              r"WT_NUS = 20\b", r"WT_INFO_TUNE = 23\b", r"WT_PROG_TUNE = 9\b"),
             "wt_tun.hpp", ("RelayTune", "LoopTune", "TunerState", "tune_block"),
             ("set_tuners", "tuner_state", "tuner_params", "reset_tuners", "clear_tuners")),
}


@pytest.mark.parametrize("program", list(PROGRAMS))
def test_program_symbols_declared_and_exported(native, wt, program):
    entries, constants, source, exports, methods = PROGRAMS[program]
    entries += ("wt_program_check",)
    header = open(os.path.join(ROOT, "include", "wtphys.h")).read()
    for name in entries:
        assert re.search(r"\bint " + name + r"\(", header), name
        assert hasattr(native.lib(), name), name
    for pattern in constants + (r"#define WT_ABI_VERSION 1\b",):
        assert re.search(pattern, header), pattern
    code = "WT_PROG_" + program.upper()                      # wt_program_check's code: the package's equals the header's
    assert getattr(native, code) == int(re.search(code + r" = (\d)\b", header).group(1))
    assert source in native.BUILD_SOURCES
    for name in exports:
        assert name in wt.__all__ and hasattr(wt, name), name
    for name in methods:
        assert callable(getattr(wt.ReactorEnsemble, name)), name


def test_build_staleness_list_matches_the_includes():
    """``_native.build`` rebuilds when any source is newer than the library: the list must be wtphys.hip plus exactly
    the local headers it (transitively) includes -- no stale names, nothing missing."""
    import importlib
    native = importlib.import_module("ics-wt-physicsengine_amd.core._native")
    seen, todo = set(), ["wtphys.hip"]
    while todo:
        f = todo.pop()
        if f in seen:
            continue
        seen.add(f)
        text = open(os.path.join(native.CSRC, f)).read()
        todo += [m for m in re.findall(r'#include "([^"/]+)"', text) if os.path.exists(os.path.join(native.CSRC, m))]
    assert seen == set(native.BUILD_SOURCES)
    assert not [f for f in os.listdir(native.CSRC) if f.endswith((".hpp", ".hip")) and f not in seen], "dead source in csrc/"


def test_every_header_compiles_when_included_alone(tmp_path):
    """Each header in csrc/ names what it uses: a translation unit that includes it and nothing else passes the device
    compiler's front end (nothing is instantiated, so no code is generated)."""
    import importlib, shutil, subprocess
    from concurrent.futures import ThreadPoolExecutor
    native = importlib.import_module("ics-wt-physicsengine_amd.core._native")
    if shutil.which("hipcc") is None:
        pytest.skip("hipcc is not on the path")
    headers = sorted(f for f in os.listdir(native.CSRC) if f.endswith(".hpp"))
    assert set(headers) == {f for f in native.BUILD_SOURCES if f.endswith(".hpp")}

    def alone(h):
        unit = tmp_path / (h[:-4] + "_alone.hip")
        unit.write_text(f'#include "{h}"\n')
        p = subprocess.run(["hipcc", "--offload-arch=gfx950", "-std=c++17", "--cuda-device-only", "-fsyntax-only", "-x", "hip",
                            "-I", native.CSRC, str(unit)], capture_output=True, text=True)
        return h, p.returncode, p.stderr[-2000:]

    # one compiler call per header, four at a time (one after the other they take longer than any other CPU test)
    with ThreadPoolExecutor(4) as pool:
        failed = {h: err for h, rc, err in pool.map(alone, headers) if rc != 0}
    assert not failed, failed


def test_step_kernels_fit_the_register_file_and_four_wavefronts_per_cu(tmp_path):
    """Code-object metadata of the built library (what the loader sees): every step kernel up to 32 zones (LV <= 5,
    BASELINE config 3's n = 20 among them) runs without scratch memory, and its LDS leaves room for four wavefronts per
    CU (160 KiB / 4).  A register or LDS regression shows here, on the CPU, before it shows as a slower bench line."""
    import importlib, shutil, subprocess
    native = importlib.import_module("ics-wt-physicsengine_amd.core._native")
    llvm = "/opt/rocm/lib/llvm/bin"
    if not all(os.path.exists(os.path.join(llvm, t)) for t in ("llvm-objcopy", "clang-offload-bundler", "llvm-readelf")):
        pytest.skip("ROCm LLVM tools not installed")
    fat, dev = str(tmp_path / "fat.bin"), str(tmp_path / "dev.co")
    subprocess.run([f"{llvm}/llvm-objcopy", f"--dump-section=.hip_fatbin={fat}", os.path.join(native.CSRC, "libwtphys.so")], check=True)
    subprocess.run([f"{llvm}/clang-offload-bundler", "--type=o", "--unbundle", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
                    f"--input={fat}", f"--output={dev}"], check=True)
    notes = subprocess.run([f"{llvm}/llvm-readelf", "--notes", dev], check=True, capture_output=True, text=True).stdout
    seen = {}
    for block in notes.split("\n  - .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", block).group(1)
        m = re.search(r"step_kernelILi(\d)ELb(\d)", name)
        if not m:
            continue
        get = lambda f: int(re.search(re.escape(f) + r":\s+(\d+)", block).group(1))
        seen[(int(m.group(1)), bool(int(m.group(2))))] = (get(".private_segment_fixed_size"), get(".group_segment_fixed_size"),
                                                          get(".vgpr_count"))
    assert {(1, True), (2, True), (3, True), (4, True), (2, False), (3, False), (4, False), (5, False), (6, False)} <= set(seen)
    for (lv, row), (scratch, lds, regs) in seen.items():
        assert regs <= 512
        if lv <= 5:
            assert scratch == 0, (lv, row, scratch)
            assert lds <= 40960, (lv, row, lds)
