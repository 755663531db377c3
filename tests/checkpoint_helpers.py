"""Helpers of tests/test_gpu_checkpoint.py and tools/checkpoint_probe.py: a plant with everything in flight, and
``snapshot``, every getter of the library for the parts that are on."""
import ctypes
import struct

import numpy as np

from program_helpers import DT, _native, assert_all_equal, plant

HEADER = struct.Struct("<4sIIIqqQQIIQ")      # include/wtphys.h wt_checkpoint_header
SAVE_AT, AFTER = 190, (60, 50)               # the save is past the probes' warm-up (1800 s), off a scan boundary (chunk 7)
CHUNK = 7
T_SAVE = SAVE_AT * DT
ATTACK = (T_SAVE - 200.0, T_SAVE + 500.0)

INFO = ("PLANT_IO", "TRAIN", "PIPE", "SENSOR_HISTORY", "DISTURB_HISTORY", "SCORE_CURVE", "SCORE_BINS", "TREND_CAPACITY",
        "TRAIN_LENGTH", "WIRE", "MARK")      # every code but WT_INFO_BOUNDARY_UPLOADS and WT_INFO_WAVE_DIAG, and the programs'


def info_codes(ens):
    return np.array([ens.info(_native.WT_INFO_PROGRAM + p) for p in range(8)] +
                    [ens.info(getattr(_native, "WT_INFO_" + k)) for k in INFO])


def _flat(x):
    if x is None:
        return []
    if isinstance(x, np.ndarray):
        return [x]
    if isinstance(x, (tuple, list)):
        return [a for y in x for a in _flat(y)]
    if hasattr(x, "__dict__"):
        return _flat(list(vars(x).values()))
    return [np.asarray(x)]


def holding_words(ens):
    """The holding image (N, 6) as the device holds it: the library hands out its device address, no download call."""
    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    ir, hr = ctypes.c_void_p(), ctypes.c_void_p()
    _native.check(_native.lib().wt_ensemble_plc_device(ens._h, ctypes.byref(ir), ctypes.byref(hr)))
    ens.synchronize()
    out = np.zeros((ens.n_reactors, ens.HR_WORDS), dtype=np.uint16)
    assert hip.hipMemcpy(out.ctypes.data, hr, out.nbytes, 2) == 0     # hipMemcpyDeviceToHost
    return out


def snapshot(ens, layout=True):
    """Every getter of the library for the parts that are on, as one flat tuple of arrays.  ``layout=False`` leaves out
    what describes the wavefront packing (workers, reactors per wavefront), which a checkpoint does not carry."""
    info = info_codes(ens)
    prog = dict(zip(("control", "inject", "alarm", "actuator", "disturb", "score", "detect", "trend"), info[:8]))
    on = dict(zip(INFO, info[8:]))
    sched = ens.schedule()
    out = [info, ens.state, ens.status(), ens.bad_temperature(), ens.solver_stats(), ens.placement()[1],
           np.array([sched["mode"] == "queue", sched["streams"], sched["chunk"], sched["placement"] == "adaptive",
                     sched["cost_history_steps"]] + ([sched["workers"]] if layout else []))]
    try:
        out.append(ens.boundary())
    except _native.WtError:                   # before the first set_boundary
        out.append(None)
    try:
        out.append(ens.sensor_readings())
        if on["SENSOR_HISTORY"]:
            out.append(ens.sensor_history())
    except _native.WtError:
        pass
    if on["PLANT_IO"]:
        out += [ens.input_image(), holding_words(ens)]
    try:
        out.append(ens.trajectory())
    except _native.WtError:
        pass
    for name, getters in (("control", (ens.control_state,)), ("inject", (ens.injection_state,)),
                          ("alarm", (ens.alarm_state, ens.alarm_words)), ("actuator", (ens.actuator_state,)),
                          ("disturb", (ens.disturbance_state,) + ((ens.disturbance_history,) if on["DISTURB_HISTORY"] else ())),
                          ("score", (ens.score_state, ens.score_curve)), ("detect", (ens.detector_state,)),
                          ("trend", (ens.trend_state, ens.trend_data))):
        if prog[name]:
            out += [g() for g in getters] + [program_params(ens, name)]
    if on["TRAIN"]:
        st = ens.train_state()
        out += [st.n_fed, st.t_last, np.array([st.length] + ([st.per_wavefront] if layout else [])), train_params(ens)]
    if on["PIPE"]:
        out += [ens.pipe_state(), ens.pipe_lines()]
    if on["WIRE"]:
        out += [ens.wire_state(), ens.wire_params()]
    return tuple(_flat(out))


def _fields(name):
    """Rows of one slot of a program's parameter block, from the package's own block builders."""
    import importlib
    wt = importlib.import_module("ics-wt-physicsengine_amd")
    build = dict(control=wt.control_block, inject=wt.injection_block, alarm=wt.alarm_block, actuator=wt.actuator_block,
                 disturb=wt.disturbance_block, score=wt.score_block, detect=wt.detector_block, trend=wt.trend_block)[name]
    return build(1).shape[:2]


def program_params(ens, name):
    p = ("control", "inject", "alarm", "actuator", "disturb", "score", "detect", "trend").index(name)
    out = np.empty(_fields(name) + (ens.n_reactors,), dtype=np.float64)
    _native.check(_native.lib().wt_ensemble_program_params(ens._h, p, _native.dptr(out)))
    return out


def train_params(ens):
    out = np.empty((2, ens.n_reactors), dtype=np.float64)
    _native.check(_native.lib().wt_ensemble_train_params(ens._h, _native.dptr(out)))
    return out


def build(wt, cols, bc, n, length=0, programs=True, trend_capacity=16, seed=11):
    """A plant with everything in flight around ``T_SAVE``.  ``length`` > 1: trains with some stages unlinked, pipes
    with delays 0, 1 and 5, a wire from the last stage to the first.  ``programs`` False (the n > 32 kernel): core
    state, sensors and recording only."""
    N = len(cols["initial_chlorine"])
    r = np.arange(N)
    if not programs:
        ens = wt.ReactorEnsemble(cols, n_zones=n)
        ens.set_boundary(bc)
        ens.enable_sensors(seed=seed, history=64)
    else:
        ens = plant(wt, cols, bc, n, seed=seed, history=64)
    ens.set_schedule(0, CHUNK)
    ens.record(every=3, capacity=80)
    if not programs:
        return ens
    ens.write_commands(0.5, 0.25, 6.0)
    if length > 1:
        linked = np.ones(N)
        linked[length - 1::2 * length] = 0.0               # the last stage of every other train is not linked
        ens.set_trains(length, linked=linked, rows=np.where(r % 3 == 0, 3, 7))
        stage, delay = r % length, np.choose(r % 3, [0, 1, 5])
        ens.set_pipes(np.where((stage > 0) & (linked == 1.0), delay, 0))
        ens.set_wires(wt.Wire("chlorine_outlet", 0, length - 1))
    cl0 = np.asarray(cols["initial_chlorine"])
    u = np.random.default_rng(seed).random((4, N))
    ens.enable_control(wt.PILoop("chlorine_outlet", setpoint=cl0 + u[0], kp=0.2 + 1.8 * u[1], ki=1e-4 + 2e-3 * u[2], bias=0.2),
                       wt.PILoop("pH_outlet", setpoint=6.8 + 0.6 * u[3], kp=0.5, ki=1e-3, direction=-1, bias=0.1))
    ens.set_injections(wt.Injection("chlorine_outlet", "freeze", start=T_SAVE - 400.0, end=T_SAVE + 400.0),
                       wt.Injection("chlorine_flow_rate", "ramp", start=T_SAVE - 200.0, end=T_SAVE + 900.0, a=0.05, b=1e-4),
                       wt.Injection("temp_outlet", "bias", start=T_SAVE + 100.0, end=T_SAVE + 700.0, a=50.0))
    ens.set_alarms(wt.Alarm("temp_outlet", "high", 60.0, on_delay=100.0, latch=True, action="trip_acid", trip_value=0.3),
                   wt.Alarm("chlorine_outlet", "low", cl0 - 0.2 * u[0], deadband=0.05, source="field"))
    ens.set_actuators(wt.Actuator("chlorine", tau=40.0, rate=0.05, delay=3), wt.Actuator("acid", delay=2, rate=0.01))
    ens.set_disturbances(wt.Disturbance.ou("ambient_temperature", 0.5, 300.0),
                         wt.Disturbance.sine("chlorine_concentration", 2.0, 86400.0), seed=5, reactor_base=3, history=48)
    ens.set_scores(wt.Score("chlorine", 0.5, 3.0), wt.Score("pH", 6.5, 8.5, reduce="mean"), curve=400, bins=8,
                   fan_range=([0.0, 5.0, 0.0, 0.0], [6.0, 9.0, 1.0, 1.0]))
    ens.set_detectors(wt.Detector("chlorine_outlet", "cusum", 4.0, sigma=0.05, ref_value=cl0),
                      wt.Detector("pH_outlet", "ewma", 2.0, sigma=0.02, ref="track", tau=100.0), attack=ATTACK)
    ens.set_trends(wt.Trend("control", ("chlorine", "output")), wt.Trend("image_value", "chlorine_outlet", deadband=0.0),
                   wt.Trend("alarm_word", deadband=0.0), wt.Trend("actuator", ("chlorine", "position"), every=2),
                   capacity=trend_capacity, wrap=True)
    return ens


def same(what, ref, got):
    assert len(ref) == len(got), (what, len(ref), len(got))
    assert_all_equal(ref, got, what)


def both(what, a, b, layout=True):
    same(what, snapshot(a, layout), snapshot(b, layout))


def continue_alike(what, a, b, steps=(40,), layout=True):
    """The same further calls on both; the getters agree after each."""
    for i, k in enumerate(steps):
        a.step(DT, n_steps=k, download=False)
        b.step(DT, n_steps=k, download=False)
        both((what, "after call", i), a, b, layout)


def header_of(blob):
    return dict(zip(("magic", "format", "abi", "n_zones", "n_reactors", "bytes", "layout", "checksum", "n_parts", "r0", "r1"),
                    HEADER.unpack_from(blob)))


def with_header(blob, **fields):
    h = header_of(blob)
    h.update(fields)
    return HEADER.pack(*h.values()) + bytes(blob[HEADER.size:])
