"""Host-side mirror of the reference's reactor API over the HIP ensemble library.

``IntegratedCSTR(config).step(dt, boundary) -> ReactorState`` keeps the
reference's signature, field names, defaults and error behaviour
(/root/reference/src/wt_simulator/core/reactor.py:52-186, 203-227, 450-541) so
the unchanged sensor and Modbus layers can sit on top of it.
``ReactorEnsemble`` is the batched front door the reference does not have: N
independent reactors advanced by one kernel launch.  All arithmetic of the step
runs in ``csrc/`` on the GPU; this module only packs SoA blocks, moves buffers
and turns status bits back into the reference's exceptions and log lines.
"""
from __future__ import annotations

import ctypes as C
import logging
from dataclasses import dataclass, field, fields
from typing import Dict, Iterable, List, Optional, Sequence, Union

import numpy as np

from . import (_native, _program, actuator, alarm, control, detect, disturb, inject, install, junction, link, mpc, params, respond,
               score, service, train, trend, tune, wire)

logger = logging.getLogger(__name__)

ST_T_RANGE, ST_SOLVER_FAILED, ST_CLAMP_PH, ST_CLAMP_CL, ST_CLAMP_T, ST_T_RANGE_POST, ST_NONFINITE = (
    1, 2, 4, 8, 16, 32, 64)
ST_STEP_LIMIT = 128

_T_RANGE_TEXT = (
    "Temperature {value}°C outside liquid water range [0.0, 100.0]°C. This indicates either:\n"
    "  1. Invalid input data\n"
    "  2. Numerical instability in ODE integration (reduce tolerances)\n"
    "  3. System requires pressurized/supercooled water model")
_SOLVER_FAILED_TEXT = "ODE solver failed: Required step size is less than spacing between numbers."
_NONFINITE_TEXT = "All components of the initial state `y0` must be finite."   # scipy base.py:19-20, out of reactor.py:476


# --------------------------------------------------------------------------- dataclasses
@dataclass
class ReactorConfiguration:
    """Geometry, flow, chemistry and operating point of one CSTR (reactor.py:52-110)."""

    volume: float = 1000.0            # [L]
    height: float = 2.0               # [m]
    diameter: float = 0.798           # [m]
    n_zones: int = 5

    flow_rate: float = 5.0            # [L/min]
    turbulent_intensity: float = 0.15
    recirculation_ratio: float = 5.0
    impeller_speed: float = 60.0      # [rpm]
    impeller_diameter: float = 0.3    # [m]
    power_number: float = 5.0

    initial_pH: float = 7.0
    alkalinity: float = 100.0         # [mg/L as CaCO3]
    total_carbonate: float = 2.0      # [mmol/L]

    initial_chlorine: float = 2.0     # [mg/L]

    temperature: float = 20.0         # [degC]
    enable_thermal_stratification: bool = True

    inlet_pH: float = 7.5
    inlet_chlorine: float = 0.0
    inlet_temperature: float = 20.0

    def validate(self) -> None:
        """Same checks, same exception types as reactor.py:91-110."""
        calculated_volume = np.pi * (self.diameter / 2) ** 2 * self.height * 1000
        volume_error = abs(calculated_volume - self.volume) / self.volume
        if volume_error > 0.01:
            raise ValueError(
                f"Volume mismatch: specified {self.volume}L, "
                f"calculated {calculated_volume:.1f}L from geometry. "
                f"Error: {volume_error*100:.1f}%")
        assert 0 < self.volume < 1e6, "Volume out of range"
        assert 0 <= self.flow_rate < 1e5, "Flow rate out of range (use 0 for batch mode)"
        assert 0 <= self.initial_pH <= 14, "pH out of range"
        assert 0 <= self.initial_chlorine <= 10, "Chlorine out of range"
        assert 0 <= self.temperature <= 40, "Temperature out of typical range"


@dataclass
class ReactorState:
    """State of one reactor; every per-zone quantity is an array of length n_zones
    (reactor.py:113-147)."""

    time: float = 0.0
    pH: np.ndarray = field(default_factory=lambda: np.full(5, 7.0))
    chlorine: np.ndarray = field(default_factory=lambda: np.full(5, 2.0))
    temperature: np.ndarray = field(default_factory=lambda: np.full(5, 20.0))
    flow_rate: float = 5.0

    H_concentration: np.ndarray = field(init=False)
    density: np.ndarray = field(init=False)
    chlorine_decay_rate: np.ndarray = field(init=False)

    def __post_init__(self):
        self.update_derived()

    def update_derived(self):
        self.H_concentration = 10 ** (-self.pH)
        if not hasattr(self, "density"):
            self.density = np.full_like(self.pH, 998.2)
        if not hasattr(self, "chlorine_decay_rate"):
            self.chlorine_decay_rate = np.full_like(self.pH, 0.0001)

    def state_dict(self) -> Dict[str, object]:
        """Plain-dict view (the 'state-dict API' BASELINE.json mentions)."""
        return {f.name: getattr(self, f.name) for f in fields(self)}


@dataclass
class BoundaryConditions:
    """Physical streams entering the tank during a step (reactor.py:150-186)."""

    inlet_flow_rate: float = 5.0          # [L/min]
    inlet_pH: float = 7.5
    inlet_chlorine: float = 0.0           # [mg/L]
    inlet_temperature: float = 20.0       # [degC]
    acid_flow_rate: float = 0.0           # [L/min]
    acid_concentration: float = 0.1       # [mol/L]
    chlorine_flow_rate: float = 0.0       # [L/min]
    chlorine_concentration: float = 50.0  # [mg/L]
    ambient_temperature: float = 20.0     # [degC]
    heat_loss_coefficient: float = 0.0    # [W/K]


@dataclass
class EnsembleState:
    """State of N reactors; per-zone arrays are (N, n_zones), per-reactor arrays (N,)."""

    time: np.ndarray
    pH: np.ndarray
    chlorine: np.ndarray
    temperature: np.ndarray
    flow_rate: np.ndarray
    H_concentration: np.ndarray
    density: np.ndarray
    chlorine_decay_rate: np.ndarray
    status: np.ndarray

    def reactor(self, r: int) -> ReactorState:
        s = ReactorState(time=float(self.time[r]), pH=self.pH[r].copy(), chlorine=self.chlorine[r].copy(),
                         temperature=self.temperature[r].copy(), flow_rate=float(self.flow_rate[r]))
        s.H_concentration = self.H_concentration[r].copy()
        s.density = self.density[r].copy()
        s.chlorine_decay_rate = self.chlorine_decay_rate[r].copy()
        return s


@dataclass
class Trajectory:
    """Recorded states of N reactors (ReactorEnsemble.record / .trajectory): record i is what
    ``ReactorEnsemble.state`` would have shown after outer step (i + 1) * every since recording started."""

    time: np.ndarray          # (R, N)
    pH: np.ndarray            # (R, N, n_zones)
    chlorine: np.ndarray      # (R, N, n_zones)
    temperature: np.ndarray   # (R, N, n_zones)
    flow_rate: np.ndarray     # (R, N)
    status: np.ndarray        # (R, N) uint32 status words (ST_* bits)

    def __len__(self) -> int:
        return self.time.shape[0]


_CFG_FIELDS = [f.name for f in fields(ReactorConfiguration)]


def _columns_from_configs(configs: Sequence[ReactorConfiguration]) -> Dict[str, np.ndarray]:
    return {name: np.array([getattr(c, name) for c in configs]) for name in _CFG_FIELDS if name != "n_zones"}


def boundary_block(boundaries, n_reactors: int) -> np.ndarray:
    """(NB, N) float64 SoA block from a BoundaryConditions, a sequence of them, a
    dict of columns (scalars broadcast) or a ready block."""
    NB = params.NB
    if isinstance(boundaries, np.ndarray):
        blk = np.ascontiguousarray(boundaries, dtype=np.float64)
        if blk.shape != (NB, n_reactors):
            raise ValueError(f"boundary block must have shape {(NB, n_reactors)}, got {blk.shape}")
        return blk
    blk = np.empty((NB, n_reactors), dtype=np.float64)
    if isinstance(boundaries, BoundaryConditions):
        for i, name in enumerate(params.BOUNDARY_FIELDS):
            blk[i] = getattr(boundaries, name)
    elif isinstance(boundaries, dict):
        defaults = BoundaryConditions()
        for i, name in enumerate(params.BOUNDARY_FIELDS):
            blk[i] = np.asarray(boundaries.get(name, getattr(defaults, name)), dtype=np.float64)
    else:
        seq = list(boundaries)
        if len(seq) != n_reactors:
            raise ValueError(f"expected {n_reactors} boundary conditions, got {len(seq)}")
        for i, name in enumerate(params.BOUNDARY_FIELDS):
            blk[i] = [getattr(b, name) for b in seq]
    return blk


def boundary_schedule_block(schedule, n_steps: int, n_reactors: int) -> np.ndarray:
    """(K, NB, N) float64 block of a per-step boundary schedule: row k is the boundary of outer step k.  Takes an
    array (K, NB, N) or a sequence of K items that :func:`boundary_block` accepts; K must equal ``n_steps``."""
    NB = params.NB
    if isinstance(schedule, np.ndarray):
        blk = np.ascontiguousarray(schedule, dtype=np.float64)
        if blk.ndim != 3 or blk.shape[1:] != (NB, n_reactors):
            raise ValueError(f"boundary schedule must have shape (n_steps, {NB}, {n_reactors}), got {blk.shape}")
    else:
        rows = list(schedule)
        blk = np.empty((len(rows), NB, n_reactors), dtype=np.float64)
        for k, row in enumerate(rows):
            blk[k] = boundary_block(row, n_reactors)
    if blk.shape[0] != n_steps:
        raise ValueError(f"boundary schedule has {blk.shape[0]} rows for n_steps = {n_steps}")
    return blk


# --------------------------------------------------------------------------- ensemble
class ReactorEnsemble:
    """N independent multi-zone CSTRs resident on one MI355X.

    The whole of ``IntegratedCSTR.step`` (RHS + adaptive Radau + derived + clamps)
    runs inside one kernel; the host never sees intermediate values.
    """

    def __init__(self, configs: Union[Sequence[ReactorConfiguration], Dict[str, np.ndarray]],
                 n_zones: Optional[int] = None, device: int = 0, validate: bool = True):
        if isinstance(configs, dict):
            if n_zones is None:
                raise ValueError("n_zones is required with column input")
            cols = {k: np.atleast_1d(np.asarray(v)) for k, v in configs.items()}
            N = max(v.shape[0] for v in cols.values())
            defaults = ReactorConfiguration()
            for name in _CFG_FIELDS:
                if name == "n_zones":
                    continue
                v = cols.get(name, np.asarray([getattr(defaults, name)]))
                cols[name] = np.broadcast_to(v, (N,)).copy()
            if validate:
                _validate_columns(cols)
        else:
            configs = list(configs)
            if not configs:
                raise ValueError("need at least one reactor")
            nz = {c.n_zones for c in configs}
            if len(nz) != 1:
                raise ValueError("all reactors of one ensemble must have the same n_zones")
            n_zones = nz.pop()
            if validate:
                for c in configs:
                    c.validate()
            cols = _columns_from_configs(configs)
            N = len(configs)
        if n_zones < 2:
            raise ValueError(f"Need at least 2 zones, got {n_zones}")       # transport.py:88-89
        self.n_reactors = int(N)
        self.n_zones = int(n_zones)
        self.device = int(device)
        self.columns = cols
        self.constants = params.derive_constants(cols, self.n_zones)
        self._h = C.c_void_p()
        L = _native.lib()
        _native.check(L.wt_ensemble_create(self.n_reactors, self.n_zones, self.device,
                                           _native.dptr(np.ascontiguousarray(self.constants)), C.byref(self._h)))
        shape = (self.n_reactors, self.n_zones)
        self.set_state(np.broadcast_to(np.asarray(cols["initial_pH"], dtype=np.float64)[:, None], shape),
                       np.broadcast_to(np.asarray(cols["initial_chlorine"], dtype=np.float64)[:, None], shape),
                       np.broadcast_to(np.asarray(cols["temperature"], dtype=np.float64)[:, None], shape),
                       np.zeros(self.n_reactors))
        # nothing else is kept here: what is switched on, every capacity and the boundary block last uploaded live in
        # the handle, and the methods below ask it (info, and the library's own getters)

    # -- lifetime
    def close(self) -> None:
        if getattr(self, "_h", None) is not None and self._h:
            _native.lib().wt_ensemble_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- data movement
    def set_state(self, pH, chlorine, temperature, time=None) -> None:
        shape = (self.n_reactors, self.n_zones)
        a = [np.ascontiguousarray(np.broadcast_to(np.asarray(x, dtype=np.float64), shape)) for x in (pH, chlorine, temperature)]
        t = None if time is None else np.ascontiguousarray(np.broadcast_to(np.asarray(time, dtype=np.float64), (self.n_reactors,)))
        _native.check(_native.lib().wt_ensemble_set_state(self._h, _native.dptr(a[0]), _native.dptr(a[1]),
                                                          _native.dptr(a[2]), _native.dptr(t)))

    def set_boundary(self, boundaries) -> None:
        """The boundary of every reactor from now on.  The library uploads the block unless the device still holds
        exactly these bytes (``info(WT_INFO_BOUNDARY_UPLOADS)`` counts the uploads)."""
        blk = boundary_block(boundaries, self.n_reactors)
        _native.check(_native.lib().wt_ensemble_set_boundary(self._h, _native.dptr(blk)))

    def info(self, what: int) -> int:
        """One of the handle's switches, capacities or counters (``_native.WT_INFO_*``); no synchronisation."""
        v = C.c_int64(0)
        _native.check(_native.lib().wt_ensemble_info(self._h, int(what), C.byref(v)))
        return int(v.value)

    def step(self, dt: float, boundaries=None, n_steps: int = 1, fused: bool = True,
             download: bool = True, boundary_schedule=None) -> Optional[EnsembleState]:
        """Advance every reactor ``n_steps`` outer steps of length ``dt`` [s].

        ``boundary_schedule``: one boundary per outer step, (n_steps, NB, N) or a sequence of n_steps items
        :func:`boundary_block` accepts -- the same bits as ``set_boundary(S[k]); step(dt, n_steps=1)`` for every k, in
        one fused call.  Afterwards the boundary is ``S[-1]``.  Not with ``boundaries``, not under plant I/O."""
        if boundary_schedule is not None:
            if boundaries is not None:
                raise ValueError("give either boundaries or boundary_schedule, not both")
            blk = boundary_schedule_block(boundary_schedule, int(n_steps), self.n_reactors)
            try:
                _native.check(_native.lib().wt_ensemble_step_scheduled(self._h, float(dt), int(n_steps), 1 if fused else 0,
                                                                       _native.dptr(blk)))
            except _native.WtError as e:
                if e.code in (_native.WT_E_ARG, _native.WT_E_STATE):
                    raise ValueError(e.message) from None
                raise
            return self.state if download else None
        if boundaries is not None:
            self.set_boundary(boundaries)
        try:
            _native.check(_native.lib().wt_ensemble_step(self._h, float(dt), int(n_steps), 1 if fused else 0))
        except _native.WtError as e:
            if e.code in (_native.WT_E_ARG, _native.WT_E_STATE):
                raise ValueError(e.message) from None
            raise
        return self.state if download else None

    def record(self, every: int = 1, capacity: int = 0) -> None:
        """Record the state after every ``every``-th outer step of later :meth:`step` calls (scheduled or not), up to
        ``capacity`` records; then recording stops.  ``capacity=0`` switches it off.  Calling it again restarts."""
        try:
            _native.check(_native.lib().wt_ensemble_record(self._h, int(every), int(capacity)))
        except _native.WtError as e:
            if e.code == _native.WT_E_ARG:
                raise ValueError(e.message) from None
            raise

    def trajectory(self) -> Trajectory:
        """The records taken since :meth:`record` (one synchronisation per call)."""
        L = _native.lib()
        nr = C.c_int(0)
        _native.check(L.wt_ensemble_get_record(self._h, None, None, None, None, None, None, C.byref(nr)))
        R, N, n = nr.value, self.n_reactors, self.n_zones
        pH, Cl, T = np.empty((R, N, n)), np.empty((R, N, n)), np.empty((R, N, n))
        t, flow, st = np.empty((R, N)), np.empty((R, N)), np.zeros((R, N), dtype=np.uint32)
        _native.check(L.wt_ensemble_get_record(self._h, _native.dptr(pH), _native.dptr(Cl), _native.dptr(T), _native.dptr(t),
                                               _native.dptr(flow), st.ctypes.data_as(C.POINTER(C.c_uint32)), C.byref(nr)))
        return Trajectory(time=t, pH=pH, chlorine=Cl, temperature=T, flow_rate=flow, status=st)

    def set_schedule(self, n_streams: int = 0, chunk_steps: int = 50) -> None:
        """Advance the ensemble as ``n_streams`` contiguous reactor ranges on internal HIP
        streams (0 = the library default), at most ``chunk_steps`` outer steps per launch
        (0 = one launch per call)."""
        _native.check(_native.lib().wt_ensemble_set_schedule(self._h, int(n_streams), int(chunk_steps)))

    def schedule(self) -> Dict[str, object]:
        """The schedule in force: {"mode", "streams", "chunk", "workers", "kernel", "placement"}."""
        m, s, c, w = C.c_int(0), C.c_int(0), C.c_int(0), C.c_int(0)
        _native.check(_native.lib().wt_ensemble_get_schedule(self._h, C.byref(m), C.byref(s), C.byref(c), C.byref(w)))
        mode = {0: "streams", 1: "queue"}.get(m.value, str(m.value))
        pm = C.c_int(0)
        _native.check(_native.lib().wt_ensemble_get_placement(self._h, C.byref(pm), None))
        rd, hs = C.c_int64(0), C.c_int64(0)
        _native.check(_native.lib().wt_ensemble_placement_info(self._h, C.byref(rd), C.byref(hs)))
        return {"mode": mode, "streams": s.value, "chunk": c.value, "workers": w.value,
                "kernel": "wt::step_kernel", "placement": "adaptive" if pm.value else "identity",
                "redeals": int(rd.value), "cost_history_steps": int(hs.value)}

    def item_steps(self, n_steps: int) -> int:
        """Outer steps a reactor's state stays in registers before it returns to memory in a call of ``n_steps``."""
        return int(_native.lib().wt_ensemble_item_steps(self._h, int(n_steps)))

    def set_step_limit(self, max_attempts: int) -> None:
        """Stop a reactor that needs more than ``max_attempts`` Radau step attempts in one outer step
        (status SOLVER_FAILED | STEP_LIMIT).  0 = unlimited, which is what the reference does."""
        _native.check(_native.lib().wt_ensemble_set_step_limit(self._h, int(max_attempts)))

    def set_placement(self, adaptive: bool) -> None:
        """Which reactors share a wavefront.  ``True`` (default): once 32 outer steps of solver counters are in, the
        next :meth:`step` call re-deals the wavefront slots in order of solver cost, so a wavefront no longer waits for
        one expensive reactor among cheap ones.  ``False``: reactor r in slot r.  Results do not depend on it."""
        _native.check(_native.lib().wt_ensemble_set_placement(self._h, 1 if adaptive else 0))

    def placement(self):
        """(adaptive?, slot -> reactor index table)."""
        mode = C.c_int(0)
        perm = np.empty(self.n_reactors, dtype=np.int32)
        _native.check(_native.lib().wt_ensemble_get_placement(self._h, C.byref(mode), perm.ctypes.data_as(C.POINTER(C.c_int32))))
        return bool(mode.value), perm

    def set_sync(self, sync_outer: bool) -> None:
        _native.check(_native.lib().wt_ensemble_set_sync(self._h, 1 if sync_outer else 0))

    def launch_timing(self, enable: bool = True) -> None:
        _native.check(_native.lib().wt_ensemble_launch_timing(self._h, 1 if enable else 0))

    def launch_stats(self):
        """(number of step-kernel launches, sum of their durations [ms], longest [ms]) since the last call."""
        n, s, m = C.c_int64(0), C.c_double(0.0), C.c_double(0.0)
        _native.check(_native.lib().wt_ensemble_launch_stats(self._h, C.byref(n), C.byref(s), C.byref(m)))
        return int(n.value), float(s.value), float(m.value)

    def synchronize(self) -> None:
        _native.check(_native.lib().wt_ensemble_synchronize(self._h))

    @property
    def state(self) -> EnsembleState:
        N, n = self.n_reactors, self.n_zones
        pH, Cl, T = np.empty((N, n)), np.empty((N, n)), np.empty((N, n))
        H, rho, kd = np.empty((N, n)), np.empty((N, n)), np.empty((N, n))
        t, flow = np.empty(N), np.empty(N)
        st = np.zeros(N, dtype=np.uint32)
        _native.check(_native.lib().wt_ensemble_get_snapshot(
            self._h, _native.dptr(pH), _native.dptr(Cl), _native.dptr(T), _native.dptr(t), _native.dptr(flow),
            _native.dptr(H), _native.dptr(rho), _native.dptr(kd), st.ctypes.data_as(C.POINTER(C.c_uint32))))
        return EnsembleState(time=t, pH=pH, chlorine=Cl, temperature=T, flow_rate=flow,
                             H_concentration=H, density=rho, chlorine_decay_rate=kd, status=st)

    def status(self) -> np.ndarray:
        st = np.zeros(self.n_reactors, dtype=np.uint32)
        _native.check(_native.lib().wt_ensemble_get_status(self._h, st.ctypes.data_as(C.POINTER(C.c_uint32))))
        return st

    def bad_temperature(self) -> np.ndarray:
        """(N,) the temperature the reference's ValueError names (thermodynamics.py:151) for reactors whose
        status carries T_RANGE / T_RANGE_POST; undefined for the others."""
        v = np.zeros(self.n_reactors)
        _native.check(_native.lib().wt_ensemble_get_bad_temperature(self._h, _native.dptr(v)))
        return v

    def clear_status(self) -> None:
        _native.check(_native.lib().wt_ensemble_clear_status(self._h))

    def solver_stats(self) -> np.ndarray:
        """(N, 5) int32: nfev, njev, nlu, accepted, rejected of the last outer step."""
        arr = np.zeros((self.n_reactors, 5), dtype=np.int32)
        _native.check(_native.lib().wt_ensemble_get_stats(self._h, arr.ctypes.data_as(C.POINTER(_native.SolverStats))))
        return arr

    def derivatives(self, pH, chlorine, temperature):
        """Batched ``IntegratedCSTR.derivatives`` at the given states; returns (dpH, dCl, dT, flags)."""
        shape = (self.n_reactors, self.n_zones)
        a = [np.ascontiguousarray(np.broadcast_to(np.asarray(x, dtype=np.float64), shape)) for x in (pH, chlorine, temperature)]
        out = [np.empty(shape) for _ in range(3)]
        fl = np.zeros(self.n_reactors, dtype=np.uint32)
        _native.check(_native.lib().wt_ensemble_rhs(self._h, *[_native.dptr(x) for x in a], *[_native.dptr(x) for x in out],
                                                   fl.ctypes.data_as(C.POINTER(C.c_uint32))))
        return out[0], out[1], out[2], fl

    # -- fused sensor suite (NEXT-1)
    SENSOR_NAMES = _program.SENSOR_NAMES

    def enable_sensors(self, seed: int = 0x5EED, reactor_base: int = 0, history: int = 0) -> None:
        """Attach the reference's seven-sensor suite (``create_realistic_sensor_suite`` +
        ``initialize_sensors``) to every reactor, calibrated now; every later outer step is followed by
        ``read_all_sensors`` on the device.  ``history`` > 0 keeps that many reads per sensor."""
        c = self.columns
        d = ReactorConfiguration()
        col = lambda k: np.ascontiguousarray(np.broadcast_to(np.asarray(c.get(k, getattr(d, k)), dtype=np.float64), (self.n_reactors,)))
        _native.check(_native.lib().wt_ensemble_sensors_enable(
            self._h, C.c_uint64(int(seed) & 0xFFFFFFFFFFFFFFFF), int(reactor_base), _native.dptr(col("flow_rate")),
            _native.dptr(col("initial_chlorine")), _native.dptr(col("temperature")), int(history)))

    def sensor_readings(self):
        """(values float32 (7, N), status uint8 (7, N), fault uint8 (7, N)) of the last read."""
        N = self.n_reactors
        v = np.empty((7, N), dtype=np.float32); s = np.empty((7, N), dtype=np.uint8); f = np.empty((7, N), dtype=np.uint8)
        u8 = C.POINTER(C.c_uint8)
        _native.check(_native.lib().wt_ensemble_sensors_get(self._h, v.ctypes.data_as(C.POINTER(C.c_float)),
                                                            s.ctypes.data_as(u8), f.ctypes.data_as(u8)))
        return v, s, f

    def sensor_history(self):
        """(values (H, 7, N), status, fault, reads per reactor (N,)) recorded since enable_sensors(history=H)."""
        N, H = self.n_reactors, self.info(_native.WT_INFO_SENSOR_HISTORY)
        v = np.empty((H, 7, N), dtype=np.float32); s = np.empty((H, 7, N), dtype=np.uint8); f = np.empty((H, 7, N), dtype=np.uint8)
        n = np.zeros(N, dtype=np.int32)
        u8 = C.POINTER(C.c_uint8)
        _native.check(_native.lib().wt_ensemble_sensors_history(self._h, v.ctypes.data_as(C.POINTER(C.c_float)), s.ctypes.data_as(u8),
                                                                f.ctypes.data_as(u8), n.ctypes.data_as(C.POINTER(C.c_int32))))
        return v, s, f, n

    # -- the service program: calibrate, clean and replace the instruments, on the device (wt_svc.hpp)
    def set_services(self, *services: "service.Service") -> None:
        """Run a service program of up to four :class:`Service` slots after every read, inside the step call: a slot
        calibrates, cleans or replaces one sensor at a suite time (once or periodically) or some time after a read
        returned a status; the action changes the next read, never the one just taken -- the bits of a host that
        makes one-step calls and calls :meth:`service_sensors` in between.  Replaces any program and resets the slot
        state.  Needs :meth:`enable_sensors` (not plant I/O) and at most 32 zones per reactor."""
        blk = service.service_block(self.n_reactors, *services)
        self._program_call(_native.lib().wt_ensemble_service_set, _native.dptr(blk))

    def service_state(self) -> "service.ServiceState":
        """Services done, the time of the last, the next due time and the open work order of every slot by reactor
        (one synchronisation)."""
        blk = np.empty((service.SLOTS, service.NSVS, self.n_reactors), dtype=np.float64)
        self._program_call(_native.lib().wt_ensemble_service_get, _native.dptr(blk))
        return service.ServiceState.from_block(blk)

    def service_params(self) -> np.ndarray:
        """The (4, 12, N) block of the service program in force, as :func:`service_block` built it."""
        blk = np.empty((service.SLOTS, service.NSV, self.n_reactors), dtype=np.float64)
        self._program_call(_native.lib().wt_ensemble_program_params, _native.WT_PROG_SERVICE, _native.dptr(blk))
        return blk

    def reset_services(self) -> None:
        """Slot state back to its set-time values: counts 0, every timed slot due at its first time again, no work
        order open.  The sensors keep what the services did to them."""
        self._program_call(_native.lib().wt_ensemble_service_reset)

    def clear_services(self) -> None:
        """Stop the service program; the sensors keep what the services did to them."""
        self._program_call(_native.lib().wt_ensemble_service_clear)

    def service_sensors(self, sensor, action, ref=0.0, ref2=0.0, ref_mode="constant", mask=None) -> None:
        """One maintenance action now, on one sensor of every reactor ``mask`` selects ((N,) bool; None: all): what a
        :class:`Service` slot does when it falls due, at the time and with the taps of the stored state.  ``ref`` and
        ``ref2``: scalars or (N,) arrays.  Works at any zone count."""
        N = self.n_reactors
        code = lambda v, names, what: int(_program.codes(v, names, what)) if isinstance(v, str) else int(v)
        col = lambda v: np.ascontiguousarray(np.broadcast_to(np.asarray(v, dtype=np.float64), (N,)))
        m = None
        if mask is not None:
            m = np.ascontiguousarray(np.broadcast_to(np.asarray(mask), (N,)).astype(bool).astype(np.uint8))
        self._program_call(_native.lib().wt_ensemble_sensors_service, code(sensor, _program.SENSOR_NAMES, "sensor"),
                           code(action, service.ACTIONS, "action"), code(ref_mode, service.REF_MODES, "ref_mode"),
                           _native.dptr(col(ref)), _native.dptr(col(ref2)),
                           None if m is None else m.ctypes.data_as(C.POINTER(C.c_uint8)))

    def sensor_health(self) -> Dict[str, np.ndarray]:
        """What the maintenance decisions look at, by name of :data:`service.HEALTH_ROWS`, (7, N) float64 each: the
        calibration offset and time, the power-on (warm-up) time, the three slow ageing fields of the sensor's kind
        (pH: fouling, days since cleaning, reference contamination; amperometric: fouling, membrane age; DPD: potency,
        light hours, reagent age; flow: electrode fouling), and the instrument's status and fault."""
        out = np.empty((7, service.NSH, self.n_reactors), dtype=np.float64)
        self._program_call(_native.lib().wt_ensemble_sensors_health, _native.dptr(out))
        return {k: np.array(out[:, i]) for i, k in enumerate(service.HEALTH_ROWS)}

    # -- the installation: every reactor's own sample lines and InstallationQuality (wt_ins.hpp)
    def set_installation(self, inst: "install.Installation") -> None:
        """Give every reactor its own sample lines and instrument installation (:class:`Installation`) from the next
        read on; needs the sensor suite.  Replaces the installation in force.  Mid-run the lines keep their samples
        and only the delay changes."""
        blk = install.installation_block(self.n_reactors, inst)
        self._program_call(_native.lib().wt_ensemble_install_set, _native.dptr(blk))

    def installation(self) -> np.ndarray:
        """The (9, N) block of the installation in force, rows in :data:`install.PARAM_ROWS` order; the suite's own
        build while none is set."""
        blk = np.empty((install.NINS, self.n_reactors), dtype=np.float64)
        self._program_call(_native.lib().wt_ensemble_install_get, _native.dptr(blk))
        return blk

    def clear_installation(self) -> None:
        """Back to the suite's own build for every reactor (250 mL at 500 mL/min, 0.5 m/s, no bubbles, grounding 0.9,
        vibration 0.1 g, ambient 30 degC)."""
        self._program_call(_native.lib().wt_ensemble_install_clear)

    # -- plant I/O: one virtual Modbus slave per reactor (NEXT-2 / NEXT-3)
    INPUT_REGISTERS = {"pH_inlet": 0, "pH_middle": 2, "pH_outlet": 4, "chlorine_inlet": 6, "chlorine_outlet": 8, "flow_rate": 10,
                       "temperature_inlet": 12, "temperature_outlet": 14, "simulation_time": 100, "system_status": 102}
    HOLDING_REGISTERS = {"acid_flow_rate": 0, "chlorine_flow_rate": 2, "inlet_flow_rate": 4}
    DISCRETE_INPUTS = {"sensor_fault_pH_inlet": 0, "sensor_fault_pH_outlet": 1, "sensor_fault_chlorine": 2}
    IR_WORDS, HR_WORDS = 20, 6

    def enable_plant_io(self) -> None:
        """Keep the reference loop's Modbus data blocks for every reactor on the device: after each launch
        of :meth:`step` (one PLC scan; ``fused=False`` scans every outer step like ``__main__.main``) the
        input image is refreshed from the sensor readings (``update_modbus_inputs``) and the holding image
        is validated into the boundary conditions (``read_modbus_commands`` + ``apply_boundary_conditions``)."""
        _native.check(_native.lib().wt_ensemble_plc_enable(self._h))

    @staticmethod
    def encode_float32(values) -> np.ndarray:
        """``ModbusEncoder.float32_to_registers`` for an array: (..., 2) uint16 = (high word, low word)."""
        bits = np.ascontiguousarray(values, dtype=np.float64).astype(np.float32).view(np.uint32)
        return np.stack([(bits >> 16).astype(np.uint16), (bits & 0xFFFF).astype(np.uint16)], axis=-1)

    @staticmethod
    def decode_float32(words) -> np.ndarray:
        """``ModbusDecoder.registers_to_float32`` for an array (..., 2) of (high, low) words."""
        w = np.asarray(words).astype(np.uint32)
        return ((w[..., 0] << 16) | w[..., 1]).astype(np.uint32).view(np.float32)

    def write_holding(self, words, first_reactor: int = 0) -> None:
        """Overwrite the holding image (count, 6) uint16 of reactors first_reactor.. (what masters wrote)."""
        w = np.ascontiguousarray(words, dtype=np.uint16)
        if w.ndim != 2 or w.shape[1] != self.HR_WORDS:
            raise ValueError(f"holding image must be (count, {self.HR_WORDS}) uint16")
        _native.check(_native.lib().wt_ensemble_plc_write_holding(self._h, w.ctypes.data_as(C.POINTER(C.c_uint16)),
                                                                 int(first_reactor), int(w.shape[0])))

    def write_commands(self, acid_flow_rate, chlorine_flow_rate, inlet_flow_rate, first_reactor: int = 0) -> None:
        """``slave.write_holding_register`` of the three actuator setpoints for a block of reactors
        (arrays: one entry per reactor starting at ``first_reactor``; all scalars: every reactor from there on)."""
        raw = [np.asarray(c, dtype=np.float64) for c in (acid_flow_rate, chlorine_flow_rate, inlet_flow_rate)]
        cols = [np.atleast_1d(c) for c in raw]
        # scalars only: the same setpoints for every reactor from first_reactor on
        cnt = (self.n_reactors - int(first_reactor)) if all(c.ndim == 0 for c in raw) else max(c.shape[0] for c in cols)
        w = np.concatenate([self.encode_float32(np.broadcast_to(c, (cnt,))) for c in cols], axis=1)
        self.write_holding(w, first_reactor)

    def input_image(self):
        """(image (N, 20) uint16, update_ok (N,) bool) -- layout in include/wtphys.h."""
        img = np.empty((self.n_reactors, self.IR_WORDS), dtype=np.uint16); ok = np.empty(self.n_reactors, dtype=np.uint8)
        _native.check(_native.lib().wt_ensemble_plc_read_inputs(self._h, img.ctypes.data_as(C.POINTER(C.c_uint16)),
                                                               ok.ctypes.data_as(C.POINTER(C.c_uint8))))
        return img, ok.astype(bool)

    def input_blocks(self, reactor: int, image: Optional[np.ndarray] = None):
        """The reference's ``ir_block`` (200 words) and ``di_block`` (100 bits) of one reactor as lists."""
        img = self.input_image()[0] if image is None else image
        row = img[reactor]
        ir = [0] * 200; di = [0] * 100
        ir[0:16] = [int(x) for x in row[0:16]]; ir[100:103] = [int(x) for x in row[16:19]]
        for b in range(3):
            di[b] = (int(row[19]) >> b) & 1
        return ir, di

    def boundary(self) -> np.ndarray:
        """Current boundary block (10, N) in BoundaryConditions field order (after the command path)."""
        out = np.empty((len(params.BOUNDARY_FIELDS), self.n_reactors), dtype=np.float64)
        _native.check(_native.lib().wt_ensemble_get_boundary(self._h, _native.dptr(out)))
        return out

    def _program_call(self, fn, *args) -> None:
        """A call of one of the ten per-reactor programs: a refusal is the caller's ValueError."""
        try:
            _native.check(fn(self._h, *args))
        except _native.WtError as e:
            if e.code in (_native.WT_E_ARG, _native.WT_E_STATE):
                raise ValueError(e.message) from None
            raise

    # -- PI dosing programs at every PLC scan, on the device (wt_ctl.hpp)
    def enable_control(self, chlorine: Optional["control.PILoop"] = None, acid: Optional["control.PILoop"] = None) -> None:
        """Run up to two PI loops per reactor at every PLC scan, inside the step call: ``chlorine`` writes the
        chlorine_flow_rate holding register, ``acid`` the acid_flow_rate one; a loop left out stays off and its
        register free for :meth:`write_commands`.  Each enabled loop starts with integral 0 and output
        ``clip(bias, out_min, out_max)``.  The output acts from the next scan on, exactly as a host master writing
        between two calls of one scan interval would.  Needs :meth:`enable_plant_io`."""
        blk = control.control_block(self.n_reactors, chlorine, acid)
        self._program_call(_native.lib().wt_ensemble_control_enable, _native.dptr(blk))

    def retune_control(self, chlorine=None, acid=None) -> None:
        """New parameters for running loops: a :class:`PILoop` replaces a loop's parameters, ``None`` keeps them,
        ``False`` switches the loop off.  Integral, output and metrics stay; a loop switched on starts as at enable."""
        blk = np.empty((len(control.LOOPS), control.NC, self.n_reactors), dtype=np.float64)
        if chlorine is None or acid is None:    # a loop that is kept: its rows as the library holds them
            self._program_call(_native.lib().wt_ensemble_program_params, _native.WT_PROG_CONTROL, _native.dptr(blk))
        for i, (name, loop) in enumerate(zip(control.LOOPS, (chlorine, acid))):
            if loop is not None:
                blk[i] = control.loop_rows(loop, name, self.n_reactors)
        self._program_call(_native.lib().wt_ensemble_control_retune, _native.dptr(blk))

    def disable_control(self) -> None:
        """Stop the PI programs; the holding registers keep their last outputs."""
        self._program_call(_native.lib().wt_ensemble_control_disable)

    def control_state(self) -> "control.ControlState":
        """Integral, output and metrics of both loops by reactor (one synchronisation)."""
        blk = np.empty((len(control.LOOPS), control.NCS, self.n_reactors), dtype=np.float64)
        self._program_call(_native.lib().wt_ensemble_control_get, _native.dptr(blk))
        return control.ControlState.from_block(blk)

    # -- relay autotune programs at every PLC scan, before the PI programs, on the device (wt_tun.hpp)
    def set_tuners(self, chlorine: Optional["tune.RelayTune"] = None, acid: Optional["tune.RelayTune"] = None) -> None:
        """Run up to two relay experiments per reactor at the PLC scans, inside the step call: ``chlorine`` owns the
        chlorine_flow_rate holding register while it runs, ``acid`` the acid_flow_rate one, and the PI loop of that
        register is skipped meanwhile.  An experiment starts at the first scan whose loop time reaches its ``start``;
        with ``commission`` it writes the gains it found into the PI loop (:meth:`enable_control` first).  Replaces any
        program and resets the state.  Needs :meth:`enable_plant_io` and at most 32 zones per reactor."""
        blk = tune.tune_block(self.n_reactors, chlorine, acid)
        self._program_call(_native.lib().wt_ensemble_tune_set, _native.dptr(blk))

    def tuner_state(self) -> "tune.TunerState":
        """Phase, relay, cycle sums, period, amplitude, Ku and the gains of both tuners by reactor (one
        synchronisation)."""
        blk = np.empty((len(control.LOOPS), tune.NUS, self.n_reactors), dtype=np.float64)
        self._program_call(_native.lib().wt_ensemble_tune_get, _native.dptr(blk))
        return tune.TunerState.from_block(blk)

    def tuner_params(self) -> np.ndarray:
        """The (2, 14, N) block of the tune program in force, as :func:`tune_block` built it."""
        blk = np.empty((len(control.LOOPS), tune.NU, self.n_reactors), dtype=np.float64)
        self._program_call(_native.lib().wt_ensemble_program_params, _native.WT_PROG_TUNE, _native.dptr(blk))
        return blk

    def reset_tuners(self) -> None:
        """Every tuner waiting again, its state zeroed: an experiment whose ``start`` has passed begins again at the
        next scan.  Gains already commissioned stay in the PI loops."""
        self._program_call(_native.lib().wt_ensemble_tune_reset)

    def clear_tuners(self) -> None:
        """Stop the tune program; the holding registers and commissioned gains stay as they are."""
        self._program_call(_native.lib().wt_ensemble_tune_clear)

    # -- model predictive controllers at the PLC scans, between tune and PI programs, on the device (wt_mpc.hpp)
    def set_mpc(self, chlorine: Optional["mpc.DMCLoop"] = None, acid: Optional["mpc.DMCLoop"] = None) -> None:
        """Run up to two dynamic matrix controllers per reactor at the PLC scans, inside the step call: ``chlorine``
        owns the chlorine_flow_rate holding register from its ``t_start`` on, ``acid`` the acid_flow_rate one, and the PI
        loop of that register is skipped meanwhile; a relay experiment (:meth:`set_tuners`) still takes the loop while
        it runs.  Replaces any controllers and resets state and prediction.  Needs :meth:`enable_plant_io` and at most
        32 zones per reactor."""
        blocks = mpc.mpc_block(self.n_reactors, chlorine, acid)
        self._program_call(_native.lib().wt_ensemble_mpc_set, *(_native.dptr(b) for b in blocks))

    def mpc_state(self) -> "mpc.MpcState":
        """Phase, output, bias, last move, metrics and counts of both controllers by reactor (one synchronisation)."""
        blk = np.empty((len(control.LOOPS), mpc.NMS, self.n_reactors), dtype=np.float64)
        self._program_call(_native.lib().wt_ensemble_mpc_get, _native.dptr(blk))
        return mpc.MpcState.from_block(blk)

    def mpc_prediction(self) -> np.ndarray:
        """The (2, 64, N) predictions: entry i is the reading a controller expects i of its periods after its last
        execution if the output stays where it is."""
        blk = np.empty((len(control.LOOPS), mpc.H, self.n_reactors), dtype=np.float64)
        self._program_call(_native.lib().wt_ensemble_mpc_prediction, _native.dptr(blk))
        return blk

    def mpc_params(self):
        """The (2, 10, N) parameter block and the (2, 64, N) step and gain blocks of the controllers in force, as
        :func:`mpc_block` built them."""
        n = self.n_reactors
        blocks = (np.empty((len(control.LOOPS), mpc.NM, n)), np.empty((len(control.LOOPS), mpc.H, n)),
                  np.empty((len(control.LOOPS), mpc.H, n)))
        self._program_call(_native.lib().wt_ensemble_mpc_params, *(_native.dptr(b) for b in blocks))
        return blocks

    def reset_mpc(self) -> None:
        """Every controller waiting again, state and prediction zeroed: it starts afresh from ``u0`` at the next due
        scan with a valid reading.  The holding registers stay as they are."""
        self._program_call(_native.lib().wt_ensemble_mpc_reset)

    def clear_mpc(self) -> None:
        """Stop the controllers; the holding registers stay as they are and the PI programs resume."""
        self._program_call(_native.lib().wt_ensemble_mpc_clear)

    # -- response programs at every PLC scan, between the tune program and the controllers, on the device (wt_rsp.hpp)
    def set_responses(self, *responses: "respond.Response") -> None:
        """Run a response program of up to four :class:`Response` slots at every PLC scan, inside the step call: a slot
        whose cause (an active alarm slot, a detector slot in alarm, a bad reading) has stood for its ``delay`` takes its
        dosing loop from the PI and model predictive controllers, holds or drives the holding register, and hands the
        loop back when the cause has been clear for ``clear_delay``.  The lowest engaged slot of a loop owns it; a relay
        experiment (:meth:`set_tuners`) keeps a loop it has.  Replaces any program and restarts the state.  Needs
        :meth:`enable_plant_io` and at most 32 zones per reactor."""
        block = respond.response_block(self.n_reactors, *responses)
        self._program_call(_native.lib().wt_ensemble_respond_set, _native.dptr(block))

    def response_state(self) -> "respond.ResponseState":
        """Phase, timers, forced output, times and counts of every slot, and the owner of each loop, by reactor (one
        synchronisation)."""
        n = self.n_reactors
        st, rst = np.empty((respond.SLOTS, respond.NRS, n), dtype=np.float64), np.empty((respond.NRR, n), dtype=np.float64)
        self._program_call(_native.lib().wt_ensemble_respond_state, _native.dptr(st), _native.dptr(rst))
        return respond.ResponseState.from_block(st, rst)

    def response_params(self) -> np.ndarray:
        """The (4, 11, N) parameter block of the program in force, as :func:`response_block` built it."""
        blk = np.empty((respond.SLOTS, respond.NR, self.n_reactors), dtype=np.float64)
        self._program_call(_native.lib().wt_ensemble_respond_params, _native.dptr(blk))
        return blk

    def reset_responses(self) -> None:
        """Every slot idle again, latched ones included, counts and times zeroed.  The holding registers stay as they
        are, and the controllers resume from their own state."""
        self._program_call(_native.lib().wt_ensemble_respond_reset)

    def clear_responses(self) -> None:
        """Stop the response program; the holding registers stay as they are and the controllers resume."""
        self._program_call(_native.lib().wt_ensemble_respond_clear)

    # -- link programs at every PLC scan, before the injection programs on both paths, on the device (wt_lnk.hpp)
    def set_links(self, *links: "link.Link", seed: int = 0) -> None:
        """Run a link program of up to four :class:`Link` slots at every PLC scan, inside the step call: each slot keeps
        a ring of the last 64 samples of one reading or command and, inside its window, delivers a delayed sample, the
        last value that came through (with a timeout into a fail state) or a replayed tape.  Readings are linked after
        the wire program and before the injection program; commands after the decoding and before the injection
        program's command slots.  ``seed`` keys the draws of LOSS and jittered DELAY slots.  Replaces any program and
        restarts state and rings.  Needs :meth:`enable_plant_io` and at most 32 zones per reactor."""
        block = link.link_block(self.n_reactors, *links)
        self._program_call(_native.lib().wt_ensemble_link_set, _native.dptr(block), int(seed) & 0xFFFFFFFFFFFFFFFF)

    def link_state(self) -> "link.LinkState":
        """Counts, the last fresh delivery and the tape mark of every slot, by reactor (one synchronisation)."""
        st = np.empty((link.SLOTS, link.NLS, self.n_reactors), dtype=np.float64)
        self._program_call(_native.lib().wt_ensemble_link_state, _native.dptr(st))
        return link.LinkState.from_block(st)

    def link_params(self) -> np.ndarray:
        """The (4, 8, N) parameter block of the program in force, as :func:`link_block` built it."""
        blk = np.empty((link.SLOTS, link.NL, self.n_reactors), dtype=np.float64)
        self._program_call(_native.lib().wt_ensemble_link_params, _native.dptr(blk), None)
        return blk

    def link_ring(self):
        """The rings in recording order: ``(values, faults, n_rec)`` with values and faults (4, 64, N) -- entry k is the
        k-th oldest sample a ring still holds, NaN and 0 past the ``min(n_rec, 64)`` it has -- and n_rec (4, N)."""
        n = self.n_reactors
        v, f = np.empty((link.SLOTS, link.DEPTH, n), dtype=np.float64), np.empty((link.SLOTS, link.DEPTH, n), dtype=np.float64)
        c = np.empty((link.SLOTS, n), dtype=np.float64)
        self._program_call(_native.lib().wt_ensemble_link_ring, _native.dptr(v), _native.dptr(f), _native.dptr(c))
        return v, f, c

    def reset_links(self) -> None:
        """State and rings as :meth:`set_links` left them; the parameters and the seed stay."""
        self._program_call(_native.lib().wt_ensemble_link_reset)

    def clear_links(self) -> None:
        """Stop the link program; readings and commands pass as they are again."""
        self._program_call(_native.lib().wt_ensemble_link_clear)

    # -- injection programs at every PLC scan, on the device (wt_inj.hpp)
    def set_injections(self, *injections: "inject.Injection") -> None:
        """Run an injection program of up to four :class:`Injection` slots at every PLC scan, inside the step call:
        sensor targets spoof the reading the input image and the PI programs see (the instrument itself is
        untouched), command targets tamper with the decoded actuator command before it is validated (the holding
        registers keep what the master wrote).  Replaces any program and resets the state.  Needs
        :meth:`enable_plant_io` and at most 32 zones per reactor."""
        blk = inject.injection_block(self.n_reactors, *injections)
        self._program_call(_native.lib().wt_ensemble_inject_set, _native.dptr(blk))

    def injection_state(self) -> "inject.InjectionState":
        """Applications, first and last application time and the FREEZE value of every slot by reactor (one
        synchronisation)."""
        blk = np.empty((inject.SLOTS, inject.NIS, self.n_reactors), dtype=np.float64)
        self._program_call(_native.lib().wt_ensemble_inject_get, _native.dptr(blk))
        return inject.InjectionState.from_block(blk)

    def clear_injections(self) -> None:
        """Stop the injection program."""
        self._program_call(_native.lib().wt_ensemble_inject_clear)

    # -- alarm and interlock programs at every PLC scan, on the device (wt_alm.hpp)
    def set_alarms(self, *alarms: "alarm.Alarm") -> None:
        """Run an alarm program of up to four :class:`Alarm` slots at every PLC scan, inside the step call, after the
        PI programs: a HIGH or LOW limit on an image or field reading with deadband, on-delay and latch; an active
        slot with a trip action forces the acid or chlorine command to its trip value from the next scan on (the
        holding registers keep what the master wrote).  Replaces any program and resets the state.  Needs
        :meth:`enable_plant_io` and at most 32 zones per reactor."""
        blk = alarm.alarm_block(self.n_reactors, *alarms)
        self._program_call(_native.lib().wt_ensemble_alarm_set, _native.dptr(blk))

    def alarm_state(self) -> "alarm.AlarmState":
        """Slot and reactor state of the alarm program (one synchronisation)."""
        slots = np.empty((alarm.SLOTS, alarm.NAS, self.n_reactors), dtype=np.float64)
        reactors = np.empty((alarm.NAR, self.n_reactors), dtype=np.float64)
        self._program_call(_native.lib().wt_ensemble_alarm_get, _native.dptr(slots), _native.dptr(reactors))
        return alarm.AlarmState.from_block(slots, reactors)

    def alarm_words(self) -> np.ndarray:
        """(N,) uint16 alarm words: bits 0-3 active slots, 4-7 their conditions, 8 acid trip, 9 chlorine trip,
        12-14 first-out slot + 1."""
        w = np.empty(self.n_reactors, dtype=np.uint16)
        self._program_call(_native.lib().wt_ensemble_alarm_words, w.ctypes.data_as(C.POINTER(C.c_uint16)))
        return w

    def reset_alarms(self, reactors=None) -> None:
        """Acknowledge latched alarms: in the given reactors (indices or an (N,) bool mask; None: all), every latched
        slot whose condition has cleared becomes inactive; one whose condition still stands stays active."""
        if reactors is None:
            self._program_call(_native.lib().wt_ensemble_alarm_reset, None)
            return
        r = np.asarray(reactors)
        mask = np.zeros(self.n_reactors, dtype=np.uint8)
        if r.dtype == bool:
            if r.shape != (self.n_reactors,):
                raise ValueError(f"a reactor mask must have shape ({self.n_reactors},)")
            mask[r] = 1
        else:
            mask[r.astype(np.int64)] = 1
        self._program_call(_native.lib().wt_ensemble_alarm_reset, mask.ctypes.data_as(C.POINTER(C.c_uint8)))

    def clear_alarms(self) -> None:
        """Stop the alarm program (trips in force end with it)."""
        self._program_call(_native.lib().wt_ensemble_alarm_clear)

    # -- actuator programs at every PLC scan, on the device (wt_act.hpp)
    def set_actuators(self, *actuators: "actuator.Actuator") -> None:
        """Put a final element with dead time, lag, rate limit, backlash and a fault window on up to three channels
        (one :class:`Actuator` each: "acid", "chlorine", "inlet").  At every PLC scan, inside the step call and
        downstream of the whole command path (PI outputs, command tampering, interlock trips), the element's position
        becomes the boundary row the next step integrates under.  Every element starts at its row in force.  Replaces
        any program.  Needs :meth:`enable_plant_io` and at most 32 zones per reactor."""
        blk = actuator.actuator_block(self.n_reactors, *actuators)
        self._program_call(_native.lib().wt_ensemble_actuator_set, _native.dptr(blk))

    def actuator_state(self) -> "actuator.ActuatorState":
        """Channel state, demand queues and t_prev of the actuator program (one synchronisation)."""
        N = self.n_reactors
        st = np.empty((len(actuator.CHANNELS), actuator.NVS, N), dtype=np.float64)
        q = np.empty((len(actuator.CHANNELS), actuator.MAX_DELAY, N), dtype=np.float64)
        tp = np.empty(N, dtype=np.float64)
        self._program_call(_native.lib().wt_ensemble_actuator_get, _native.dptr(st), _native.dptr(q), _native.dptr(tp))
        return actuator.ActuatorState.from_block(st, q, tp)

    def clear_actuators(self) -> None:
        """Stop the actuator program: from the next scan on the commands reach the plant at once."""
        self._program_call(_native.lib().wt_ensemble_actuator_clear)

    # -- disturbance programs after every outer step, on the device (wt_dst.hpp)
    def set_disturbances(self, *disturbances: "disturb.Disturbance", seed: int = 0xD157, reactor_base: int = 0,
                         history: int = 0) -> None:
        """Move up to four boundary rows per reactor on their own (one :class:`Disturbance` per slot: steps, ramps,
        sines, Ornstein-Uhlenbeck wandering) on the rows the command path does not own.  After every outer step,
        inside the step call, the rows become ``clamp(base + offsets)`` for the reactor's next step; the base is the
        boundary in force now (a later :meth:`set_boundary` replaces it).  ``seed`` and ``reactor_base`` key the OU
        draws (shards of one ensemble pass their first global reactor); ``history`` > 0 keeps that many offsets per
        reactor.  Replaces any program.  Not with ``boundary_schedule``; at most 32 zones per reactor."""
        blk = disturb.disturbance_block(self.n_reactors, *disturbances)
        self._program_call(_native.lib().wt_ensemble_disturb_set, _native.dptr(blk),
                           C.c_uint64(int(seed) & 0xFFFFFFFFFFFFFFFF), int(reactor_base), int(history))

    def disturbance_state(self) -> "disturb.DisturbanceState":
        """Slot state, base block and t_prev of the disturbance program (one synchronisation)."""
        N = self.n_reactors
        st = np.empty((disturb.SLOTS, disturb.NDS, N), dtype=np.float64)
        base = np.empty((len(params.BOUNDARY_FIELDS), N), dtype=np.float64)
        tp = np.empty(N, dtype=np.float64)
        self._program_call(_native.lib().wt_ensemble_disturb_get, _native.dptr(st), _native.dptr(base), _native.dptr(tp))
        return disturb.DisturbanceState.from_block(st, base, tp)

    def disturbance_history(self):
        """(offsets (H, 4, N), entries filled per reactor (N,)): entry k holds the offsets the reactor's k-th step
        after :meth:`set_disturbances` integrated under (entry 0: those made at set time)."""
        N, H = self.n_reactors, self.info(_native.WT_INFO_DISTURB_HISTORY)
        off = np.empty((H, disturb.SLOTS, N), dtype=np.float64)
        filled = np.empty(N, dtype=np.int32)
        self._program_call(_native.lib().wt_ensemble_disturb_history, _native.dptr(off) if H else None,
                           filled.ctypes.data_as(C.POINTER(C.c_int32)))
        return off, filled

    def clear_disturbances(self) -> None:
        """Stop the disturbance program: the targeted rows go back to the base."""
        self._program_call(_native.lib().wt_ensemble_disturb_clear)

    # -- anomaly detector programs at every PLC scan, on the device (wt_det.hpp)
    # -- the train program: stages feed their downstream after every outer step, on the device (wt_trn.hpp)
    def set_trains(self, length: int, linked=True, rows=train.ALL_ROWS) -> None:
        """Read the ensemble as ``N / length`` treatment trains of ``length`` stages: reactor r is stage ``r % length``
        of train ``r // length``.  After every outer step its upstream took, a linked stage gets the upstream's outlet
        zone in its boundary rows inlet_pH / inlet_chlorine / inlet_temperature (``rows``: names, or masks 1 | 2 | 4),
        the boundary of its next outer step -- the bits of a host loop of one-step calls that copies outlets into
        ``set_boundary`` between them.  ``linked`` and ``rows`` take a scalar or an (N,) array; first stages are never
        linked.  Flows are not carried.  The stages of a train share a wavefront: ``2 <= length <= 64 // n_zones`` and
        ``N % length == 0``.  A shard of a sharded ensemble must hold whole trains (``shard_bounds`` does not know
        about trains: choose sizes that are multiples of ``length``).  Replaces any program; :meth:`clear_trains`."""
        blk = train.train_block(self.n_reactors, self.n_zones, length, linked, rows)
        self._program_call(_native.lib().wt_ensemble_train_set, int(length), _native.dptr(blk))

    def train_state(self) -> "train.TrainState":
        """Feeds counted per reactor, the upstream's time at the last one, the train length and the reactors per
        wavefront in force (one synchronisation)."""
        st = np.empty((train.NTRS, self.n_reactors), dtype=np.float64)
        length, per = C.c_int(0), C.c_int(0)
        self._program_call(_native.lib().wt_ensemble_train_get, C.byref(length), C.byref(per), _native.dptr(st))
        return train.TrainState.from_block(st, length.value, per.value)

    def clear_trains(self) -> None:
        """Stop the train program: the linked rows go back to what ``set_boundary`` last gave, the handle to the
        wavefront packing it had before."""
        self._program_call(_native.lib().wt_ensemble_train_clear)

    # -- the pipe program: dead time between the stages of a train, on the device (wt_trn.hpp)
    def set_pipes(self, delay) -> None:
        """Give the links of the train program a dead time of ``delay`` whole outer steps (a scalar or an (N,) array,
        0..4095; ``train.pipe_delay`` converts seconds): the upstream's outlet reaches the downstream's rows through a
        FIFO of that many samples, which starts full of the water the upstream holds now -- the bits of the train
        program's host loop with a FIFO per link.  First stages and stages that are not linked get 0.  A link with
        delay 0 behaves as it does without pipes.  Needs a train program; replaces any pipe program;
        :meth:`clear_pipes`.  ``set_trains`` and ``clear_trains`` clear the pipes."""
        par = np.empty((train.NTR, self.n_reactors), dtype=np.float64)
        self._program_call(_native.lib().wt_ensemble_train_params, _native.dptr(par))   # refused without a train program
        d = train.pipe_block(self.n_reactors, self.info(_native.WT_INFO_TRAIN_LENGTH), delay, par[0])
        self._program_call(_native.lib().wt_ensemble_pipe_set, _native.dptr(d))

    def pipe_state(self) -> "train.PipeState":
        """Feeds through each line, the time stamp of the sample last delivered, the delays and the ring slots (one
        synchronisation)."""
        N = self.n_reactors
        st, d, slots = np.empty((train.NPS, N), dtype=np.float64), np.empty(N, dtype=np.float64), C.c_int(0)
        self._program_call(_native.lib().wt_ensemble_pipe_get, C.byref(slots), _native.dptr(d), _native.dptr(st), None)
        return train.PipeState(np.array(st[0]), np.array(st[1]), d.astype(np.int64), slots.value)

    def pipe_lines(self) -> np.ndarray:
        """(Dmax, 4, N): the samples in flight in every line, oldest first -- pH, chlorine, temperature of the
        upstream's outlet zone and the upstream's time when they were taken (NaN for the initial fill) -- padded with
        NaN beyond a line's own delay.  Dmax is the largest delay of the program."""
        slots = C.c_int(0)
        self._program_call(_native.lib().wt_ensemble_pipe_get, C.byref(slots), None, None, None)
        lines = np.empty((max(slots.value - 1, 0), len(train.PIPE_SAMPLE), self.n_reactors), dtype=np.float64)
        if lines.size:
            self._program_call(_native.lib().wt_ensemble_pipe_get, None, None, None, _native.dptr(lines))
        return lines

    def clear_pipes(self) -> None:
        """Stop the pipe program: the linked rows stay as they are, the next feed is undelayed."""
        self._program_call(_native.lib().wt_ensemble_pipe_clear)

    # -- the wire program: a stage's PLC inputs from another stage's instruments, on the device (wt_wir.hpp)
    def set_wires(self, *wires: "wire.Wire") -> None:
        """Wire input slots of stages to instruments of other stages of the same train (:class:`Wire`): at every PLC
        scan, before everything else in the scan, a wired slot of a reactor's controller-side copy of the readings gets
        the source instrument's reading and fault code of this outer step, so the injection program, the input image,
        the PI loops, the IMAGE slots of alarms and detectors and the trend recorder's image tags see the remote value
        -- the bits of a host master that routes ``sensor_readings()`` between calls of one scan interval.  FIELD
        slots, ``sensor_readings()`` and the sensor history stay the reactor's own instrument; a source that did not
        take the step reads NaN with fault 1.  Needs a train program and plant I/O; replaces any wire program;
        :meth:`clear_wires`.  ``set_trains`` and ``clear_trains`` clear the wires."""
        if not self.info(_native.WT_INFO_TRAIN):
            self._program_call(_native.lib().wt_ensemble_wire_set, None)    # the library's refusal
        blk = wire.wire_block(self.n_reactors, self.info(_native.WT_INFO_TRAIN_LENGTH), *wires)
        self._program_call(_native.lib().wt_ensemble_wire_set, _native.dptr(blk))

    def wire_state(self) -> "wire.WireState":
        """Per reactor and input slot: the scans that delivered a source's reading and those that found the source
        stopped (one synchronisation)."""
        st = np.empty((wire.NSENS, wire.NWS, self.n_reactors), dtype=np.float64)
        self._program_call(_native.lib().wt_ensemble_wire_get, None, _native.dptr(st))
        return wire.WireState.from_block(st)

    def wire_params(self) -> np.ndarray:
        """The (7, 2, N) block of the wire program in force: per slot the source stage (-1: own instrument) and the
        source sensor."""
        blk = np.empty((wire.NSENS, wire.NW, self.n_reactors), dtype=np.float64)
        self._program_call(_native.lib().wt_ensemble_wire_get, _native.dptr(blk), None)
        return blk

    def clear_wires(self) -> None:
        """Stop the wire program: every slot is the reactor's own instrument again."""
        self._program_call(_native.lib().wt_ensemble_wire_clear)

    # -- the junction program: flow-weighted merges and splits in a train, on the device (wt_trn.hpp)
    def set_junctions(self, *junctions: "junction.Junction") -> None:
        """Feed stages of the train program from up to four other stages of their train (:class:`Junction`): after
        every outer step all its sources took, a junction's inlet rows get the blend of the sources' outlet zones
        weighted by ``share * the source's inlet flow`` -- chlorine and temperature as flow-weighted means, pH through
        H+ -- and with ``carry`` its inlet flow becomes the summed flow: the bits (a blended pH: within 2e-14) of the
        train program's host loop with that blend between the calls.  Needs a train program; set it before the pipes;
        replaces any junction program; :meth:`clear_junctions`.  ``set_trains`` and ``clear_trains`` clear the
        junctions.  A carried flow excludes plant I/O."""
        if not self.info(_native.WT_INFO_TRAIN):
            self._program_call(_native.lib().wt_ensemble_junction_set, None, None)    # the library's refusal
        par = np.empty((train.NTR, self.n_reactors), dtype=np.float64)
        self._program_call(_native.lib().wt_ensemble_train_params, _native.dptr(par))
        blk, carry = junction.junction_block(self.n_reactors, self.info(_native.WT_INFO_TRAIN_LENGTH), par[0], *junctions)
        self._program_call(_native.lib().wt_ensemble_junction_set, _native.dptr(blk), _native.dptr(carry))

    def junction_state(self) -> "junction.JunctionState":
        """Per reactor: the feeds a junction got inside step calls, the outer steps it was held, the summed flow of the
        last feed (one synchronisation)."""
        st = np.empty((junction.NJS, self.n_reactors), dtype=np.float64)
        self._program_call(_native.lib().wt_ensemble_junction_get, _native.dptr(st))
        return junction.JunctionState.from_block(st)

    def junction_params(self):
        """The (4, 2, N) block of the junction program in force -- per slot the source stage (-1: unused) and its share
        -- and the (N,) carry flags."""
        blk = np.empty((junction.JCT_SLOTS, junction.NJ, self.n_reactors), dtype=np.float64)
        carry = np.empty(self.n_reactors, dtype=np.float64)
        self._program_call(_native.lib().wt_ensemble_junction_params, _native.dptr(blk), _native.dptr(carry))
        return blk, carry

    def clear_junctions(self) -> None:
        """Stop the junction program: the bases go back into the linked rows and the carriers' inlet flows, then every
        link is fed by its upstream as the train program does."""
        self._program_call(_native.lib().wt_ensemble_junction_clear)

    def set_detectors(self, *detectors: "detect.Detector", attack=None) -> None:
        """Run a detector program of up to four :class:`Detector` slots at every PLC scan, inside the step call, last in
        the scan: each slot keeps a CUSUM, EWMA or flat-line statistic of one reading's residual, raises its alarm
        above the slot's limit and counts the scans against the ground-truth window ``attack`` = (start, end), scalars
        or (N,) arrays of loop times (default: never attacked; ``inject.attack_window`` gives the window of an
        injection block).  The program is passive: the plant and the other programs keep their bits.  Replaces any
        earlier program and resets its state.  Needs plant I/O and at most 32 zones."""
        blk = detect.detector_block(self.n_reactors, *detectors)
        lab = detect.label_block(self.n_reactors, attack)
        self._program_call(_native.lib().wt_ensemble_detect_set, _native.dptr(blk), _native.dptr(lab))

    def detector_state(self) -> "detect.DetectorState":
        """Slot state, t_prev and label of the detector program (two downloads, each synchronises)."""
        st = np.empty((detect.SLOTS, detect.NKS, self.n_reactors), dtype=np.float64)
        tp = np.empty(self.n_reactors, dtype=np.float64)
        lab = np.empty((detect.NKR, self.n_reactors), dtype=np.float64)
        self._program_call(_native.lib().wt_ensemble_detect_get, _native.dptr(st), _native.dptr(tp))
        self._program_call(_native.lib().wt_ensemble_detect_labels, _native.dptr(lab))
        return detect.DetectorState.from_block(st, tp, lab)

    def reset_detectors(self) -> None:
        """Statistics, alarms and counts back to their values at :meth:`set_detectors`, at the current loop time; the
        parameters and the label stay (detection after a warm-up)."""
        self._program_call(_native.lib().wt_ensemble_detect_reset)

    def clear_detectors(self) -> None:
        """Stop the detector program and free its buffers."""
        self._program_call(_native.lib().wt_ensemble_detect_clear)

    # -- trend recorder programs at every PLC scan, on the device (wt_trd.hpp)
    def set_trends(self, *trends: "trend.Trend", capacity: int, wrap: bool = False) -> None:
        """Record up to eight :class:`Trend` slots at every PLC scan, inside the step call, last in the scan: each slot
        appends (loop time, value) of one reading, fault code, command or entry of another program's state to a store
        of ``capacity`` samples per slot and reactor.  A full store drops further samples (``trend_state().n_dropped``
        counts them) or, with ``wrap``, overwrites the oldest.  The program is passive: the plant and the other
        programs keep their bits.  Replaces any earlier program, its state and its data.  Needs plant I/O and at most
        32 zones."""
        blk = trend.trend_block(self.n_reactors, *trends)
        self._program_call(_native.lib().wt_ensemble_trend_set, _native.dptr(blk), int(capacity), int(bool(wrap)))

    def trend_state(self) -> "trend.TrendState":
        """Slot state of the trend program (one synchronisation)."""
        st = np.empty((trend.SLOTS, trend.NTS, self.n_reactors), dtype=np.float64)
        self._program_call(_native.lib().wt_ensemble_trend_get, _native.dptr(st))
        return trend.TrendState.from_block(st)

    def trend_data(self) -> "trend.TrendData":
        """The recorded series, oldest sample first (a wrapped store is unwrapped), NaN past the samples held."""
        st = np.empty((trend.SLOTS, trend.NTS, self.n_reactors), dtype=np.float64)
        self._program_call(_native.lib().wt_ensemble_trend_get, _native.dptr(st))
        cap = self.info(_native.WT_INFO_TREND_CAPACITY)
        t = np.empty((trend.SLOTS, cap, self.n_reactors), dtype=np.float64)
        x = np.empty_like(t)
        self._program_call(_native.lib().wt_ensemble_trend_data, _native.dptr(t), _native.dptr(x))
        count = np.minimum(st[:, trend.STATE_ROWS.index("n_recorded")], cap).astype(np.int64)
        return trend.TrendData(t, x, count)

    def reset_trends(self) -> None:
        """Slot state and data back to their values at :meth:`set_trends`; the slots, the capacity and ``wrap`` stay
        (recording after a warm-up)."""
        self._program_call(_native.lib().wt_ensemble_trend_reset)

    def clear_trends(self) -> None:
        """Stop the trend program and free its buffers."""
        self._program_call(_native.lib().wt_ensemble_trend_clear)

    # -- score programs after every outer step, on the device (wt_scr.hpp)
    def set_scores(self, *scores: "score.Score", curve: int = 0, bins: int = 0, fan_range=None) -> None:
        """Judge the true reactor state after every outer step, inside the step call: one :class:`Score` per slot (up
        to four) accumulates per reactor the time below and above its band, the deficit and excess areas, the
        exposure integral and the excursion runs (:meth:`score_state`).  ``curve`` > 0 keeps that many outer steps of
        the ensemble curve (:meth:`score_curve`): reactors scored, below and above per step and slot.  ``bins`` in
        1..32 adds a histogram of the scored value per step between ``fan_range`` = (lo, hi), scalars or one pair of
        values per slot.  Nothing in the plant changes.  Replaces any program; at most 32 zones per reactor."""
        blk = score.score_block(self.n_reactors, *scores)
        cap, B = int(curve), int(bins)
        lo = hi = None
        if B > 0:
            if fan_range is None:
                raise ValueError("bins > 0 needs fan_range=(lo, hi)")
            try:
                lo = np.ascontiguousarray(np.broadcast_to(np.asarray(fan_range[0], dtype=np.float64), (score.SLOTS,)))
                hi = np.ascontiguousarray(np.broadcast_to(np.asarray(fan_range[1], dtype=np.float64), (score.SLOTS,)))
            except ValueError:
                raise ValueError("fan_range: expected (lo, hi), each a scalar or one value per slot (4,)") from None
        self._program_call(_native.lib().wt_ensemble_score_set, _native.dptr(blk), cap, B,
                           None if lo is None else _native.dptr(lo), None if hi is None else _native.dptr(hi))

    def score_state(self) -> "score.ScoreState":
        """The per-reactor accumulators of the score program (one synchronisation)."""
        st = np.empty((score.SLOTS, score.NSS, self.n_reactors), dtype=np.float64)
        tp = np.empty(self.n_reactors, dtype=np.float64)
        self._program_call(_native.lib().wt_ensemble_score_get, _native.dptr(st), _native.dptr(tp))
        return score.ScoreState.from_block(st, tp)

    def score_curve(self) -> "score.ScoreCurve":
        """The ensemble curve of the score program: the outer steps taken since :meth:`set_scores` or
        :meth:`reset_scores`, up to the curve's capacity (one synchronisation)."""
        cap, B = self.info(_native.WT_INFO_SCORE_CURVE), self.info(_native.WT_INFO_SCORE_BINS)
        counts = np.zeros((cap, score.SLOTS, 3), dtype=np.int32)
        fan = np.zeros((cap, score.SLOTS, B + 2), dtype=np.int32) if B > 0 else None
        i32p, k = C.POINTER(C.c_int32), C.c_int(0)
        self._program_call(_native.lib().wt_ensemble_score_curve, counts.ctypes.data_as(i32p) if cap else None,
                           fan.ctypes.data_as(i32p) if fan is not None else None, C.byref(k))
        K, edges = k.value, None
        if B > 0:
            lo, hi = np.empty(score.SLOTS), np.empty(score.SLOTS)
            self._program_call(_native.lib().wt_ensemble_score_fan_range, _native.dptr(lo), _native.dptr(hi))
            edges = score.fan_edges(lo, hi, B)
        return score.ScoreCurve(counts[:K, :, 0].copy(), counts[:K, :, 1].copy(), counts[:K, :, 2].copy(),
                                None if fan is None else fan[:K].copy(), edges)

    def reset_scores(self) -> None:
        """Accumulators and curve back to their values at :meth:`set_scores`, the parameters kept: scoring starts over
        at the current time (after a warm-up)."""
        self._program_call(_native.lib().wt_ensemble_score_reset)

    def clear_scores(self) -> None:
        """Stop the score program and free its buffers."""
        self._program_call(_native.lib().wt_ensemble_score_clear)

    # -- diagnostics (NEXT-4)
    # -- checkpoint, copy and rewind of everything the handle holds
    def checkpoint(self) -> bytes:
        """Everything that decides the next bits of the run -- state, sensors, register images, records, every
        program with its state and stores, trains, pipes, wires, placement and schedule -- as one blob
        (include/wtphys.h describes it).  Developer instrumentation is not part of it."""
        n = C.c_int64(0)
        _native.check(_native.lib().wt_ensemble_checkpoint_size(self._h, C.byref(n)))
        buf = np.empty(n.value, dtype=np.uint8)
        self._program_call(_native.lib().wt_ensemble_checkpoint_save, buf.ctypes.data_as(C.c_void_p), n.value)
        return buf.tobytes()

    def restore(self, blob) -> None:
        """Back to a :meth:`checkpoint` of an ensemble with the same reactors: the blob's programs and capacities
        replace whatever is set here.  A refused blob (``ValueError``) changes nothing."""
        buf = np.frombuffer(bytes(blob), dtype=np.uint8)
        self._program_call(_native.lib().wt_ensemble_checkpoint_load, buf.ctypes.data_as(C.c_void_p), buf.size)

    def clone(self) -> "ReactorEnsemble":
        """A second ensemble on the same device that continues exactly as this one would; the two share nothing."""
        other = ReactorEnsemble(self.columns, n_zones=self.n_zones, device=self.device, validate=False)
        try:
            other._program_call(_native.lib().wt_ensemble_copy, self._h)
        except Exception:
            other.close()
            raise
        return other

    def mark(self) -> None:
        """Keep a checkpoint in device memory inside the ensemble (replaces an earlier mark)."""
        self._program_call(_native.lib().wt_ensemble_mark)

    def rewind(self) -> None:
        """Back to the :meth:`mark`, any number of times: programs and capacities set since go, the marked ones return."""
        self._program_call(_native.lib().wt_ensemble_rewind)

    def unmark(self) -> None:
        self._program_call(_native.lib().wt_ensemble_unmark)

    _FILE_COLUMN = "column_"

    def save(self, path) -> None:
        """One ``.npz`` file (no pickle): the reactor columns, ``n_zones`` and the :meth:`checkpoint` blob."""
        entries = {self._FILE_COLUMN + k: np.asarray(v) for k, v in self.columns.items()}
        np.savez(path, n_zones=np.int64(self.n_zones), checkpoint=np.frombuffer(self.checkpoint(), dtype=np.uint8), **entries)

    @classmethod
    def load(cls, path, device: int = 0) -> "ReactorEnsemble":
        """The ensemble a :meth:`save` file describes, on ``device``.  A file without the expected entries is a
        ``ValueError`` that names the entry."""
        with np.load(path, allow_pickle=False) as f:
            for name in ("n_zones", "checkpoint"):
                if name not in f.files:
                    raise ValueError(f"{path}: no '{name}' entry: not a ReactorEnsemble.save file")
            n_zones, blob = f["n_zones"], f["checkpoint"]
            cols = {k[len(cls._FILE_COLUMN):]: f[k] for k in f.files if k.startswith(cls._FILE_COLUMN)}
        if n_zones.shape != () or n_zones.dtype.kind != "i":
            raise ValueError(f"{path}: 'n_zones' must be one integer")
        if blob.ndim != 1 or blob.dtype != np.uint8:
            raise ValueError(f"{path}: 'checkpoint' must be a one-dimensional uint8 array")
        missing = [name for name in _CFG_FIELDS if name != "n_zones" and name not in cols]
        if missing:
            raise ValueError(f"{path}: no '{cls._FILE_COLUMN}{missing[0]}' entry: not a ReactorEnsemble.save file")
        if len({v.shape for v in cols.values()}) != 1 or next(iter(cols.values())).ndim != 1:
            raise ValueError(f"{path}: the '{cls._FILE_COLUMN}*' entries must be one-dimensional and of one length")
        ens = cls(cols, n_zones=int(n_zones), device=device, validate=False)
        try:
            ens.restore(blob.tobytes())
        except Exception:
            ens.close()
            raise
        return ens

    DIAGNOSTIC_FIELDS = ("total_chlorine_mg", "total_H_mol", "total_OH_mol", "charge_balance_mol", "thermal_energy_kJ",
                         "pH_CV", "pH_segregation", "chlorine_CV", "chlorine_segregation", "thermocline_depth_m") + tuple(
        f"{p}_{k}" for p in ("pH", "chlorine", "temperature")
        for k in ("mean_value", "std_value", "max_value", "min_value", "range", "max_gradient", "mean_gradient", "gradient_location"))

    def diagnostics(self, as_dict: bool = True):
        """``validate_conservation`` + ``calculate_mixing_quality`` (pH, chlorine) + ``identify_thermocline``
        (NaN = None) + ``calculate_spatial_gradients`` (pH, chlorine, temperature) of every reactor,
        reduced on the device: dict name -> (N,) array, or the raw (34, N) block."""
        out = np.empty((len(self.DIAGNOSTIC_FIELDS), self.n_reactors), dtype=np.float64)
        _native.check(_native.lib().wt_ensemble_diagnostics(self._h, _native.dptr(out)))
        return dict(zip(self.DIAGNOSTIC_FIELDS, out)) if as_dict else out

    def wave_diag(self) -> Optional[np.ndarray]:
        """Per-wavefront diagnostics of the last launch, (n_waves, 8) int64:
        loop trips, Newton trips, shader clocks, 100 MHz wall ticks, factorize / num_jac /
        deferred-f block executions, spare.  The first
        call only switches recording on and returns None."""
        nw = C.c_int64(0)
        L = _native.lib()
        on = self.info(_native.WT_INFO_WAVE_DIAG)
        _native.check(L.wt_ensemble_wave_diag(self._h, None, 0, C.byref(nw)))     # not allocated: switches them on
        if not on:
            return None
        out = np.zeros((nw.value, L.wt_wave_diag_slots()), dtype=np.int64)
        _native.check(L.wt_ensemble_wave_diag(self._h, out.ctypes.data_as(C.POINTER(C.c_int64)), nw.value, C.byref(nw)))
        return out

    def export_state_device(self, device_ptr: int) -> None:
        """Async device-to-device copy of [pH, Cl, T] (3, N, n) into caller device memory."""
        _native.check(_native.lib().wt_ensemble_export_state_device(self._h, C.c_void_p(device_ptr)))

    def set_stream(self, hip_stream: int) -> None:
        _native.check(_native.lib().wt_ensemble_set_stream(self._h, C.c_void_p(hip_stream)))

    def timer_start(self) -> None:
        _native.check(_native.lib().wt_ensemble_timer_start(self._h))

    def timer_stop(self) -> float:
        ms = C.c_float(0.0)
        _native.check(_native.lib().wt_ensemble_timer_stop(self._h, C.byref(ms)))
        return float(ms.value)


def _validate_columns(cols: Dict[str, np.ndarray]) -> None:
    """Vectorised ReactorConfiguration.validate (reactor.py:91-110)."""
    calc = np.pi * (cols["diameter"] / 2) ** 2 * cols["height"] * 1000
    err = np.abs(calc - cols["volume"]) / cols["volume"]
    if np.any(err > 0.01):
        r = int(np.argmax(err > 0.01))
        raise ValueError(f"Volume mismatch: specified {cols['volume'][r]}L, calculated {calc[r]:.1f}L "
                         f"from geometry. Error: {err[r]*100:.1f}%")
    assert np.all((0 < cols["volume"]) & (cols["volume"] < 1e6)), "Volume out of range"
    assert np.all((0 <= cols["flow_rate"]) & (cols["flow_rate"] < 1e5)), "Flow rate out of range (use 0 for batch mode)"
    assert np.all((0 <= cols["initial_pH"]) & (cols["initial_pH"] <= 14)), "pH out of range"
    assert np.all((0 <= cols["initial_chlorine"]) & (cols["initial_chlorine"] <= 10)), "Chlorine out of range"
    assert np.all((0 <= cols["temperature"]) & (cols["temperature"] <= 40)), "Temperature out of typical range"


# --------------------------------------------------------------------------- single-reactor drop-in
class IntegratedCSTR:
    """Drop-in for the reference class of the same name (reactor.py:189-611),
    backed by a one-reactor ensemble on the GPU."""

    #: Radau step attempts per outer step before the solve is given up with a warning.  scipy's solve_ivp has no such
    #: limit, but the step kernel cannot be cancelled: where the solution slides along the 8 degC density jump the
    #: reference needs millions of internal steps (hours), and an unbounded device solve looks like a hang from the
    #: host.  Ten million attempts is far beyond anything a finite reference run was seen to need; pass
    #: ``step_limit=0`` for the reference's unbounded behaviour.
    DEFAULT_STEP_LIMIT = 10_000_000

    def __init__(self, config: ReactorConfiguration, device: int = 0, step_limit: Optional[int] = None):
        config.validate()
        self.config = config
        self._ens = ReactorEnsemble([config], device=device, validate=False)
        self._ens.set_step_limit(self.DEFAULT_STEP_LIMIT if step_limit is None else int(step_limit))
        self._last = None                # (pH, chlorine, temperature, time) as the device holds them, when known
        n = config.n_zones
        self._initialize_physics_modules()
        self.state = ReactorState(
            pH=np.full(n, config.initial_pH),
            chlorine=np.full(n, config.initial_chlorine),
            temperature=np.full(n, config.temperature),
            flow_rate=config.flow_rate)
        # same log line as reactor.py:224-227 (and, as there, a TypeError when
        # flow_rate == 0 because residence_time is None)
        logger.info(f"Reactor initialized: {config.n_zones} zones, "
                    f"V={config.volume}L, τ={self.transport.residence_time:.1f}min")

    def _initialize_physics_modules(self) -> None:
        """The sub-objects the reference builds (reactor.py:229-270): host-side holders of the reactor's init-time
        constants and scalar diagnostics; the step itself runs on the device from ``self._ens.constants``."""
        from .chemistry import AqueousChemistry, BufferSystem
        from .physics import (FlowParameters, GeometryParameters, SpatialModel, StratificationParameters,
                              TemperatureDependentKinetics, TransportModel)
        c = self.config
        self.thermo = TemperatureDependentKinetics()
        self.buffer = BufferSystem(alkalinity=c.alkalinity, total_carbonate=c.total_carbonate, temperature=c.temperature)
        self.chemistry = AqueousChemistry(self.buffer, device=self._ens.device)
        geometry = GeometryParameters(volume=c.volume, height=c.height, diameter=c.diameter, n_zones=c.n_zones)
        flow = FlowParameters(flow_rate=c.flow_rate, turbulent_intensity=c.turbulent_intensity,
                              recirculation_ratio=c.recirculation_ratio, impeller_speed=c.impeller_speed,
                              impeller_diameter=c.impeller_diameter, power_number=c.power_number)
        self.transport = TransportModel(geometry, flow, c.temperature)
        self.spatial = SpatialModel(n_zones=c.n_zones, height=c.height, stratification_params=StratificationParameters(
            enable_thermal_stratification=c.enable_thermal_stratification))

    def derivatives(self, t: float, y: np.ndarray, boundary: BoundaryConditions) -> np.ndarray:
        n = self.config.n_zones
        y = np.asarray(y, dtype=np.float64)
        self._ens.set_boundary(boundary)
        dpH, dCl, dT, fl = self._ens.derivatives(y[None, 0:n], y[None, n:2 * n], y[None, 2 * n:3 * n])
        if fl[0] & ST_T_RANGE:
            T = y[2 * n:3 * n]
            bad = T[(T < 0) | (T > 100)]
            raise ValueError(_T_RANGE_TEXT.format(value=bad[0] if bad.size else "nan"))
        return np.concatenate([dpH[0], dCl[0], dT[0]])

    def step(self, dt: float, boundary: BoundaryConditions) -> ReactorState:
        """Advance by ``dt`` seconds under ``boundary`` (reactor.py:450-509)."""
        ens = self._ens
        s = self.state
        # honour host-side edits of self.state between steps (reactor.py:467-469): upload unless the state is
        # exactly what the device left there
        last = self._last
        if not (last is not None and s.time == last[3] and np.array_equal(s.pH, last[0], equal_nan=True)
                and np.array_equal(s.chlorine, last[1], equal_nan=True) and np.array_equal(s.temperature, last[2], equal_nan=True)):
            ens.set_state(np.asarray(s.pH, dtype=np.float64)[None, :], np.asarray(s.chlorine, dtype=np.float64)[None, :],
                          np.asarray(s.temperature, dtype=np.float64)[None, :], np.array([s.time], dtype=np.float64))
        self._last = None
        es = ens.step(dt, boundary, n_steps=1)
        flags = int(es.status[0])
        if flags & ST_NONFINITE and float(es.time[0]) == float(s.time):
            raise ValueError(_NONFINITE_TEXT)         # solve_ivp refused y0: self.state untouched
        if flags & ST_T_RANGE:
            raise ValueError(_T_RANGE_TEXT.format(value=np.float64(ens.bad_temperature()[0])))
        if flags & ST_STEP_LIMIT:
            logger.warning("ODE solver stopped: internal step-attempt limit reached (see set_step_limit)")
        elif flags & ST_SOLVER_FAILED:
            logger.warning(_SOLVER_FAILED_TEXT)
        pre = None
        s.pH, s.chlorine, s.temperature = es.pH[0].copy(), es.chlorine[0].copy(), es.temperature[0].copy()
        s.time = float(es.time[0])
        s.flow_rate = float(es.flow_rate[0])
        s.H_concentration = es.H_concentration[0].copy()
        s.density = es.density[0].copy()
        if flags & ST_T_RANGE_POST:
            raise ValueError(_T_RANGE_TEXT.format(value=np.float64(ens.bad_temperature()[0])))
        s.chlorine_decay_rate = es.chlorine_decay_rate[0].copy()
        if flags & ST_CLAMP_PH:
            logger.error("pH out of bounds: clipped to [0, 14]")
        if flags & ST_CLAMP_CL:
            logger.warning("Negative chlorine detected: clipped to 0")
        if flags & ST_CLAMP_T:
            logger.error("Temperature out of bounds: clipped to [0, 100]")
        if flags == 0:
            self._last = (s.pH.copy(), s.chlorine.copy(), s.temperature.copy(), s.time)
        return s

    def get_state_at_location(self, zone_idx: int, parameter: str) -> float:
        if zone_idx < 0 or zone_idx >= self.config.n_zones:
            raise ValueError(f"Zone index {zone_idx} out of range [0, {self.config.n_zones-1}]")
        table = {"pH": self.state.pH, "chlorine": self.state.chlorine,
                 "temperature": self.state.temperature, "density": self.state.density}
        if parameter not in table:
            raise ValueError(f"Unknown parameter: {parameter}")
        return table[parameter][zone_idx]

    def _device_diagnostics(self) -> Dict[str, np.ndarray]:
        s = self.state
        self._ens.set_state(np.asarray(s.pH, dtype=np.float64)[None, :], np.asarray(s.chlorine, dtype=np.float64)[None, :],
                            np.asarray(s.temperature, dtype=np.float64)[None, :], np.array([s.time], dtype=np.float64))
        return self._ens.diagnostics()

    def validate_conservation(self) -> Dict[str, float]:
        """Mass / charge / energy inventory of ``self.state`` (reactor.py:570-611), reduced on the device."""
        d = self._device_diagnostics()
        out = {k: float(d[k][0]) for k in ("total_chlorine_mg", "total_H_mol", "total_OH_mol", "charge_balance_mol", "thermal_energy_kJ")}
        out["zones"] = self.config.n_zones
        out["timestamp"] = self.state.time
        return out

    def mixing_quality(self) -> Dict[str, float]:
        """(CV, segregation index) of pH and chlorine as ``print_diagnostics`` reports them
        (transport.py:338-384 via reactor.py:638-639)."""
        d = self._device_diagnostics()
        return {k: float(d[k][0]) for k in ("pH_CV", "pH_segregation", "chlorine_CV", "chlorine_segregation")}


    def print_diagnostics(self) -> None:
        """The report of reactor.py:613-645 (numbers from the device diagnostics)."""
        d = self._device_diagnostics()
        s, n = self.state, self.config.n_zones
        print("\n" + "=" * 70 + "\nCSTR PHYSICS DIAGNOSTICS\n" + "=" * 70)
        print(f"\nTime: {s.time:.1f} s")
        print(f"Residence time: {self.transport.residence_time:.1f} min")
        print(f"Mixing time: {self.transport.mixing_time_seconds:.1f} s")
        print(f"\n{'Zone':<6} {'pH':<8} {'Cl(mg/L)':<10} {'T(°C)':<8} {'ρ(kg/m³)':<10}\n" + "-" * 50)
        for i in range(n):
            print(f"{i:<6} {s.pH[i]:<8.3f} {s.chlorine[i]:<10.3f} {s.temperature[i]:<8.2f} {s.density[i]:<10.2f}")
        print("\nConservation Laws:")
        print(f"  Total Chlorine: {d['total_chlorine_mg'][0]:.2f} mg")
        print(f"  Charge Balance: {d['charge_balance_mol'][0]:.2e} mol")
        print("\nMixing Quality:")
        print(f"  pH segregation index: {d['pH_segregation'][0]:.4f}")
        print(f"  Chlorine segregation index: {d['chlorine_segregation'][0]:.4f}")
        print("=" * 70 + "\n")


PhysicsEngine = IntegratedCSTR  # the name BASELINE.json uses for this API
