"""Helpers of the GPU tests and probes of the per-reactor programs (test_gpu_control.py ... test_gpu_trend.py,
test_gpu_program_shapes.py, tools/*_probe.py): a plant with sensors and plant I/O, a pair of PI loops, the plant's
observable state and every program's, the message of a refused parameter block, and the host side of the PLC scan --
the calls of one scan interval, the device's whole scan order (``HostScan.scan``) and the holding words of a host
master; the zone count -> kernel instantiation rule, the wavefront packing and the sensor suite's pass structure in a
packed wavefront."""
import importlib

import numpy as np
import pytest

import trend_ref as TR
from inject_ref import CMD_ACID, I_TARGET

DT, K = 10.0, 300          # 3000 s: the pH sensors' 1800 s warm-up ends inside the run
MASTER = (0.5, 0.25, 6.0)  # acid, chlorine, inlet flow commands the master writes

_E = importlib.import_module("ics-wt-physicsengine_amd").ReactorEnsemble
_native = importlib.import_module("ics-wt-physicsengine_amd.core._native")


def instantiation(n):
    """(level, row mode) of the step kernel that serves ``n`` zones, as ``with_step_kernel`` in csrc/wtphys.hip picks
    it: level = smallest l >= 1 with 2^l >= n, row mode for the zone counts that fill DPP rows exactly."""
    level = 1
    while (1 << level) < n:
        level += 1
    return level, n in (2, 4, 8, 16)


@pytest.fixture
def full_waves(monkeypatch):
    """The library spreads an ensemble smaller than the device's wavefront slots over more wavefronts than it needs
    (down to one reactor each); WT_FULL_WAVES, read when an ensemble is created, packs 64 // n reactors into each, as
    a large ensemble is packed.  Test modules import the fixture by name."""
    monkeypatch.setenv("WT_FULL_WAVES", "1")


def ragged_size(n, groups=5):
    """(R, N): reactors per wavefront at ``n`` zones, and ``groups`` full wavefront-groups plus a last one that holds a
    single reactor."""
    R = 64 // n
    return R, groups * R + 1


def wavefront_groups(ens):
    """Wavefront-groups the library deals the ensemble's reactors into (it spreads a small ensemble over more wavefronts
    than 64 // n reactors each would need).  Ask after the last step: the call also switches the wave diagnostics on."""
    import ctypes
    nw = ctypes.c_int64(0)
    _native.check(_native.lib().wt_ensemble_wave_diag(ens._h, None, 0, ctypes.byref(nw)))
    return int(nw.value)


PACKINGS = ("spread", "packed")


def set_packing(monkeypatch, packing):
    """How the ensembles created from now on are dealt into wavefronts: "packed" sets WT_FULL_WAVES (64 // n reactors in
    every wavefront), "spread" removes it (the library's own choice, which depends on the card's CU count)."""
    assert packing in PACKINGS, packing
    if packing == "packed":
        monkeypatch.setenv("WT_FULL_WAVES", "1")
    else:
        monkeypatch.delenv("WT_FULL_WAVES", raising=False)


def assert_packing(ens, packing):
    """The run really had the packing it was meant to have, by the library's own count of wavefront-groups: packed,
    ceil(N / (64 // n)) of them; spread, more than that wherever a wavefront has room for a second reactor and there is
    one (how many more is the library's business: it depends on the card).  Ask after the last step."""
    assert packing in PACKINGS, packing
    n, N = ens.n_zones, ens.n_reactors
    R = 64 // n
    full, got = -(-N // R), wavefront_groups(ens)
    if packing == "packed":
        assert got == full, (packing, n, N, got, full)
    elif R > 1 and N > 1:
        assert got > full, (packing, n, N, got, full)
    else:
        assert got == N, (packing, n, N, got)


class Packing:
    """What the ``packing`` fixture hands a test: ``name`` ("spread" or "packed"), ``place`` for an ensemble just created
    (packed runs take the identity placement, so that reactor r sits in slot r % R of group r // R; spread runs keep what
    they had) and ``check`` for an ensemble after its last step (``assert_packing``).  The fixture fails a test that
    never called ``check``."""

    def __init__(self, name):
        self.name, self.packed, self.checked = name, name == "packed", 0

    def __repr__(self):
        return self.name

    def place(self, ens):
        if self.packed:
            ens.set_placement(False)
        return ens

    def check(self, ens):
        assert_packing(ens, self.name)
        self.checked += 1


@pytest.fixture(params=PACKINGS)
def packing(request, monkeypatch):
    """Runs a test once with the library's own spreading of a small ensemble and once with full wavefronts.  Test modules
    import the fixture by name; a test that takes only some zone counts packed parametrises it indirectly."""
    p = Packing(request.param)
    set_packing(monkeypatch, p.name)
    yield p
    assert p.checked, f"a {p.name} test ended without asserting its wavefront-groups (Packing.check)"


def spread_only(monkeypatch):
    """The ``Packing`` of a test that keeps the id it had before a packed twin was written beside it: the library's own
    spreading, stated (WT_FULL_WAVES removed) and to be asserted through ``check`` like any other."""
    set_packing(monkeypatch, "spread")
    return Packing("spread")


def both_packings(argnames, argvalues, packed=None):
    """``pytest.mark.parametrize`` over ``argvalues`` and the ``packing`` fixture, for a test that was parametrised over
    ``argvalues`` before it ran packed as well: the spread cases keep the ids they always had (pytest's own for numbers
    and strings, name and index for anything else), the packed ones put ``packed`` in front.  ``packed``: the values
    that run packed, where not all do."""
    names = [a.strip() for a in argnames.split(",")]

    def ident(name, i, x):
        return x if isinstance(x, str) else str(x) if isinstance(x, (bool, int, float)) else f"{name}{i}"

    params = []
    for pk, values in (("spread", list(argvalues)), ("packed", list(argvalues if packed is None else packed))):
        for i, v in enumerate(values):
            vals = tuple(v) if len(names) > 1 else (v,)
            base = "-".join(ident(nm, i, x) for nm, x in zip(names, vals))
            params.append(pytest.param(*vals, pk, id=base if pk == "spread" else f"packed-{base}"))
    return pytest.mark.parametrize(",".join(names + ["packing"]), params, indirect=["packing"])


# Zone counts of the packed sensor, service and plant I/O cases: every program-carrying instantiation, the aligned
# multi-pass shapes (2, 4), the ones where a pass boundary cuts a sensor's run (3, 5, 6) and single-pass shapes at 8, 5,
# 4, 3 and 2 reactors per wavefront (tests/test_sensor_passes.py asserts it)
SENSOR_NS = (2, 3, 4, 5, 6, 8, 12, 16, 20, 32)
SENSOR_LINES = ((0, 5), (1, 6))    # (pH electrode, RTD) of the inlet and of the outlet sample line


class SensorPasses:
    """The lane rule of ``wts::suite_step`` (csrc/wt_sensors.hpp) in a wavefront that holds R = 64 // n reactors: lane l
    of pass p reads sensor idx // R of slot idx % R, idx = 64 p + l, over 7 R sensor lanes.
    ``cuts``: sensor -> first slot of its run that falls in the later pass, for the sensors a pass boundary cuts;
    ``split``: line -> the slots whose RTD lane runs in a later pass than the pH lane it takes the line from."""

    def __init__(self, n):
        self.n, self.R = n, 64 // n
        self.lanes = 7 * self.R
        self.passes = -(-self.lanes // 64)
        self.cuts, self.split = {}, {}
        for i in range(7):
            first, last = self.pass_of(i, 0), self.pass_of(i, self.R - 1)
            assert last - first <= 1
            if last != first:
                self.cuts[i] = 64 * last - i * self.R
        for line, (ph, rtd) in enumerate(SENSOR_LINES):
            assert all(self.pass_of(ph, sl) <= self.pass_of(rtd, sl) for sl in range(self.R))
            later = tuple(sl for sl in range(self.R) if self.pass_of(rtd, sl) > self.pass_of(ph, sl))
            if later:
                self.split[line] = later

    def pass_of(self, sensor, slot):
        return (sensor * self.R + slot) // 64


def sensor_passes(n):
    return SensorPasses(n)


def assert_equal_by_reactor(ref, got, what, R):
    """``assert_all_equal`` for arrays whose last axis is the reactor: a mismatch names the reactors and, for the identity
    placement, their (wavefront-group, slot)."""
    for i, (a, b) in enumerate(zip(ref, got)):
        a, b = np.asarray(a), np.asarray(b)
        assert a.shape == b.shape, (what, i, a.shape, b.shape)
        bad = ~((a == b) | (np.isnan(a) & np.isnan(b)))
        if bad.any():
            rs = np.unique(np.nonzero(bad)[-1])
            raise AssertionError((what, i, "reactors", rs[:8].tolist(), "(group, slot)", [(int(r) // R, int(r) % R) for r in rs[:8]]))


_SPREAD = {}


def equals_spread(monkeypatch, packing, key, n, got, run):
    """``got``: the arrays (reactor on the last axis) a test's run left under ``packing``.  A spread case files them
    under ``key``; a packed case requires its own to equal them bit for bit and names mismatches as (group, slot).  A
    packed case that runs before its spread twin, or has none, makes the spread run itself: ``run(Packing("spread"))``,
    which must end in the twin's ``check``."""
    if not packing.packed:
        _SPREAD[key] = got
        return
    if key not in _SPREAD:
        set_packing(monkeypatch, "spread")
        twin = Packing("spread")
        _SPREAD[key] = run(twin)
        assert twin.checked, key
    assert len(_SPREAD[key]) == len(got), key
    assert_equal_by_reactor(_SPREAD[key], got, ("packed against spread", key), 64 // n)


def plant(wt, cols, bc, n, seed=11, history=0):
    ens = wt.ReactorEnsemble(cols, n_zones=n)
    ens.set_boundary(bc)
    ens.enable_sensors(seed=seed, history=history)
    ens.enable_plant_io()
    return ens


def pi_loops(wt, cols, seed=5):
    """Both loops on, per-reactor gains and setpoints: chlorine dosing on the outlet DPD reading, acid dosing (reverse
    acting: more acid while the pH is above its setpoint) on the outlet pH probe."""
    N = len(cols["initial_chlorine"])
    u = np.random.default_rng(seed).random((6, N))
    chlorine = wt.PILoop("chlorine_outlet", setpoint=cols["initial_chlorine"] + u[0], kp=0.2 + 1.8 * u[1],
                         ki=1e-4 + 2e-3 * u[2], bias=0.2)
    acid = wt.PILoop("pH_outlet", setpoint=6.8 + 0.6 * u[3], kp=0.1 + 0.9 * u[4], ki=1e-4 + 1e-3 * u[5], direction=-1,
                     bias=0.1)
    return chlorine, acid


def plant_state(ens):
    """State, sensor readings and boundary of every reactor."""
    es = ens.state
    v, s, f = ens.sensor_readings()
    return (es.pH, es.chlorine, es.temperature, es.time, es.flow_rate, es.status, v, s, f, ens.boundary())


def alarms(ens):
    """The device's alarm state, reset state and words; ``ref_alarms`` is the restatement's side of the comparison."""
    return ens.alarm_state().block() + (ens.alarm_words(),)


def ref_alarms(ref):
    return ref.st, ref.rst, ref.words


def acts(ens):
    """The device's actuator state, queues, t_prev and the boundary rows the elements drive; ``ref_acts`` likewise."""
    return ens.actuator_state().block() + (ens.boundary()[[0, 4, 6]],)


def ref_acts(ref):
    return ref.st, ref.q, ref.t_prev, ref.rows()


def _disturbance(ens):
    d = ens.disturbance_state()
    return d.value, d.x, d.n_eval, d.n_draw, d.base, d.t_prev


def _score(ens):
    c = ens.score_curve()
    return tuple(vars(ens.score_state()).values()) + (c.n_scored, c.n_low, c.n_high)


# what ``everything`` returns of each program, in its order
_STATE = dict(control=lambda ens: (ens.control_state().block(),), inject=lambda ens: (ens.injection_state().block(),),
              alarm=alarms, actuator=acts, detect=lambda ens: tuple(ens.detector_state().block()), disturb=_disturbance,
              score=_score)
SCAN_PROGRAMS = ("control", "inject", "alarm", "actuator")


def everything(ens, *, programs=SCAN_PROGRAMS):
    """State, readings, boundary and input image of every reactor, then the state blocks of the named programs (each
    must be set), in the fixed order control, inject, alarm, actuator, detect, disturb, score."""
    assert set(programs) <= set(_STATE), programs
    out = plant_state(ens) + ens.input_image()
    for name, state in _STATE.items():
        if name in programs:
            out += tuple(state(ens))
    return out


def trend_tag_values(ens, image=None):
    """Tag -> rows of the trend recorder's values at the scan that closed the last call, from the public getters of an
    ensemble with all of control, injection, alarm, actuator and detector programs set.  ``image``: the (values, faults)
    that scan saw, for the reading tags; without it they are left to ``HostScan.tag_values``."""
    N = ens.n_reactors
    rows = lambda block: block.reshape(-1, N)
    out = {TR.COMMAND: ens.boundary()[[4, 6, 0]], TR.CONTROL: rows(ens.control_state().block()),
           TR.INJECT: rows(ens.injection_state().block()), TR.ALARM: rows(ens.alarm_state().block()[0]),
           TR.ALARM_WORD: ens.alarm_words().astype(np.float64), TR.ACTUATOR: rows(ens.actuator_state().block()[0]),
           TR.DETECT: rows(ens.detector_state().block()[0])}
    if image is not None:
        v, _, f = ens.sensor_readings()
        out.update(_reading_tags(v, f, *image))
    return out


def _reading_tags(v, f, vt, ft):
    return {TR.IMAGE_VALUE: np.asarray(vt, dtype=np.float64), TR.IMAGE_FAULT: np.asarray(ft, dtype=np.float64),
            TR.FIELD_VALUE: np.asarray(v, dtype=np.float64), TR.FIELD_FAULT: np.asarray(f, dtype=np.float64)}


def refused_as_checked(nat, program, block) -> bool:
    """The message of the set call just refused on ``block`` is the one wt_program_check gives for it."""
    msg = nat.lib().wt_last_error()
    return (nat.lib().wt_program_check(program, nat.dptr(block), block.shape[-1]) == nat.WT_E_ARG
            and nat.lib().wt_last_error() == msg)


def assert_all_equal(ref, got, what):
    for i, (a, b) in enumerate(zip(ref, got)):
        assert np.array_equal(a, b, equal_nan=True), (what, i)


def words(cmd):
    """(3, N) (acid, chlorine, inlet) commands -> (N, 6) holding words."""
    return np.concatenate([_E.encode_float32(cmd[i]) for i in range(3)], axis=1)


def commands(holding):
    """(N, 6) holding words -> (3, N) float32 (acid, chlorine, inlet) commands."""
    return _E.decode_float32(np.asarray(holding).reshape(-1, 3, 2)).T.copy()


def calls(n_steps, interval, lt=0.0, dt=DT):
    """``n_steps`` outer steps as calls of one scan interval: yields each call's length and the loop time after it.  The
    loop time advances by repeated addition of ``dt`` from ``lt``, as the device's does (c * dt rounds otherwise)."""
    done = 0
    while done < n_steps:
        c = min(interval, n_steps - done)
        for _ in range(c):
            lt = lt + dt
        yield c, lt
        done += c


class HostScan:
    """The host side of the PLC scan of N reactors, the one host-side statement of the device's scan order: inject ->
    pack -> apply commands -> alarm override -> actuator -> loop time -> tune -> PI -> alarm -> detector -> trend.  It
    holds the restatements of the programs that are on (``ctl`` ControlRef, ``tun`` TuneRef, ``inj`` InjectRef, ``alm``
    AlarmRef, ``act`` ActuatorRef, ``det`` DetectRef, ``trd`` TrendRef; None for a program that is off) and the loop
    time ``lt`` (N,) of the next scan.  The disturbance and score programs run after every outer step and the service
    program after every read, not in the scan, and stay outside.

    ``emulated``: the device runs plant I/O without these programs, and the host master emulates the command path in
    the words it writes before a call (``holding``).  Otherwise the device runs them, and ``scan`` follows its command
    path from the decoded commands it is given."""

    def __init__(self, N, ctl=None, inj=None, alm=None, act=None, det=None, trd=None, tun=None, emulated=False, dt=DT):
        self.ctl, self.tun, self.inj, self.alm, self.act, self.det, self.trd = ctl, tun, inj, alm, act, det, trd
        self.emulated, self.dt = emulated, dt
        self.lt = np.zeros(N)
        self.values = None         # the tag -> rows dict the trend recorder saw at the last scan
        # an injection program without command slots leaves the commands as they are: skip its copy of them
        self.tampers = inj is not None and bool((inj.p[:, I_TARGET] >= CMD_ACID).any())

    def calls(self, n_steps, interval):
        """The lengths of ``calls``; inside the loop ``lt`` is the loop time the scan closing the call stores."""
        for c, self.lt in calls(n_steps, interval, self.lt, self.dt):
            yield c

    def _command_path(self, cmd, stepped=None):
        """The decoded commands (3, N) after the injection's command slots and then the alarm trips in force."""
        if self.tampers:
            cmd = self.inj.commands(cmd, self.lt, stepped)
        if self.alm is not None:
            cmd = self.alm.override(cmd, stepped)
        return cmd

    def holding(self, cmd=None):
        """The words a host master writes before a call: those of ``cmd`` (3, N), by default the PI's holding words
        (which a tuner beside it shares; the tuner's own without a PI).
        When ``emulated``, the injection's command slots and the alarm trips in force act on them here, at the loop time
        of the scan that closes the call; the alarm program then counts its overrides here and not in ``scan``."""
        own = None if cmd is not None else self.tun.holding if self.ctl is None else self.ctl.holding
        if self.emulated and (self.tampers or self.alm is not None):
            return words(self._command_path(commands(own) if cmd is None else cmd))
        return own if cmd is None else words(cmd)

    def tag_values(self, v, f, vt, ft):
        """Tag -> rows of what a trend slot can read at the end of a scan, for every tag whose source is held here:
        the image (``vt``, ``ft``) and field (``v``, ``f``) readings and fault codes, and the state of the restatements
        that are on, laid out as the device's get blocks (row = ``unit * rows + row``).  A tag without a source is
        absent and reads NaN, as on the device; COMMAND is the caller's (``scan``'s ``tags``): the validated command
        rows are the device's ``boundary()``."""
        N = len(self.lt)
        out = _reading_tags(v, f, vt, ft)
        for tag, ref in ((TR.CONTROL, self.ctl), (TR.INJECT, self.inj), (TR.ALARM, self.alm), (TR.ACTUATOR, self.act),
                         (TR.DETECT, self.det)):
            if ref is not None:
                out[tag] = ref.st.reshape(-1, N)
        if self.alm is not None:
            out[TR.ALARM_WORD] = self.alm.words.astype(np.float64)
        return out

    def scan(self, v, f, cmd=None, stepped=None, tags=None):
        """One PLC scan at loop time ``lt`` in the device's order (the blocks under ``if (plc_on)`` of ``run_item`` in
        csrc/wt_step.hpp):
          inject          the injection's sensor slots tamper the readings ``v`` / ``f`` (7, N),
          pack            which the input image then packs;
          apply commands  the decoded commands ``cmd`` (3, N) go through the injection's command slots,
          alarm override  the alarm trips in force
          actuator        and the actuators (no command path with ``cmd`` None);
          loop time       the scan stores ``lt``;
          tune            the tuners run on the tampered readings and own the loops whose experiment is live;
          PI              runs on the tampered readings and skips the loops the tuners owned in this scan;
          alarm           FIELD slots on the raw readings, IMAGE slots on the tampered ones;
          detector        likewise;
          trend           last: a sample is an entry of ``tag_values`` as it stands at the end of this scan, with the
                          entries of ``tags`` (tag -> rows) added or put in their place.
        ``stepped`` (N,): reactors that took the step (default: all).  Returns the tampered readings."""
        assert cmd is None or not self.emulated, "an emulated command path runs in holding()"
        t = self.lt
        vt, ft = (v, f) if self.inj is None else self.inj.sensors(v, f, t, stepped)
        if cmd is not None:
            cmd = self._command_path(cmd, stepped)
            if self.act is not None:
                self.act.scan(cmd, t, stepped)
        if self.tun is not None:
            self.tun.scan(vt, ft, t, stepped)
        if self.ctl is not None:
            self.ctl.scan(vt, ft, t, stepped, skip=None if self.tun is None else self.tun.owned)
        if self.alm is not None:
            self.alm.scan(v, f, t, stepped, image=(vt, ft))
        if self.det is not None:
            self.det.scan(v, f, t, stepped, image=(vt, ft))
        if self.trd is not None:
            self.values = {**self.tag_values(v, f, vt, ft), **(tags or {})}
            self.trd.scan(self.values, t, stepped)
        return vt, ft

    def run(self, ens, n_steps, interval, fused=True, image=False):
        """The host loop a fused call replaces: calls of one scan interval, each after the master's write of
        ``holding()`` and closed by ``scan`` of the readings (and, unless ``emulated``, of the commands written).
        ``image``: read the input image after every call, as a host master would.  A trend recorder gets its COMMAND
        rows from the device's ``boundary()``.  Returns the last scan's tampered readings."""
        for c in self.calls(n_steps, interval):
            w = self.holding()
            ens.write_holding(w)
            ens.step(self.dt, n_steps=c, fused=fused, download=False)
            v, _, f = ens.sensor_readings()
            if image:
                ens.input_image()
            tags = None if self.trd is None else {TR.COMMAND: ens.boundary()[[4, 6, 0]]}
            out = self.scan(v, f, None if self.emulated else commands(w), tags=tags)
        return out
