"""Helpers of the GPU tests and probes of the per-reactor scan programs (test_gpu_control.py, test_gpu_inject.py,
test_gpu_alarm.py, test_gpu_actuator.py, test_gpu_program_shapes.py, tools/*_probe.py): a plant with sensors and plant I/O, a pair of PI loops, the
plant's observable state, the message of a refused parameter block, and the host side of the PLC scan -- the calls of
one scan interval, the device's scan order and the holding words of a host master; the zone count -> kernel instantiation
rule and the wavefront packing."""
import importlib

import numpy as np

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
    """The host side of the PLC scan of N reactors: the restatements of the programs that are on (``ctl`` ControlRef,
    ``inj`` InjectRef, ``alm`` AlarmRef, ``act`` ActuatorRef; None for a program that is off) and the loop time ``lt``
    (N,) of the next scan.

    ``emulated``: the device runs plant I/O without these programs, and the host master emulates the command path in
    the words it writes before a call (``holding``).  Otherwise the device runs them, and ``scan`` follows its command
    path from the decoded commands it is given."""

    def __init__(self, N, ctl=None, inj=None, alm=None, act=None, emulated=False, dt=DT):
        self.ctl, self.inj, self.alm, self.act = ctl, inj, alm, act
        self.emulated, self.dt = emulated, dt
        self.lt = np.zeros(N)
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
        """The words a host master writes before a call: those of ``cmd`` (3, N), by default the PI's holding words.
        When ``emulated``, the injection's command slots and the alarm trips in force act on them here, at the loop time
        of the scan that closes the call; the alarm program then counts its overrides here and not in ``scan``."""
        if self.emulated and (self.tampers or self.alm is not None):
            return words(self._command_path(commands(self.ctl.holding) if cmd is None else cmd))
        return self.ctl.holding if cmd is None else words(cmd)

    def scan(self, v, f, cmd=None, stepped=None):
        """One PLC scan at loop time ``lt`` in the device's order (the plant-I/O section of ``run_item`` in
        csrc/wt_device.hpp): the injection's sensor slots tamper the readings ``v`` / ``f`` (7, N), which the input
        image then packs; the decoded commands ``cmd`` (3, N) go through the injection's command slots, the alarm trips
        and the actuators (no command path with ``cmd`` None); PI runs on the tampered readings; the alarms evaluate,
        FIELD slots on the raw readings and IMAGE slots on the tampered ones.  ``stepped`` (N,): reactors that took
        the step (default: all).  Returns the tampered readings."""
        assert cmd is None or not self.emulated, "an emulated command path runs in holding()"
        t = self.lt
        vt, ft = (v, f) if self.inj is None else self.inj.sensors(v, f, t, stepped)
        if cmd is not None:
            cmd = self._command_path(cmd, stepped)
            if self.act is not None:
                self.act.scan(cmd, t, stepped)
        if self.ctl is not None:
            self.ctl.scan(vt, ft, t, stepped)
        if self.alm is not None:
            self.alm.scan(v, f, t, stepped, image=(vt, ft))
        return vt, ft

    def run(self, ens, n_steps, interval, fused=True, image=False):
        """The host loop a fused call replaces: calls of one scan interval, each after the master's write of
        ``holding()`` and closed by ``scan`` of the readings (and, unless ``emulated``, of the commands written).
        ``image``: read the input image after every call, as a host master would.  Returns the last scan's
        tampered readings."""
        for c in self.calls(n_steps, interval):
            w = self.holding()
            ens.write_holding(w)
            ens.step(self.dt, n_steps=c, fused=fused, download=False)
            v, _, f = ens.sensor_readings()
            if image:
                ens.input_image()
            out = self.scan(v, f, None if self.emulated else commands(w))
        return out
