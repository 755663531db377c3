"""Host restatement of the per-reactor response programs (include/wtphys.h, csrc/wt_rsp.hpp), vectorised over reactors,
operation for operation.

numpy fp64 never contracts a product and a sum into an fma, and every expression below has the association the device
code has, so the results are bit-comparable with ``ReactorEnsemble.response_state()``.  ``RespondRef`` runs after the
tuners and before the controllers and the PI programs; ``ResponseOwners`` puts a ``TuneRef``, a ``RespondRef`` and an
``MpcRef`` together as the one object ``HostScan`` takes as its ``tun``, which makes
``HostScan(..., tun=ResponseOwners(...))`` the host statement of the scan order
... -> loop time -> tune -> response -> mpc -> PI -> alarm -> detector -> ...
The restatement holds references to the ``AlarmRef`` and the ``DetectRef`` and reads their state when it scans, which
is before they do: the previous scan's state, as on the device.
"""
import numpy as np

from alarm_ref import AS_ACTIVE
from control_ref import C_BIAS, C_DIRECTION, C_ENABLE, C_KP, C_SENSOR, C_SETPOINT, CS_INTEGRAL, HOLDING_WORD, float32_words
from detect_ref import KS_ALARM
from mpc_ref import M_ENABLE, MS_OUTPUT, MS_PHASE, RUNNING

(R_CAUSE, R_INDEX, R_DELAY, R_LOOP, R_ACTION, R_VALUE, R_RATE, R_LATCH, R_CLEAR_DELAY, R_MIN_HOLD, R_HANDBACK) = range(11)
(RS_PHASE, RS_PENDING, RS_CLEARING, RS_OUTPUT, RS_T_FIRST, RS_T_ENGAGED, RS_T_RELEASED, RS_N_ENGAGED, RS_TIME_ENGAGED,
 RS_N_OWNED, RS_N_BLOCKED, RS_N_CAUSE, RS_N_TRACKED, RS_N_HANDBACK) = range(14)
RR_T_PREV, RR_OWNER_CHLORINE, RR_OWNER_ACID = range(3)
OFF, ALARM, DETECTOR, BAD = range(4)
HOLD, MANUAL, RAMP = range(3)
BUMP, BUMPLESS = range(2)
IDLE, ENGAGED = range(2)
_NAN_ROWS = (RS_PENDING, RS_CLEARING, RS_T_FIRST, RS_T_ENGAGED, RS_T_RELEASED)


def words_value(holding, loop):
    """The float32 the words of ``loop`` (N,) decode to, widened to float64: (N,)."""
    col = np.where(np.asarray(loop) == 0, HOLDING_WORD[0], HOLDING_WORD[1])
    idx = np.arange(len(col))
    bits = (holding[idx, col].astype(np.uint32) << 16) | holding[idx, col + 1].astype(np.uint32)
    return bits.view(np.float32).astype(np.float64)


class RespondRef:
    """State of the four slots of N reactors.  ``params`` (4, 11, N) block; ``loop_time`` (N,) loop time at set.
    ``words``: an object whose ``holding`` (N, 6) words the slots read and write, in place (a ``ControlRef``, a
    ``TuneRef`` or an ``MpcRef`` that runs beside them); None: words of their own, all 0 as plant I/O starts.  ``ctl``,
    ``mpc``: the ``ControlRef`` and ``MpcRef`` a bumpless hand-back writes into; ``alm``, ``det``: the ``AlarmRef`` and
    ``DetectRef`` the causes read; None for a program that is off.  ``owned`` (2, N): the loops the slots held in the
    last scan."""

    def __init__(self, params, loop_time, words=None, ctl=None, mpc=None, alm=None, det=None):
        self.p = np.array(params, dtype=np.float64)
        N = self.p.shape[2]
        self.ctl, self.mpc, self.alm, self.det = ctl, mpc, alm, det
        self.holding = np.zeros((N, 6), dtype=np.uint16) if words is None else words.holding
        self.owned = np.zeros((2, N), dtype=bool)
        self.reset(loop_time)

    def reset(self, loop_time):
        N = self.p.shape[2]
        self.st = np.zeros((4, 14, N))
        self.st[:, _NAN_ROWS] = np.nan
        self.rst = np.full((3, N), -1.0)
        self.rst[RR_T_PREV] = np.broadcast_to(np.asarray(loop_time, dtype=np.float64), (N,))

    def scan(self, values, faults, t_now, stepped=None, skip=None):
        """One PLC scan: ``values`` float32 (7, N) readings as the image sees them, ``faults`` (7, N), ``t_now`` (N,) the
        loop time the scan stores, ``stepped`` (N,) reactors that took the step (default: all), ``skip`` (2, N) the loops
        the tuners owned in this scan (default: none)."""
        N = self.p.shape[2]
        stepped = np.ones(N, dtype=bool) if stepped is None else np.asarray(stepped, dtype=bool)
        skip = np.zeros((2, N), dtype=bool) if skip is None else np.asarray(skip, dtype=bool)
        t = np.array(np.broadcast_to(np.asarray(t_now, dtype=np.float64), (N,)))
        idx = np.arange(N)
        v32 = np.asarray(values, dtype=np.float32)
        faults = np.asarray(faults)
        bad_reading = ~np.isfinite(v32) | (faults != 0)
        h = t - self.rst[RR_T_PREV]
        self.rst[RR_T_PREV] = np.where(stepped, t, self.rst[RR_T_PREV])
        prev = self.rst[RR_OWNER_CHLORINE:RR_OWNER_ACID + 1].copy()
        own = np.full((2, N), -1, dtype=np.int64)                   # this scan's owner of each loop
        held = np.zeros((2, N), dtype=bool)
        nan = np.nan
        with np.errstate(invalid="ignore", over="ignore"):
            for s in range(4):
                p, q = self.p[s], self.st[s]
                live = stepped & (p[R_CAUSE] != OFF)
                ix, l = p[R_INDEX].astype(np.int64), np.clip(p[R_LOOP].astype(np.int64), 0, 1)
                # 1. the cause
                c = (p[R_CAUSE] == BAD) & bad_reading[np.clip(ix, 0, 6), idx]
                if self.alm is not None:
                    c = c | ((p[R_CAUSE] == ALARM) & (self.alm.st[np.clip(ix, 0, 3), AS_ACTIVE, idx] != 0))
                if self.det is not None:
                    c = c | ((p[R_CAUSE] == DETECTOR) & (self.det.st[np.clip(ix, 0, 3), KS_ALARM, idx] != 0))
                c = c & live
                q[RS_N_CAUSE] += c
                was = live & (q[RS_PHASE] != IDLE)
                idle = live & ~was
                blocked = skip[l, idx]
                above = own[l, idx]
                # 2. engaged over the interval that just ended; the release
                q[RS_TIME_ENGAGED] = np.where(was, q[RS_TIME_ENGAGED] + h, q[RS_TIME_ENGAGED])
                unlatched = was & (p[R_LATCH] == 0)
                q[RS_CLEARING] = np.where(unlatched & c, nan, q[RS_CLEARING])
                cl = unlatched & ~c
                clearing = np.where(np.isnan(q[RS_CLEARING]), t, q[RS_CLEARING])
                rel = cl & (t - clearing >= p[R_CLEAR_DELAY]) & (t - q[RS_T_ENGAGED] >= p[R_MIN_HOLD])
                q[RS_CLEARING] = np.where(cl, np.where(rel, nan, clearing), q[RS_CLEARING])
                q[RS_PHASE] = np.where(rel, float(IDLE), q[RS_PHASE])
                q[RS_T_RELEASED] = np.where(rel, t, q[RS_T_RELEASED])
                hb = rel & (p[R_HANDBACK] == BUMPLESS) & (prev[l, idx] == s) & ~blocked & (above < 0)
                q[RS_N_HANDBACK] += hb
                out = q[RS_OUTPUT]
                for ll in range(2):
                    if self.ctl is not None:
                        cp = self.ctl.p[ll]
                        m = hb & (l == ll) & (cp[C_ENABLE] != 0)
                        si = cp[C_SENSOR].astype(np.int64)
                        v = v32[si, idx]
                        ok = np.isfinite(v) & (faults[si, idx] == 0)
                        e = cp[C_DIRECTION] * (cp[C_SETPOINT] - v.astype(np.float64))
                        base = np.where(ok, cp[C_BIAS] + cp[C_KP] * e, cp[C_BIAS])
                        self.ctl.st[ll, CS_INTEGRAL] = np.where(m, out - base, self.ctl.st[ll, CS_INTEGRAL])
                    if self.mpc is not None:
                        m = hb & (l == ll) & (self.mpc.p[ll, M_ENABLE] != 0) & (self.mpc.st[ll, MS_PHASE] == RUNNING)
                        self.mpc.st[ll, MS_OUTPUT] = np.where(m, out, self.mpc.st[ll, MS_OUTPUT])
                # 3. the reaction time; the engagement
                q[RS_PENDING] = np.where(idle & ~c, nan, q[RS_PENDING])
                pc = idle & c
                pending = np.where(np.isnan(q[RS_PENDING]), t, q[RS_PENDING])
                eng = pc & (t - pending >= p[R_DELAY])
                q[RS_PENDING] = np.where(pc, np.where(eng, nan, pending), q[RS_PENDING])
                q[RS_PHASE] = np.where(eng, float(ENGAGED), q[RS_PHASE])
                q[RS_CLEARING] = np.where(eng, nan, q[RS_CLEARING])
                q[RS_N_ENGAGED] += eng
                q[RS_T_FIRST] = np.where(eng & np.isnan(q[RS_T_FIRST]), t, q[RS_T_FIRST])
                q[RS_T_ENGAGED] = np.where(eng, t, q[RS_T_ENGAGED])
                q[RS_OUTPUT] = np.where(eng, words_value(self.holding, l), q[RS_OUTPUT])
                # 4. the loop
                now = (was & ~rel) | eng
                q[RS_N_BLOCKED] += now & blocked
                tracks = now & ~blocked & (above >= 0)
                q[RS_OUTPUT] = np.where(tracks, self.st[np.clip(above, 0, 3), RS_OUTPUT, idx], q[RS_OUTPUT])
                q[RS_N_TRACKED] += tracks
                owns = now & ~blocked & (above < 0)
                output = q[RS_OUTPUT]
                step = p[R_RATE] * h
                d = p[R_VALUE] - output
                ramp = np.where(d > step, output + step, np.where(d < -step, output - step, p[R_VALUE]))
                y = np.where(p[R_ACTION] == MANUAL, p[R_VALUE], np.where(p[R_ACTION] == RAMP, ramp, output))
                q[RS_OUTPUT] = np.where(owns, y, output)
                q[RS_N_OWNED] += owns
                for ll in range(2):
                    m = owns & (l == ll)
                    w = HOLDING_WORD[ll]
                    self.holding[m, w:w + 2] = float32_words(y[m])
                    own[ll, m] = s
                    held[ll] |= m
        self.rst[RR_OWNER_CHLORINE:RR_OWNER_ACID + 1] = np.where(stepped, own.astype(np.float64), prev)
        self.owned = held


class ResponseOwners:
    """A ``TuneRef`` (or None), a ``RespondRef`` and an ``MpcRef`` (or None) as ``HostScan``'s ``tun``: the tuners run,
    then the response slots with the tuners' mask, then the controllers with the union of both; ``owned`` is the union of
    all three, which the PI programs skip; ``holding`` is the one image they share."""

    def __init__(self, tun, rsp, mpc=None):
        self.tun, self.rsp, self.mpc = tun, rsp, mpc
        assert tun is None or tun.holding is rsp.holding, "one holding image"
        assert mpc is None or mpc.holding is rsp.holding, "one holding image"
        self.owned = np.zeros_like(rsp.owned)

    @property
    def holding(self):
        return self.rsp.holding

    def scan(self, values, faults, t_now, stepped=None):
        skip = None
        if self.tun is not None:
            self.tun.scan(values, faults, t_now, stepped)
            skip = self.tun.owned
        self.rsp.scan(values, faults, t_now, stepped, skip=skip)
        owned = self.rsp.owned if skip is None else (skip | self.rsp.owned)
        if self.mpc is not None:
            self.mpc.scan(values, faults, t_now, stepped, skip=owned)
            owned = owned | self.mpc.owned
        self.owned = owned
