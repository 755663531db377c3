"""Host restatement of the per-reactor alarm and interlock programs (include/wtphys.h, csrc/wt_alm.hpp), vectorised
over reactors.

numpy fp64 never contracts a product and a sum into an fma and every comparison below has the operands the device
code has, so the state and the words are bit-comparable with ``ReactorEnsemble.alarm_state()`` / ``alarm_words()``.
"""
import numpy as np

A_KIND, A_SENSOR, A_SOURCE, A_SETPOINT, A_DEADBAND, A_ON_DELAY, A_LATCH, A_ON_BAD, A_ACTION, A_TRIP_VALUE = range(10)
AS_ACTIVE, AS_COND, AS_PENDING, AS_N_ACT, AS_T_FIRST, AS_T_LAST, AS_TIME_ACTIVE, AS_N_BAD = range(8)
AR_T_PREV, AR_FIRST_OUT, AR_OVR_ACID, AR_OVR_CHLORINE, AR_N_OVR_ACID, AR_N_OVR_CHLORINE = range(6)
OFF, HIGH, LOW = range(3)
IMAGE, FIELD = range(2)
HOLD, ALARM = range(2)
NONE, TRIP_ACID, TRIP_CHLORINE = range(3)


class AlarmRef:
    """State of the program of N reactors.  ``params``: (4, 10, N) block of ``alarm_block``; ``loop_time``: (N,) loop
    time at set."""

    def __init__(self, params, loop_time):
        self.p = np.array(params, dtype=np.float64)
        S, _, N = self.p.shape
        self.st = np.zeros((S, 8, N))
        self.st[:, [AS_PENDING, AS_T_FIRST, AS_T_LAST]] = np.nan
        self.rst = np.zeros((6, N))
        self.rst[AR_T_PREV] = np.broadcast_to(np.asarray(loop_time, dtype=np.float64), (N,))
        self.rst[AR_FIRST_OUT] = -1.0
        self.rst[[AR_OVR_ACID, AR_OVR_CHLORINE]] = np.nan
        self.words = np.zeros(N, dtype=np.uint16)

    def scan(self, v, f, t, stepped=None, image=None):
        """One PLC scan: ``v`` float32 (7, N) field readings, ``f`` (7, N) their fault codes, ``t`` (N,) the loop time
        the scan stores, ``stepped`` (N,) reactors that took the step (default: all), ``image`` the scan's (values,
        faults) after an injection program (default: the field readings)."""
        S, _, N = self.p.shape
        stepped = np.ones(N, dtype=bool) if stepped is None else np.asarray(stepped, dtype=bool)
        t = np.broadcast_to(np.asarray(t, dtype=np.float64), (N,))
        fv, ff = np.asarray(v, dtype=np.float32), np.asarray(f).astype(np.int64)
        iv, iff = (fv, ff) if image is None else (np.asarray(image[0], dtype=np.float32), np.asarray(image[1]).astype(np.int64))
        rs = self.rst
        h = t - rs[AR_T_PREV]
        rs[AR_T_PREV] = np.where(stepped, t, rs[AR_T_PREV])
        first_out = rs[AR_FIRST_OUT].copy()
        idx = np.arange(N)
        for s in range(S):
            p, q = self.p[s], self.st[s]
            on = stepped & (p[A_KIND] != OFF)
            active = q[AS_ACTIVE] != 0
            q[AS_TIME_ACTIVE] = np.where(on & active, q[AS_TIME_ACTIVE] + h, q[AS_TIME_ACTIVE])
            si = p[A_SENSOR].astype(np.int64)
            field = p[A_SOURCE] == FIELD
            val = np.where(field, fv[si, idx], iv[si, idx])
            flt = np.where(field, ff[si, idx], iff[si, idx])
            bad = ~np.isfinite(val) | (flt != 0)
            q[AS_N_BAD] = np.where(on & bad, q[AS_N_BAD] + 1.0, q[AS_N_BAD])
            ev = on & ~(bad & (p[A_ON_BAD] == HOLD))
            vd = val.astype(np.float64)
            sp, db = p[A_SETPOINT], p[A_DEADBAND]
            with np.errstate(invalid="ignore"):
                high = np.where(active, ~(vd < sp - db), vd > sp)
                low = np.where(active, ~(vd > sp + db), vd < sp)
            c = bad | np.where(p[A_KIND] == HIGH, high, low)
            q[AS_COND] = np.where(ev, c.astype(np.float64), q[AS_COND])
            rise = ev & ~active & c
            pending = np.where(rise & np.isnan(q[AS_PENDING]), t, q[AS_PENDING])
            fire = rise & (t - pending >= p[A_ON_DELAY])
            q[AS_PENDING] = np.where(fire | (ev & ~active & ~c), np.nan, np.where(rise, pending, q[AS_PENDING]))
            q[AS_N_ACT] = np.where(fire, q[AS_N_ACT] + 1.0, q[AS_N_ACT])
            q[AS_T_FIRST] = np.where(fire & np.isnan(q[AS_T_FIRST]), t, q[AS_T_FIRST])
            first_out = np.where(fire & (first_out == -1.0), float(s), first_out)
            drop = ev & active & ~c & (p[A_LATCH] == 0)
            now = (active & ~drop) | fire
            q[AS_ACTIVE] = now.astype(np.float64)
            q[AS_T_LAST] = np.where(ev & now, t, q[AS_T_LAST])
        rs[AR_FIRST_OUT] = np.where(stepped, first_out, rs[AR_FIRST_OUT])
        self._settle(stepped)

    def _settle(self, mask):
        """ovr_*, the word (and first_out with no active slot, after a reset) of the reactors in ``mask``."""
        S, _, N = self.p.shape
        ovr = np.full((2, N), np.nan)
        word = np.zeros(N, dtype=np.int64)
        for s in range(S):
            act = self.st[s, AS_ACTIVE] != 0
            for k, code in enumerate((TRIP_ACID, TRIP_CHLORINE)):
                take = act & (self.p[s, A_ACTION] == code) & np.isnan(ovr[k])
                ovr[k] = np.where(take, self.p[s, A_TRIP_VALUE], ovr[k])
            word |= act.astype(np.int64) << s
            word |= (self.st[s, AS_COND] != 0).astype(np.int64) << (4 + s)
        rs = self.rst
        rs[AR_OVR_ACID] = np.where(mask, ovr[0], rs[AR_OVR_ACID])
        rs[AR_OVR_CHLORINE] = np.where(mask, ovr[1], rs[AR_OVR_CHLORINE])
        word |= (~np.isnan(rs[AR_OVR_ACID])).astype(np.int64) << 8
        word |= (~np.isnan(rs[AR_OVR_CHLORINE])).astype(np.int64) << 9
        word |= (rs[AR_FIRST_OUT].astype(np.int64) + 1) << 12
        self.words = np.where(mask, word, self.words).astype(np.uint16)

    def override(self, cmd, stepped=None):
        """The interlock at a scan on the decoded (acid, chlorine, inlet) commands (3, N): a float32 copy with the
        tripped channels replaced by float32(trip value) -- what a host master writes to get the device's commands."""
        N = self.p.shape[2]
        stepped = np.ones(N, dtype=bool) if stepped is None else np.asarray(stepped, dtype=bool)
        out = np.array(cmd, dtype=np.float32)
        for row, k, n in ((0, AR_OVR_ACID, AR_N_OVR_ACID), (1, AR_OVR_CHLORINE, AR_N_OVR_CHLORINE)):
            on = stepped & ~np.isnan(self.rst[k])
            out[row] = np.where(on, self.rst[k].astype(np.float32), out[row])
            self.rst[n] = np.where(on, self.rst[n] + 1.0, self.rst[n])
        return out

    def reset(self, mask=None):
        """``wt_ensemble_alarm_reset``: latched slots whose condition cleared go inactive in the reactors of ``mask``."""
        N = self.p.shape[2]
        mask = np.ones(N, dtype=bool) if mask is None else np.asarray(mask, dtype=bool)
        for s in range(self.p.shape[0]):
            q = self.st[s]
            off = mask & (self.p[s, A_LATCH] == 1) & (q[AS_ACTIVE] == 1) & (q[AS_COND] == 0)
            q[AS_ACTIVE] = np.where(off, 0.0, q[AS_ACTIVE])
            q[AS_PENDING] = np.where(off, np.nan, q[AS_PENDING])
        none = ~(self.st[:, AS_ACTIVE] != 0).any(axis=0)
        self.rst[AR_FIRST_OUT] = np.where(mask & none, -1.0, self.rst[AR_FIRST_OUT])
        self._settle(mask)
