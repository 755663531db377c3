"""Host restatement of the per-reactor injection programs (include/wtphys.h, csrc/wt_inj.hpp), vectorised over
reactors.

numpy fp64 never contracts a product and a sum into an fma, every expression below has the association the device
code has, and the result is rounded once to float32, so the values and the state are bit-comparable with
``ReactorEnsemble.injection_state()``.
"""
import numpy as np

I_MODE, I_TARGET, I_T_START, I_T_END, I_A, I_B = range(6)
IS_N_APPLIED, IS_T_FIRST, IS_T_LAST, IS_HELD = range(4)
OFF, BIAS, GAIN, CONSTANT, RAMP, FREEZE, DROPOUT, FAULT = range(8)
N_SENSORS, CMD_ACID = 7, 7


class InjectRef:
    """State of the program of N reactors.  ``params``: (4, 6, N) block of ``injection_block``."""

    def __init__(self, params):
        self.p = np.array(params, dtype=np.float64)
        S, _, N = self.p.shape
        self.st = np.zeros((S, 4, N))
        self.st[:, IS_T_FIRST:] = np.nan

    def _apply(self, s, x, t, on):
        """Slot s on the float32 values x (N,) of the reactors in ``on``: (new values, fault code or -1)."""
        p, q = self.p[s], self.st[s]
        mode = p[I_MODE]
        xd = np.asarray(x, dtype=np.float32).astype(np.float64)
        first = on & (q[IS_N_APPLIED] == 0)
        q[IS_T_FIRST] = np.where(first, t, q[IS_T_FIRST])
        q[IS_HELD] = np.where(first & (mode == FREEZE), xd, q[IS_HELD])
        q[IS_N_APPLIED] = np.where(on, q[IS_N_APPLIED] + 1.0, q[IS_N_APPLIED])
        q[IS_T_LAST] = np.where(on, t, q[IS_T_LAST])
        a, b = p[I_A], p[I_B]
        with np.errstate(invalid="ignore", over="ignore"):
            y = np.select([mode == BIAS, mode == GAIN, mode == CONSTANT, mode == RAMP, mode == FREEZE, mode == DROPOUT],
                          [xd + a, xd * a, a, xd + (a + b * (t - p[I_T_START])), q[IS_HELD], np.nan], xd)
            y32 = y.astype(np.float32)
        out = np.where(on, y32, np.asarray(x, dtype=np.float32))
        fault = np.where(on & (mode == FAULT), a, -1).astype(np.int64)
        return out, fault

    def _active(self, s, t, command, stepped):
        p = self.p[s]
        return (stepped & (p[I_MODE] != OFF) & ((p[I_TARGET] >= CMD_ACID) == command)
                & (p[I_T_START] <= t) & (t < p[I_T_END]))

    def _run(self, rows, faults, t, command, stepped):
        N = self.p.shape[2]
        t = np.broadcast_to(np.asarray(t, dtype=np.float64), (N,))
        stepped = np.ones(N, dtype=bool) if stepped is None else np.asarray(stepped, dtype=bool)
        idx = np.arange(N)
        off = CMD_ACID if command else 0
        for s in range(self.p.shape[0]):
            on = self._active(s, t, command, stepped)
            if not on.any():
                continue
            row = np.where(on, self.p[s, I_TARGET], off).astype(np.int64) - off
            x = rows[row, idx]
            y, f = self._apply(s, x, t, on)
            rows[row[on], idx[on]] = y[on]
            if faults is not None:
                hit = f >= 0
                faults[row[hit], idx[hit]] = f[hit]
        return rows

    def sensors(self, values, faults, t, stepped=None):
        """One scan's sensor slots on the readings (7, N) float32 and fault codes (7, N): tampered copies."""
        v = np.array(values, dtype=np.float32)
        f = np.array(faults).astype(np.int64)
        self._run(v, f, t, False, stepped)
        return v, f

    def commands(self, commands, t, stepped=None):
        """One scan's command slots on the decoded (acid, chlorine, inlet) float32 commands (3, N): a tampered copy."""
        c = np.array(commands, dtype=np.float32)
        return self._run(c, None, t, True, stepped)
