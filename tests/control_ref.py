"""Host restatement of the per-reactor PI programs (include/wtphys.h, csrc/wt_ctl.hpp), vectorised over reactors.

numpy fp64 never contracts a product and a sum into an fma, and every expression below has the association the device
code has, so the results are bit-comparable with ``ReactorEnsemble.control_state()``.
"""
import numpy as np

C_ENABLE, C_SENSOR, C_DIRECTION, C_SETPOINT, C_KP, C_KI, C_BIAS, C_OUT_MIN, C_OUT_MAX = range(9)
CS_INTEGRAL, CS_OUTPUT, CS_ISE, CS_IAE, CS_DOSE, CS_N_EXEC, CS_N_HELD, CS_N_SAT = range(8)
HOLDING_WORD = (2, 0)      # loop 0 chlorine -> holding words 2-3, loop 1 acid -> words 0-1


def float32_words(y):
    """float32(y), rounded to nearest even, as (high, low) uint16 words: (..., 2)."""
    b = np.asarray(y, dtype=np.float64).astype(np.float32).view(np.uint32)
    return np.stack([(b >> 16).astype(np.uint16), (b & 0xFFFF).astype(np.uint16)], axis=-1)


class ControlRef:
    """State of both loops of N reactors.  ``params``: (2, 9, N) block; ``loop_time``: (N,) loop time at enable."""

    def __init__(self, params, loop_time, holding=None):
        self.p = np.array(params, dtype=np.float64)
        N = self.p.shape[2]
        self.st = np.zeros((2, 8, N))
        self.t_prev = np.array(loop_time, dtype=np.float64)
        self.holding = np.zeros((N, 6), dtype=np.uint16) if holding is None else np.array(holding, dtype=np.uint16)
        self._start(self.p[:, C_ENABLE] == 1)

    def _start(self, mask):
        """Loops in ``mask`` (2, N) start: integral 0, output = clamped bias, metrics 0, words written."""
        for l in range(2):
            m = mask[l]
            y0 = np.fmin(np.fmax(self.p[l, C_BIAS], self.p[l, C_OUT_MIN]), self.p[l, C_OUT_MAX])
            self.st[l][:, m] = 0.0
            self.st[l, CS_OUTPUT, m] = y0[m]
            w = HOLDING_WORD[l]
            self.holding[m, w:w + 2] = float32_words(y0[m])

    def retune(self, params):
        new = np.array(params, dtype=np.float64)
        switched_on = (new[:, C_ENABLE] == 1) & (self.p[:, C_ENABLE] != 1)
        self.p = new
        self._start(switched_on)

    def scan(self, values, faults, t_now, stepped=None, skip=None):
        """One PLC scan: ``values`` float32 (7, N) raw readings, ``faults`` (7, N), ``t_now`` (N,) the loop time the
        scan stores, ``stepped`` (N,) reactors that took the step (default: all).  ``skip`` (2, N) bool: loops a tune
        program owns in this scan (``pi_execute``'s ``owned``): no state change and no holding word for them;
        ``t_prev`` advances all the same."""
        N = self.p.shape[2]
        stepped = np.ones(N, dtype=bool) if stepped is None else np.asarray(stepped, dtype=bool)
        t_now = np.asarray(t_now, dtype=np.float64)
        h = t_now - self.t_prev
        self.t_prev = np.where(stepped, t_now, self.t_prev)
        idx = np.arange(N)
        for l in range(2):
            p, q = self.p[l], self.st[l]
            on = stepped & (p[C_ENABLE] == 1)
            if skip is not None:
                on &= ~np.asarray(skip, dtype=bool)[l]
            s = p[C_SENSOR].astype(np.int64)
            v = np.asarray(values, dtype=np.float32)[s, idx]
            f = np.asarray(faults)[s, idx]
            held = on & (~np.isfinite(v) | (f != 0))
            ex = on & ~held
            q[CS_N_HELD] = np.where(held, q[CS_N_HELD] + 1.0, q[CS_N_HELD])
            with np.errstate(invalid="ignore", over="ignore"):
                e = p[C_DIRECTION] * (p[C_SETPOINT] - v.astype(np.float64))
                integral = q[CS_INTEGRAL]
                Ic = integral + (p[C_KI] * e) * h
                u = (p[C_BIAS] + p[C_KP] * e) + Ic
                wind = ((u > p[C_OUT_MAX]) & (e > 0)) | ((u < p[C_OUT_MIN]) & (e < 0))
                Ic = np.where(wind, integral, Ic)
                u = np.where(wind, (p[C_BIAS] + p[C_KP] * e) + integral, u)
                y = np.fmin(np.fmax(u, p[C_OUT_MIN]), p[C_OUT_MAX])
                upd = {CS_INTEGRAL: Ic, CS_OUTPUT: y, CS_ISE: q[CS_ISE] + (e * e) * h, CS_IAE: q[CS_IAE] + np.abs(e) * h,
                       CS_DOSE: q[CS_DOSE] + y * h, CS_N_EXEC: q[CS_N_EXEC] + 1.0,
                       CS_N_SAT: q[CS_N_SAT] + (y != u).astype(np.float64)}
            for k, val in upd.items():
                q[k] = np.where(ex, val, q[k])
            w = HOLDING_WORD[l]
            self.holding[ex, w:w + 2] = float32_words(y[ex])
