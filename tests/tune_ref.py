"""Host restatement of the per-reactor relay autotune programs (include/wtphys.h, csrc/wt_tun.hpp), vectorised over
reactors.

numpy fp64 never contracts a product and a sum into an fma, its division and square root are correctly rounded, and
every expression below has the association the device code has, so the results are bit-comparable with
``ReactorEnsemble.tuner_state()``.  ``TuneRef`` is ``HostScan``'s ``tun``: it runs before the PI programs, and the
loops it ``owned`` in a scan are the ones ``ControlRef.scan`` then skips.
"""
import numpy as np

from control_ref import C_BIAS, C_ENABLE, C_KI, C_KP, CS_INTEGRAL, HOLDING_WORD, float32_words

(U_ENABLE, U_SENSOR, U_DIRECTION, U_SETPOINT, U_BIAS, U_AMPLITUDE, U_HYSTERESIS, U_T_START, U_T_MAX, U_SETTLE, U_CYCLES,
 U_KP_FACTOR, U_TI_FACTOR, U_COMMISSION) = range(14)
(US_PHASE, US_RELAY, US_OUTPUT, US_N_UP, US_T_UP, US_E_MAX, US_E_MIN, US_SUM_PERIOD, US_SUM_AMP, US_N_CYCLES, US_PERIOD,
 US_AMPLITUDE, US_KU, US_KP, US_KI, US_T_BEGIN, US_T_DONE, US_N_EXEC, US_N_HELD, US_COMMISSIONED) = range(20)
WAITING, RUNNING, DONE, FAILED = range(4)


class TuneRef:
    """State of both tuners of N reactors.  ``params``: (2, 14, N) block.  ``ctl``: the ``ControlRef`` of the PI
    programs that run beside the tuners, kept for two things only: a tuner commissions its gains into it, and its
    holding words are then the tuners'.  None: then ``holding`` (N, 6) are the words the tuners write into (default:
    all 0, as plant I/O starts).  ``owned`` (2, N): the loops the tuners owned in the last scan."""

    def __init__(self, params, ctl=None, holding=None):
        self.p = np.array(params, dtype=np.float64)
        N = self.p.shape[2]
        self.st = np.zeros((2, 20, N))
        self.ctl = ctl
        if ctl is not None:
            assert holding is None, "with a ControlRef the words are its own"
            self.holding = ctl.holding
        else:
            self.holding = np.zeros((N, 6), dtype=np.uint16) if holding is None else np.array(holding, dtype=np.uint16)
        self.owned = np.zeros((2, N), dtype=bool)      # loops the tuners owned in the last scan

    def reset(self):
        self.st[:] = 0.0

    def scan(self, values, faults, t_now, stepped=None):
        """One PLC scan: ``values`` float32 (7, N) readings as the PI sees them, ``faults`` (7, N), ``t_now`` (N,) the
        loop time the scan stores, ``stepped`` (N,) reactors that took the step (default: all)."""
        N = self.p.shape[2]
        stepped = np.ones(N, dtype=bool) if stepped is None else np.asarray(stepped, dtype=bool)
        t = np.broadcast_to(np.asarray(t_now, dtype=np.float64), (N,))
        idx = np.arange(N)
        for l in range(2):
            p, q = self.p[l], self.st[l]
            bias, d, eps = p[U_BIAS], p[U_AMPLITUDE], p[U_HYSTERESIS]
            on = stepped & (p[U_ENABLE] == 1) & (q[US_PHASE] < DONE)
            start = on & (q[US_PHASE] == WAITING) & (t >= p[U_T_START])
            live = on & ((q[US_PHASE] == RUNNING) | start)
            q[US_PHASE, start] = RUNNING
            q[US_T_BEGIN, start] = t[start]
            q[US_RELAY, start] = 0.0
            q[US_E_MAX, start], q[US_E_MIN, start] = -np.inf, np.inf
            q[US_OUTPUT, start] = bias[start]
            write = start.copy()
            s = p[U_SENSOR].astype(np.int64)
            v = np.asarray(values, dtype=np.float32)[s, idx]
            f = np.asarray(faults)[s, idx]
            bad = ~np.isfinite(v) | (f != 0)
            held, ex = live & bad, live & ~bad
            q[US_N_HELD] += held
            q[US_N_EXEC] += ex
            with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
                e = p[U_DIRECTION] * (p[U_SETPOINT] - v.astype(np.float64))
                relay = np.where(ex & (q[US_RELAY] == 0), np.where(e >= 0, 1.0, -1.0), q[US_RELAY])
                e_max = np.where(ex, np.fmax(q[US_E_MAX], e), q[US_E_MAX])
                e_min = np.where(ex, np.fmin(q[US_E_MIN], e), q[US_E_MIN])
                up = ex & (relay < 0) & (e > eps)
                down = ex & ~up & (relay > 0) & (e < -eps)
                relay = np.where(up, 1.0, np.where(down, -1.0, relay))
                n_up = q[US_N_UP] + up
                counted = up & (n_up >= 2) & (n_up - 1.0 > p[U_SETTLE])
                q[US_SUM_PERIOD] = np.where(counted, q[US_SUM_PERIOD] + (t - q[US_T_UP]), q[US_SUM_PERIOD])
                q[US_SUM_AMP] = np.where(counted, q[US_SUM_AMP] + (e_max - e_min) * 0.5, q[US_SUM_AMP])
                q[US_N_CYCLES] += counted
                q[US_N_UP] = n_up
                q[US_T_UP] = np.where(up, t, q[US_T_UP])
                q[US_E_MAX] = np.where(up, -np.inf, e_max)
                q[US_E_MIN] = np.where(up, np.inf, e_min)
                q[US_RELAY] = relay
                fin = ex & (q[US_N_CYCLES] == p[U_CYCLES])
                period = q[US_SUM_PERIOD] / q[US_N_CYCLES]
                amplitude = q[US_SUM_AMP] / q[US_N_CYCLES]
                arg = amplitude * amplitude - eps * eps
                ok = fin & (arg > 0)
                ku = (4.0 * d) / (3.141592653589793 * np.sqrt(arg))
                kp = p[U_KP_FACTOR] * ku
                ki = np.where(p[U_TI_FACTOR] > 0, kp / (p[U_TI_FACTOR] * period), 0.0)
            q[US_PERIOD] = np.where(fin, period, q[US_PERIOD])
            q[US_AMPLITUDE] = np.where(fin, amplitude, q[US_AMPLITUDE])
            for row, val in ((US_KU, ku), (US_KP, kp), (US_KI, ki)):
                q[row] = np.where(ok, val, q[row])
            q[US_PHASE] = np.where(ok, DONE, np.where(fin, FAILED, q[US_PHASE]))
            q[US_T_DONE] = np.where(fin, t, q[US_T_DONE])
            q[US_OUTPUT] = np.where(fin, bias, np.where(ex, bias + relay * d, q[US_OUTPUT]))
            write |= ex
            if self.ctl is not None:
                c = self.ctl
                com = ok & (p[U_COMMISSION] == 1) & (c.p[l, C_ENABLE] == 1)
                c.p[l, C_KP, com], c.p[l, C_KI, com] = kp[com], ki[com]
                c.st[l, CS_INTEGRAL, com] = (bias - c.p[l, C_BIAS])[com]
                q[US_COMMISSIONED, com] = 1.0
            late = live & (q[US_PHASE] == RUNNING) & (t - q[US_T_BEGIN] >= p[U_T_MAX])
            q[US_PHASE, late] = FAILED
            q[US_T_DONE, late] = t[late]
            q[US_OUTPUT, late] = bias[late]
            write |= late
            w = HOLDING_WORD[l]
            self.holding[write, w:w + 2] = float32_words(q[US_OUTPUT, write])
            self.owned[l] = live
