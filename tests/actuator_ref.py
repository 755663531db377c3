"""Host restatement of the per-reactor actuator programs (include/wtphys.h, csrc/wt_act.hpp) together with the
command path they sit behind, vectorised over reactors.

numpy fp64 never contracts a product and a sum into an fma and every operation below has the operands and the order of
the device code, so the channel state, the queues and the boundary rows are bit-comparable with
``ReactorEnsemble.actuator_state()`` and ``boundary()``.
"""
import numpy as np

V_ENABLE, V_TAU, V_RATE, V_BACKLASH, V_DELAY, V_FAULT, V_T_FAULT, V_T_REPAIR, V_FAIL_VALUE = range(9)
VS_POSITION, VS_APPLIED, VS_PLAY, VS_DEMAND, VS_DELIVERED, VS_TRAVEL, VS_N_EXEC, VS_N_RATE, VS_N_FAULT = range(9)
NONE, STUCK, FAIL_TO = range(3)
ACID, CHLORINE, INLET = range(3)
ROWS = (4, 6, 0)
LIMITS = (2.0, 1.0, 20.0)
MAX_DELAY = 8
INLET_MIN = 0.1


def validate(words, limit):
    """validate_flow_rate on float32 commands: NaN -> 0, then clipped to [0, limit], as float64."""
    x = np.asarray(words, dtype=np.float32).astype(np.float64)
    return np.where(np.isnan(x), 0.0, np.fmax(0.0, np.fmin(x, limit)))


class ActuatorRef:
    """State of the program of N reactors and the boundary rows it drives.  ``params``: (3, 9, N) block of
    ``actuator_block``; ``bc``: (10, N) boundary block in force at set; ``loop_time``: (N,) loop time at set."""

    def __init__(self, params, bc, loop_time):
        self.p = np.array(params, dtype=np.float64)
        N = self.p.shape[2]
        self.bc = np.array(bc, dtype=np.float64)
        self.st = np.zeros((3, 9, N))
        self.q = np.zeros((3, MAX_DELAY, N))
        for k in range(3):
            self.st[k, [VS_POSITION, VS_APPLIED, VS_PLAY, VS_DEMAND]] = self.bc[ROWS[k]]
            self.q[k] = self.bc[ROWS[k]]
        self.t_prev = np.array(np.broadcast_to(np.asarray(loop_time, dtype=np.float64), (N,)))

    def scan(self, words, t, stepped=None):
        """One PLC scan: ``words`` the decoded (acid, chlorine, inlet) float32 commands (3, N) after any tamper and
        trip, ``t`` (N,) the loop time the scan stores.  Runs the command path (validation, the reference's inlet
        rule) and then every enabled channel; returns the (inlet, acid, chlorine) commands the next step gets."""
        N = self.p.shape[2]
        stepped = np.ones(N, dtype=bool) if stepped is None else np.asarray(stepped, dtype=bool)
        t = np.broadcast_to(np.asarray(t, dtype=np.float64), (N,))
        w = np.asarray(words, dtype=np.float32)
        acid, chlorine, inlet_v = validate(w[0], 2.0), validate(w[1], 1.0), validate(w[2], 20.0)
        bc = self.bc
        row0 = bc[0].copy()
        bc[4] = np.where(stepped, acid, bc[4])
        bc[6] = np.where(stepped, chlorine, bc[6])
        bc[0] = np.where(stepped & (inlet_v > INLET_MIN), inlet_v, bc[0])
        h = t - self.t_prev
        self.t_prev = np.where(stepped, t, self.t_prev)
        idx = np.arange(N)
        for k in range(3):
            p, s, q = self.p[k], self.st[k], self.q[k]
            on = stepped & (p[V_ENABLE] != 0)
            if k == ACID:
                u = acid
            elif k == CHLORINE:
                u = chlorine
            else:
                u = np.where(inlet_v > INLET_MIN, inlet_v, s[VS_DEMAND])
            applied = s[VS_APPLIED].copy()
            s[VS_DELIVERED] = np.where(on, s[VS_DELIVERED] + applied * h, s[VS_DELIVERED])
            s[VS_DEMAND] = np.where(on, u, s[VS_DEMAND])
            delay = p[V_DELAY].astype(np.int64)
            ud = np.where(delay == 0, u, q[np.maximum(delay - 1, 0), idx])
            shifted = np.concatenate([u[None], q[:-1]])
            q[:] = np.where(on, shifted, q)
            half = p[V_BACKLASH] * 0.5
            play = np.fmax(ud - half, np.fmin(ud + half, s[VS_PLAY]))
            s[VS_PLAY] = np.where(on, play, s[VS_PLAY])
            pos, tau = s[VS_POSITION].copy(), p[V_TAU]
            with np.errstate(invalid="ignore", divide="ignore"):
                pl = np.where(tau > 0, (tau * pos + h * play) / (tau + h), play)
                lim = p[V_RATE] * h
                d = pl - pos
                pn = np.where(d > lim, pos + lim, np.where(d < -lim, pos - lim, pl))
            s[VS_N_RATE] = np.where(on & (pn != pl), s[VS_N_RATE] + 1.0, s[VS_N_RATE])
            fault = p[V_FAULT]
            hit = on & (fault != NONE) & (p[V_T_FAULT] <= t) & (t < p[V_T_REPAIR])
            pn = np.where(hit, np.where(fault == STUCK, pos, p[V_FAIL_VALUE]), pn)
            s[VS_N_FAULT] = np.where(hit, s[VS_N_FAULT] + 1.0, s[VS_N_FAULT])
            s[VS_TRAVEL] = np.where(on, s[VS_TRAVEL] + np.abs(pn - pos), s[VS_TRAVEL])
            s[VS_POSITION] = np.where(on, pn, s[VS_POSITION])
            s[VS_N_EXEC] = np.where(on, s[VS_N_EXEC] + 1.0, s[VS_N_EXEC])
            a = np.fmin(np.fmax(pn, 0.0), LIMITS[k])
            if k == INLET:
                sig = a > INLET_MIN
                applied = np.where(sig, a, applied)
                row = np.where(sig, a, row0)
            else:
                applied = a
                row = a
            s[VS_APPLIED] = np.where(on, applied, s[VS_APPLIED])
            bc[ROWS[k]] = np.where(on, row, bc[ROWS[k]])
        return bc[[0, 4, 6]].copy()

    def rows(self):
        """Boundary rows 0, 4 and 6 (inlet, acid, chlorine)."""
        return self.bc[[0, 4, 6]].copy()
