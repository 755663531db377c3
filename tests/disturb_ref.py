"""Host restatement of the per-reactor disturbance programs (include/wtphys.h, csrc/wt_dst.hpp), vectorised over
reactors.

STEP and RAMP offsets and the composed rows have the operands and the order of the device code (numpy fp64 never
contracts into an fma), so they are bit-comparable.  SINE and OU go through different transcendentals: numpy's sin
and exp against the device's own polynomials, and z from the Philox stream of ``oracle/sensor_oracle.py`` with libm
Box-Muller against the device's fp32 hardware one (about 1e-6 absolute on z).  They agree within a tolerance.
"""
import math

import numpy as np

import sensor_oracle as SO

OFF, STEP, RAMP, SINE, OU = range(5)
D_KIND, D_ROW, D_T_START, D_T_END, D_A, D_B, D_C = range(7)
DS_VALUE, DS_X, DS_N_EVAL, DS_N_DRAW = range(4)
SLOTS, NB = 4, 10


def clamp_row(row, v):
    if row == 1:
        return np.fmin(np.fmax(v, 0.0), 14.0)
    if row == 3:
        return np.fmin(np.fmax(v, 0.0), 100.0)
    if row == 8:
        return v
    return np.fmax(v, 0.0)


def normal(seed, reactor, slot, draw):
    """z of the device: Philox4x32-10 on (reactor, slot, draw, 1), key = seed, then Box-Muller (fp64 here)."""
    x = SO.philox4x32_10((reactor & 0xFFFFFFFF, slot, draw & 0xFFFFFFFF, 1), (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF))
    u1 = ((x[0] >> 8) + 1) * (1.0 / 16777216.0)
    u2 = (x[1] >> 8) * (1.0 / 16777216.0)
    return math.sqrt(-2.0 * math.log(u1)) * math.cos(2.0 * math.pi * u2)


class DisturbRef:
    """The program of N reactors.  ``params``: (4, 7, N) block of ``disturbance_block``; ``bc``: (10, N) boundary in
    force at set; ``time``: (N,) ReactorState.time at set.  ``bc`` (the rows) and ``hist`` follow every evaluation."""

    def __init__(self, params, bc, time, seed=0, reactor_base=0, history=0):
        self.p = np.array(params, dtype=np.float64)
        self.N = self.p.shape[2]
        self.base = np.array(bc, dtype=np.float64)
        self.bc = self.base.copy()
        self.st = np.zeros((SLOTS, 4, self.N))
        self.t_prev = np.array(time, dtype=np.float64)
        self.seed, self.reactor_base, self.cap = int(seed), int(reactor_base), int(history)
        self.hist = np.zeros((self.cap, SLOTS, self.N))
        self.evaluate(self.t_prev, np.ones(self.N, dtype=bool))

    def evaluate(self, t, live=None):
        """One evaluation at times t (N,) of the reactors in ``live`` (default: all)."""
        t = np.asarray(t, dtype=np.float64)
        live = np.ones(self.N, dtype=bool) if live is None else np.asarray(live, dtype=bool)
        for r in np.nonzero(live)[0]:
            self._one(int(r), float(t[r]))

    def _one(self, r, t):
        p, s = self.p[:, :, r], self.st[:, :, r]
        h = t - self.t_prev[r]
        self.t_prev[r] = t
        j = int(s[0, DS_N_EVAL])
        for k in range(SLOTS):
            kind, t0, t1, a, b, c = p[k, D_KIND], p[k, D_T_START], p[k, D_T_END], p[k, D_A], p[k, D_B], p[k, D_C]
            inw = t0 <= t < t1
            d, x, nd = 0.0, s[k, DS_X], s[k, DS_N_DRAW]
            if kind == STEP:
                d = a if inw else 0.0
            elif kind == RAMP:
                d = 0.0 if t < t0 else a + b * (min(t, t1) - t0)
            elif kind == SINE:
                d = a * math.sin(2.0 * math.pi * (t - t0) / b + c) if inw else 0.0
            elif kind == OU and inw:
                if h > 0.0:
                    phi = math.exp(-h / b)
                    sc = a * math.sqrt(-math.expm1(-2.0 * h / b))
                    z = normal(self.seed, self.reactor_base + r, k, int(nd))
                    x = x * phi + sc * z
                    nd += 1.0
                d = x
            s[k] = (d, x, j + 1, nd)
            if j < self.cap:
                self.hist[j, k, r] = d
        self.compose(r)

    def compose(self, r=None):
        """The targeted rows from the base and the current offsets (all reactors when r is None)."""
        for rr in (range(self.N) if r is None else (r,)):
            p, s = self.p[:, :, rr], self.st[:, :, rr]
            done = set()
            for k in range(SLOTS):
                if p[k, D_KIND] == OFF or p[k, D_ROW] in done:
                    continue
                row = int(p[k, D_ROW])
                done.add(row)
                v = self.base[row, rr]
                for j in range(k, SLOTS):
                    if p[j, D_KIND] != OFF and p[j, D_ROW] == row:
                        v = v + s[j, DS_VALUE]
                self.bc[row, rr] = clamp_row(row, v)

    def n_filled(self):
        return np.minimum(self.st[0, DS_N_EVAL], self.cap).astype(np.int32)


def compose_rows(params, base, offsets):
    """clamp(base + offsets in slot order) for every targeted row: the boundary block a history entry stands for.
    ``offsets``: (4, N).  Exactly the device's arithmetic, vectorised over reactors."""
    p = np.asarray(params)
    base = np.asarray(base, dtype=np.float64)
    out = base.copy()
    for row in (1, 2, 3, 5, 7, 8, 9):
        v, hit = base[row].copy(), np.zeros(base.shape[1], dtype=bool)
        for k in range(SLOTS):
            m = (p[k, D_KIND] != OFF) & (p[k, D_ROW] == row)
            v = np.where(m, v + offsets[k], v)
            hit |= m
        out[row] = np.where(hit, clamp_row(row, v), base[row])
    return out
