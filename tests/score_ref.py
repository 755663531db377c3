"""Host restatement of the per-reactor score programs (include/wtphys.h, csrc/wt_scr.hpp), vectorised over reactors.

Its input is a recorded trajectory (``record(every=1)``: the state, time and status after every outer step) and the
times at set, so it shares nothing with the device code.  Every operation has the operands and the order of the
header's pseudo-code; numpy fp64 never contracts into an fma, and MEAN sums the zones in ascending order, so the
results are bit-comparable.
"""
import numpy as np

OFF, BAND = 0, 1
PH, CHLORINE, TEMPERATURE = 0, 1, 2
ZONE, MIN, MAX, MEAN = 0, 1, 2, 3
P_KIND, P_QUANTITY, P_REDUCE, P_ZONE, P_LO, P_HI, P_T_START, P_T_END = range(8)
(S_N_EVAL, S_TIME, S_INTEGRAL, S_T_LOW, S_T_HIGH, S_AREA_LOW, S_AREA_HIGH, S_V_MIN, S_V_MAX, S_LAST, S_OUT, S_N_EXC,
 S_T_FIRST_OUT, S_RUN, S_RUN_MAX) = range(15)
SLOTS, NSS = 4, 15
ST_T_RANGE_POST = 32


def fan_bin(v, lo, hi, scale, bins):
    """The fan's bin of every v (array): 0 below lo, bins + 1 at or above hi."""
    v = np.asarray(v, dtype=np.float64)
    inner = 1 + np.minimum(bins - 1, ((v - lo) * scale).astype(np.int64))
    return np.where(v < lo, 0, np.where(v >= hi, bins + 1, inner))


def reduce_zones(x, red, zone):
    """v of every reactor: x (N, n), red and zone (N,)."""
    N, n = x.shape
    zi = np.where(zone < 0, n - 1, zone).astype(np.int64)
    v_zone = x[np.arange(N), np.minimum(zi, n - 1)]
    v_min, v_max, v_sum = x[:, 0].copy(), x[:, 0].copy(), x[:, 0].copy()
    for z in range(1, n):
        v_min = np.where(x[:, z] < v_min, x[:, z], v_min)
        v_max = np.where(x[:, z] > v_max, x[:, z], v_max)
        v_sum = v_sum + x[:, z]
    return np.where(red == ZONE, v_zone, np.where(red == MIN, v_min, np.where(red == MAX, v_max, v_sum / float(n))))


class ScoreRef:
    """The program of N reactors.  ``params``: (4, 8, N) block of ``score_block``; ``time``: (N,) ReactorState.time at
    set.  ``st`` (4, 15, N), ``t_prev`` (N,), ``counts`` (C, 4, 3) and ``fan`` (C, 4, bins + 2) follow every step."""

    def __init__(self, params, time, curve=0, bins=0, fan_lo=None, fan_hi=None):
        self.p = np.array(params, dtype=np.float64)
        self.N = self.p.shape[2]
        self.cap, self.bins = int(curve), int(bins) if curve > 0 else 0
        if self.bins:
            self.fan_lo = np.broadcast_to(np.asarray(fan_lo, dtype=np.float64), (SLOTS,))
            self.fan_hi = np.broadcast_to(np.asarray(fan_hi, dtype=np.float64), (SLOTS,))
            self.scale = float(self.bins) / (self.fan_hi - self.fan_lo)
        self.reset(time)

    def reset(self, time):
        self.st = np.zeros((SLOTS, NSS, self.N))
        self.st[:, [S_V_MIN, S_V_MAX, S_LAST, S_T_FIRST_OUT]] = np.nan
        self.t_prev = np.array(time, dtype=np.float64)
        self.counts = np.zeros((self.cap, SLOTS, 3), dtype=np.int32)
        self.fan = np.zeros((self.cap, SLOTS, self.bins + 2), dtype=np.int32) if self.bins else None
        self.j = 0

    def step(self, pH, Cl, T, t, stepped):
        """One outer step of the ensemble: state (N, n) and time (N,) after it, ``stepped`` (N,) the reactors that
        took it."""
        stepped = np.asarray(stepped, dtype=bool)
        h = t - self.t_prev
        self.t_prev = np.where(stepped, t, self.t_prev)
        for s in range(SLOTS):
            p, st = self.p[s], self.st[s]
            m = stepped & (p[P_KIND] != OFF) & (p[P_T_START] <= t) & (t < p[P_T_END])
            x = np.where((p[P_QUANTITY] == PH)[:, None], pH, np.where((p[P_QUANTITY] == CHLORINE)[:, None], Cl, T))
            v = reduce_zones(x, p[P_REDUCE], p[P_ZONE])
            lo, hi = p[P_LO], p[P_HI]

            def upd(row, value, where=m):
                st[row] = np.where(where, value, st[row])

            ne = st[S_N_EVAL] + 1.0
            upd(S_N_EVAL, ne)
            upd(S_TIME, st[S_TIME] + h)
            upd(S_INTEGRAL, st[S_INTEGRAL] + v * h)
            upd(S_LAST, v)
            upd(S_V_MIN, np.where(ne == 1.0, v, np.where(v < st[S_V_MIN], v, st[S_V_MIN])))
            upd(S_V_MAX, np.where(ne == 1.0, v, np.where(v > st[S_V_MAX], v, st[S_V_MAX])))
            low, high = m & (v < lo), m & (v > hi)
            with np.errstate(invalid="ignore"):      # (lo - v) with lo = -inf where the side is open: masked out
                upd(S_T_LOW, st[S_T_LOW] + h, low)
                upd(S_AREA_LOW, st[S_AREA_LOW] + (lo - v) * h, low)
                upd(S_T_HIGH, st[S_T_HIGH] + h, high)
                upd(S_AREA_HIGH, st[S_AREA_HIGH] + (v - hi) * h, high)
            out, ok = low | high, m & ~(low | high)
            upd(S_N_EXC, st[S_N_EXC] + 1.0, out & (st[S_OUT] == 0.0))
            upd(S_T_FIRST_OUT, t, out & np.isnan(st[S_T_FIRST_OUT]))
            upd(S_OUT, 1.0, out)
            run = st[S_RUN] + h
            upd(S_RUN, run, out)
            upd(S_RUN_MAX, np.where(run > st[S_RUN_MAX], run, st[S_RUN_MAX]), out)
            upd(S_OUT, 0.0, ok)
            upd(S_RUN, 0.0, ok)
            if self.j < self.cap:
                self.counts[self.j, s] += np.array([m.sum(), low.sum(), high.sum()], dtype=np.int32)
                if self.bins:
                    b = fan_bin(v[m], self.fan_lo[s], self.fan_hi[s], self.scale[s], self.bins)
                    self.fan[self.j, s] += np.bincount(b, minlength=self.bins + 2).astype(np.int32)
        self.j += 1

    def run(self, pH, Cl, T, time, status, time0=None):
        """A whole trajectory: pH, Cl, T (K, N, n), time and status (K, N).  A reactor took step k when its time moved
        and the step left no ReactorState failure (WT_ST_T_RANGE_POST)."""
        prev = self.t_prev.copy() if time0 is None else np.asarray(time0, dtype=np.float64)
        for k in range(time.shape[0]):
            stepped = (time[k] != prev) & ((status[k] & ST_T_RANGE_POST) == 0)
            self.step(pH[k], Cl[k], T[k], time[k], stepped)
            prev = time[k]
        return self
