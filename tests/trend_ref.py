"""Host restatement of the per-reactor trend recorder programs (include/wtphys.h, csrc/wt_trd.hpp), vectorised over
reactors.

The recorder copies values, so the restatement knows nothing about the device: the caller hands every scan's values
in, by tag, and gets the thinning (``every``, the deadband, the window) and the store (drop when full, or wrap) back.
"""
import numpy as np

T_TAG, T_INDEX, T_EVERY, T_DEADBAND, T_T_START, T_T_END = range(6)
TS_N_SEEN, TS_N_RECORDED, TS_N_DROPPED, TS_LAST = range(4)
(OFF, IMAGE_VALUE, IMAGE_FAULT, FIELD_VALUE, FIELD_FAULT, COMMAND, CONTROL, INJECT, ALARM, ALARM_WORD, ACTUATOR,
 DETECT) = range(12)


class TrendRef:
    """State and store of the program of N reactors.  ``params``: (8, 6, N) block of ``trend_block``; ``capacity``:
    samples per slot and reactor; ``wrap``: overwrite the oldest sample of a full store instead of dropping the new one."""

    def __init__(self, params, capacity, wrap=False):
        self.p = np.array(params, dtype=np.float64)
        self.cap, self.wrap = int(capacity), bool(wrap)
        self.reset()

    def reset(self):
        """``wt_ensemble_trend_set`` / ``_reset``."""
        S, _, N = self.p.shape
        self.st = np.zeros((S, 4, N))
        self.st[:, TS_LAST] = np.nan
        self.ring_t = np.full((S, self.cap, N), np.nan)
        self.ring_x = np.full((S, self.cap, N), np.nan)

    def scan(self, values, t, stepped=None):
        """One PLC scan.  ``values``: a dict tag code -> (entries, N) array of that tag's values at this scan, row =
        ``index`` (an (N,) array serves a tag with one entry), or a callable ``values(tag)`` that returns one; a tag that
        is missing (the callable returns None) reads NaN, as a program that is off does.  ``t`` (N,): the loop time the
        scan stores; ``stepped`` (N,): reactors that took the step (default: all)."""
        S, _, N = self.p.shape
        stepped = np.ones(N, dtype=bool) if stepped is None else np.asarray(stepped, dtype=bool)
        t = np.array(np.broadcast_to(np.asarray(t, dtype=np.float64), (N,)))
        get = values if callable(values) else values.get
        idx = np.arange(N)
        for s in range(S):
            p, q = self.p[s], self.st[s]
            tag = p[T_TAG].astype(np.int64)
            on = stepped & (tag != OFF) & ~(t < p[T_T_START]) & ~(t >= p[T_T_END])
            if not on.any():
                continue
            q[TS_N_SEEN] = np.where(on, q[TS_N_SEEN] + 1.0, q[TS_N_SEEN])
            every = np.where(tag != OFF, p[T_EVERY], 1.0)
            cand = on & (np.fmod(q[TS_N_SEEN] - 1.0, every) == 0.0)
            x = np.full(N, np.nan)
            for g in np.unique(tag[cand]):
                v = get(int(g))
                if v is None:
                    continue
                v = np.asarray(v, dtype=np.float64)
                v = v[None] if v.ndim == 1 else v
                m = cand & (tag == g)
                x[m] = v[p[T_INDEX].astype(np.int64)[m], idx[m]]
            last, db = q[TS_LAST], p[T_DEADBAND]
            with np.errstate(invalid="ignore"):
                changed = (~np.isnan(x) | ~np.isnan(last)) & ~(np.abs(x - last) <= db)
            take = cand & ((q[TS_N_RECORDED] == 0.0) | (db < 0.0) | changed)
            full = take & (q[TS_N_RECORDED] >= self.cap) & (not self.wrap)
            store = take & ~full
            pos = np.fmod(q[TS_N_RECORDED], float(self.cap)).astype(np.int64)
            self.ring_t[s, pos[store], idx[store]] = t[store]
            self.ring_x[s, pos[store], idx[store]] = x[store]
            q[TS_N_DROPPED] = np.where(full, q[TS_N_DROPPED] + 1.0, q[TS_N_DROPPED])
            q[TS_N_RECORDED] = np.where(store, q[TS_N_RECORDED] + 1.0, q[TS_N_RECORDED])
            q[TS_LAST] = np.where(take, x, last)

    def data(self):
        """What ``wt_ensemble_trend_data`` returns: (time, value) (8, capacity, N) with every slot's samples oldest first
        and NaN past the samples held, and the number held (8, N)."""
        S, _, N = self.p.shape
        n_rec = self.st[:, TS_N_RECORDED].astype(np.int64)
        count = np.minimum(n_rec, self.cap)
        first = np.where(n_rec > self.cap, n_rec % self.cap, 0)
        k = np.arange(self.cap)[None, :, None]
        src = (first[:, None, :] + k) % self.cap
        held = k < count[:, None, :]
        time = np.where(held, np.take_along_axis(self.ring_t, src, axis=1), np.nan)
        value = np.where(held, np.take_along_axis(self.ring_x, src, axis=1), np.nan)
        return time, value, count
