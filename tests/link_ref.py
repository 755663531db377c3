"""Host restatement of the per-reactor link programs (include/wtphys.h, csrc/wt_lnk.hpp), vectorised over reactors,
operation for operation.

Every value a link delivers is a float32 the channel carried (widened to float64 in the ring, which is exact), a NaN or
a checked parameter, and every count is a whole number in float64, so state, rings and deliveries are bit-comparable
with ``ReactorEnsemble.link_state()`` and ``link_ring()``.  The draws are word 0 of the Philox4x32-10 restatement of
``oracle/sensor_oracle.py`` on the counter (reactor_base + r, slot, n_draw, 2); ``philox_word0`` is the same function
over arrays (tests/test_link_cpu.py holds one against the other).

``LinkThenInject`` puts a ``LinkRef`` and an ``InjectRef`` (or None) together as the one object ``HostScan`` takes as
its ``inj``, which makes ``HostScan(..., inj=LinkThenInject(...))`` the host statement of the scan order
wire -> link (readings) -> inject -> pack -> apply commands [link (commands) -> inject -> validate] -> ...
"""
import numpy as np

import sensor_oracle as SO

L_MODE, L_TARGET, L_START, L_END, L_A, L_B, L_TIMEOUT, L_FAIL = range(8)
(LS_N_REC, LS_N_APPLIED, LS_N_FRESH, LS_N_LOST, LS_N_TIMEOUT, LS_N_DRAW, LS_T_FRESH, LS_HELD_VALUE, LS_HELD_FAULT,
 LS_TAPE_END) = range(10)
OFF, DELAY, LOSS, REPLAY = range(4)
SLOTS, DEPTH, NL, NLS = 4, 64, 8, 10
N_SENSORS, CMD_ACID = 7, 7
DRAW_STREAM = 2
_NAN_ROWS = (LS_T_FRESH, LS_HELD_VALUE, LS_TAPE_END)
_M32 = np.uint64(0xFFFFFFFF)


def philox_word0(c0, c1, c2, c3, k0, k1):
    """Word 0 of Philox4x32-10 over arrays of counters (c0..c3) under the key (k0, k1): uint64 arrays below 2^32."""
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) & _M32 for c in np.broadcast_arrays(c0, c1, c2, c3))
    k0, k1 = np.uint64(int(k0) & 0xFFFFFFFF), np.uint64(int(k1) & 0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & _M32, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & _M32
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & _M32, (k1 + np.uint64(0xBB67AE85)) & _M32
    return c0


def uniform(seed, reactor, slot, draw):
    """u of one draw from the scalar restatement the sensor and disturbance tests use: word 0 * 2^-32."""
    x = SO.philox4x32_10((reactor & 0xFFFFFFFF, slot, draw & 0xFFFFFFFF, DRAW_STREAM), (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF))
    return x[0] * (1.0 / 4294967296.0)


def whole(c):
    """A count as an index: whole numbers below 2^32 as they are, anything else (NaN, negative, huge) 0.  int64."""
    c = np.asarray(c, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        ok = (c >= 0.0) & (c < 4294967296.0)
    return np.where(ok, c, 0.0).astype(np.int64)


class LinkRef:
    """State and rings of the four slots of N reactors.  ``params``: (4, 8, N) block of ``link_block``; ``seed``: the
    set call's; ``reactor_base``: the sensor suite's.  ``ring`` / ``fring`` (4, 64, N) are the device's rings as they
    lie in memory; ``in_order()`` gives them as ``link_ring()`` does."""

    def __init__(self, params, seed=0, reactor_base=0):
        self.p = np.array(params, dtype=np.float64)
        self.N = self.p.shape[2]
        self.seed, self.reactor_base = int(seed), int(reactor_base)
        self.reset()

    def reset(self):
        self.st = np.zeros((SLOTS, NLS, self.N))
        self.st[:, _NAN_ROWS] = np.nan
        self.ring = np.zeros((SLOTS, DEPTH, self.N))
        self.fring = np.zeros((SLOTS, DEPTH, self.N), dtype=np.int64)

    def in_order(self):
        """(values, faults, n_rec) as ``ReactorEnsemble.link_ring()``: entry k the k-th oldest sample a ring holds."""
        n = whole(self.st[:, LS_N_REC])                                   # (4, N)
        kept = np.minimum(n, DEPTH)
        k = np.arange(DEPTH)[None, :, None]
        i = (n[:, None, :] - kept[:, None, :] + k) & (DEPTH - 1)
        have = k < kept[:, None, :]
        v = np.where(have, np.take_along_axis(self.ring, i, axis=1), np.nan)
        f = np.where(have, np.take_along_axis(self.fring, i, axis=1), 0).astype(np.float64)
        return v, f, self.st[:, LS_N_REC].copy()

    def _draw(self, s, who):
        """u (N,) for the reactors in ``who``; their n_draw goes up by one."""
        q = self.st[s]
        u = np.zeros(self.N)
        if who.any():
            r = np.nonzero(who)[0]
            w = philox_word0(self.reactor_base + r, s, whole(q[LS_N_DRAW][r]), DRAW_STREAM, self.seed, self.seed >> 32)
            u[r] = w.astype(np.float64) * (1.0 / 4294967296.0)
            q[LS_N_DRAW] = np.where(who, q[LS_N_DRAW] + 1.0, q[LS_N_DRAW])
        return u

    def _slot(self, s, x, f, t, on, command):
        """One scan of slot s on the samples x float32 (N,), f (N,) of the reactors in ``on``: (delivered values float32,
        delivered fault codes)."""
        p, q, ring, fring = self.p[s], self.st[s], self.ring[s], self.fring[s]
        idx = np.arange(self.N)
        mode = p[L_MODE]
        x = np.asarray(x, dtype=np.float32)
        f = np.asarray(f).astype(np.int64)
        xd = x.astype(np.float64)
        nan = np.nan
        with np.errstate(invalid="ignore", over="ignore"):
            inside = on & (mode != OFF) & (p[L_START] <= t) & (t < p[L_END])
            # 1. record
            n_rec = q[LS_N_REC].copy()
            rec = on & ~(inside & (mode == REPLAY))
            i = whole(n_rec) & (DEPTH - 1)
            ring[i[rec], idx[rec]] = xd[rec]
            fring[i[rec], idx[rec]] = f[rec] & 0xFF
            n_rec = np.where(rec, n_rec + 1.0, n_rec)
            q[LS_N_REC] = n_rec
            # 2. outside the window
            out = on & ~inside
            q[LS_HELD_VALUE] = np.where(out, xd, q[LS_HELD_VALUE])
            q[LS_HELD_FAULT] = np.where(out, f.astype(np.float64), q[LS_HELD_FAULT])
            q[LS_T_FRESH] = np.where(out, t, q[LS_T_FRESH])
            q[LS_TAPE_END] = np.where(out, nan, q[LS_TAPE_END])
            # 3. inside
            j = q[LS_N_APPLIED].copy()
            q[LS_N_APPLIED] = np.where(inside, j + 1.0, j)
            y, g, fresh = xd.copy(), f.copy(), inside.copy()
            u = self._draw(s, inside & ((mode == LOSS) | ((mode == DELAY) & (p[L_B] != 0.0))))
            # DELAY
            dl = inside & (mode == DELAY)
            d = np.where(p[L_B] != 0.0, p[L_A] + np.floor(u * (p[L_B] + 1.0)), p[L_A])
            i = whole(np.fmax(n_rec - 1.0 - d, 0.0)) & (DEPTH - 1)
            y, g = np.where(dl, ring[i, idx], y), np.where(dl, fring[i, idx], g)
            # LOSS
            lost = inside & (mode == LOSS) & (u < p[L_A])
            q[LS_N_LOST] += lost
            tf = q[LS_T_FRESH]
            stale = lost & ~np.isnan(tf)
            fresh &= ~stale
            late = stale & (t - tf > p[L_TIMEOUT])
            q[LS_N_TIMEOUT] += late
            hold = stale & ~late
            y, g = np.where(hold, q[LS_HELD_VALUE], y), np.where(hold, whole(q[LS_HELD_FAULT]), g)
            if command:
                y, g = np.where(late, p[L_FAIL].astype(np.float32).astype(np.float64), y), np.where(late, 0, g)
            else:
                y, g = np.where(late, nan, y), np.where(late, whole(p[L_FAIL]), g)
            # REPLAY
            rp = inside & (mode == REPLAY)
            te = q[LS_TAPE_END]
            first = rp & np.isnan(te)
            empty = first & (n_rec == 0.0)
            ring[0, idx[empty]] = xd[empty]
            fring[0, idx[empty]] = f[empty] & 0xFF
            n_rec = np.where(empty, 1.0, n_rec)
            q[LS_N_REC] = n_rec
            te = np.where(first, n_rec, te)
            q[LS_TAPE_END] = te
            length = np.maximum(whole(np.fmin(p[L_A], te)), 1)
            i = (whole(te) - length + whole(j) % length) & (DEPTH - 1)
            y, g = np.where(rp, ring[i, idx], y), np.where(rp, fring[i, idx], g)
            # a fresh delivery
            q[LS_HELD_VALUE] = np.where(fresh, y, q[LS_HELD_VALUE])
            q[LS_HELD_FAULT] = np.where(fresh, g.astype(np.float64), q[LS_HELD_FAULT])
            q[LS_T_FRESH] = np.where(fresh, t, q[LS_T_FRESH])
            q[LS_N_FRESH] += fresh
            y32 = y.astype(np.float32)
        return np.where(on, y32, x), np.where(on, g, f)

    def _run(self, rows, faults, t, command, stepped):
        N = self.N
        t = np.array(np.broadcast_to(np.asarray(t, dtype=np.float64), (N,)))
        stepped = np.ones(N, dtype=bool) if stepped is None else np.asarray(stepped, dtype=bool)
        idx = np.arange(N)
        off = CMD_ACID if command else 0
        for s in range(SLOTS):
            target = self.p[s, L_TARGET]
            on = stepped & ((target >= CMD_ACID) == command)
            if not on.any():
                continue
            row = np.where(on, target, off).astype(np.int64) - off
            f = faults[row, idx] if faults is not None else np.zeros(N, dtype=np.int64)
            y, g = self._slot(s, rows[row, idx], f, t, on, command)
            rows[row[on], idx[on]] = y[on]
            if faults is not None:
                faults[row[on], idx[on]] = g[on]
        return rows

    def sensors(self, values, faults, t, stepped=None):
        """One scan's reading slots on the readings (7, N) float32 and fault codes (7, N): the linked copies."""
        v = np.array(values, dtype=np.float32)
        f = np.array(faults).astype(np.int64)
        self._run(v, f, t, False, stepped)
        return v, f

    def commands(self, commands, t, stepped=None):
        """One scan's command slots on the decoded (acid, chlorine, inlet) float32 commands (3, N): a linked copy."""
        c = np.array(commands, dtype=np.float32)
        return self._run(c, None, t, True, stepped)


class LinkThenInject:
    """A ``LinkRef`` and an ``InjectRef`` (or None) as ``HostScan``'s ``inj``: ``sensors`` and ``commands`` run the
    link, then the injection.  ``p`` carries the mode and target rows of both, so that ``HostScan`` sees command
    tampering whenever either has a command slot; ``st`` is the injection's state (the INJECT trend tag).  ``stepped``:
    the reactors that take the scan where a caller names none (an emulated command path runs in ``holding()``, which
    knows no mask)."""

    def __init__(self, lnk, inj=None, stepped=None):
        self.lnk, self.inj, self.stepped = lnk, inj, stepped
        rows = [lnk.p[:, :2]] + ([] if inj is None else [inj.p[:, :2]])
        self.p = np.concatenate(rows, axis=0)

    @property
    def st(self):
        return np.zeros((SLOTS, 4, self.lnk.N)) if self.inj is None else self.inj.st

    def sensors(self, values, faults, t, stepped=None):
        stepped = self.stepped if stepped is None else stepped
        v, f = self.lnk.sensors(values, faults, t, stepped)
        return (v, f) if self.inj is None else self.inj.sensors(v, f, t, stepped)

    def commands(self, commands, t, stepped=None):
        stepped = self.stepped if stepped is None else stepped
        c = self.lnk.commands(commands, t, stepped)
        return c if self.inj is None else self.inj.commands(c, t, stepped)
