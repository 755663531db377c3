"""Host restatement of the junction program (include/wtphys.h ``wt_ensemble_junction_*``, csrc/wt_trn.hpp) in numpy:
the blend, the feeds outside a step, the feed after an outer step with its counters and lines, and the train program's
host loop (train_ref.py, pipe_ref.py) with that blend between ``state`` and ``set_boundary``.  The loop is the
definition: the fused call must give its bits in chlorine, temperature, flows, counters and stamps, and a blended pH
within ``PH_TOL`` (the two sides use different exp10 / log10: each errs by about 8 eps / ln 10 from the H+ sum plus
2 ulp(14) from the logarithm, 4.4e-15; two sides 8.8e-15; the bound is about twice that)."""
from collections import deque

import numpy as np

from train_ref import ROWS, ST_T_RANGE_POST, params

NAN = float("nan")
SLOTS = 4
PH_TOL = 2e-14


def program(N, length, junctions):
    """(stage (4, N), share (4, N), carry (N,)) from ``junctions``: a list of (to_stage, from_stages, shares, carry,
    trains) with ``shares`` a scalar, one per source, or (sources, trains) and ``trains`` an index selection or None."""
    stage, share, carry = np.full((SLOTS, N), -1.0), np.zeros((SLOTS, N)), np.zeros(N)
    first = np.arange(0, N, length)
    for to, src, shares, c, trains in junctions:
        at = np.atleast_1d(first if trains is None else first[np.asarray(trains)]) + to
        sh = np.broadcast_to(np.asarray(shares, dtype=np.float64).T, (at.size, len(src))).T
        stage[:, at], share[:, at] = -1.0, 0.0
        for k, g in enumerate(src):
            stage[k, at], share[k, at] = float(g), sh[k]
        carry[at] = 1.0 if c else 0.0
    return stage, share, carry


def blend(pH, Cl, T, Q):
    """The sample (pH, Cl, T) and Qs of sources with outlet values ``pH``, ``Cl``, ``T`` and flows ``Q`` (sequences in
    slot order): every product and every sum rounded, sums from 0.0 in slot order, IEEE division, then the clamps."""
    Qs = aH = aCl = aT = 0.0
    for p, c, t, q in zip(pH, Cl, T, Q):
        p, c, t, q = float(p), float(c), float(t), float(q)
        Qs = Qs + q
        aH = aH + q * float(np.power(10.0, -p))
        aCl = aCl + q * c
        aT = aT + q * t
    if len(Q) == 1:
        return (float(pH[0]), float(Cl[0]), float(T[0])), Qs
    with np.errstate(all="ignore"):
        H, c, t = np.float64(aH) / np.float64(Qs), np.float64(aCl) / np.float64(Qs), np.float64(aT) / np.float64(Qs)
        p = -np.log10(H)
    return (float(min(max(p, 0.0), 14.0)), float(max(c, 0.0)), float(min(max(t, 0.0), 100.0))), Qs


class JunctionRef:
    """The junction program over a train program (``link``, ``rows``) and, with ``delay``, a pipe program: who feeds
    whom, n_fed / t_last, n_blend / n_held / q_last, n_sent / t_sent and the lines."""

    def __init__(self, N, length, stage, share, carry, link=None, rows=None, delay=None):
        self.N, self.length = N, length
        self.link, self.rows = params(N, length, link, rows)
        self.stage, self.share, self.carry = np.asarray(stage), np.asarray(share), np.asarray(carry)
        self.delay = np.zeros(N, dtype=np.int64) if delay is None else np.broadcast_to(np.asarray(delay), (N,)).astype(np.int64).copy()
        self.delay[self.link != 1.0] = 0
        self.q = [deque() for _ in range(N)]
        self.n_fed, self.t_last = np.zeros(N), np.full(N, NAN)
        self.n_blend, self.n_held, self.q_last = np.zeros(N), np.zeros(N), np.full(N, NAN)
        self.n_sent, self.t_sent = np.zeros(N), np.full(N, NAN)

    def sources(self, d):
        """[(reactor, share)] of junction ``d`` in slot order; empty: ``d`` is no junction."""
        if self.link[d] != 1.0:
            return []
        first = d - d % self.length
        return [(first + int(self.stage[k, d]), float(self.share[k, d])) for k in range(SLOTS) if self.stage[k, d] >= 0.0]

    def sample(self, d, es, row0):
        """((pH, Cl, T, stamp), Qs, source reactors) of linked reactor ``d`` from the state ``es`` and the flows ``row0``
        (N,); a plain link: its upstream's outlet, Qs None."""
        src = self.sources(d)
        if not src:
            u = d - 1
            return (float(es.pH[u, -1]), float(es.chlorine[u, -1]), float(es.temperature[u, -1]), float(es.time[u])), None, [u]
        us = [u for u, _ in src]
        s, Qs = blend([es.pH[u, -1] for u in us], [es.chlorine[u, -1] for u in us], [es.temperature[u, -1] for u in us],
                      [f * float(row0[u]) for u, f in src])
        return s + (float(es.time[us[0]]),), Qs, us

    def deliver(self, bc, d, s):
        for bit, row, _ in ROWS:
            if self.rows[d] & bit:
                bc[row, d] = s[row - 1]

    def fill(self, es, row0):
        """``wt_ensemble_pipe_set``: every line full of the sample from memory (Qs = 0: of slot 0's outlet), stamp NaN."""
        for d in np.nonzero(self.link == 1.0)[0]:
            s, Qs, us = self.sample(d, es, row0)
            if Qs is not None and not Qs > 0.0:
                u = us[0]
                s = (float(es.pH[u, -1]), float(es.chlorine[u, -1]), float(es.temperature[u, -1]), NAN)
            self.q[d] = deque([s[:3] + (NAN,)] * int(self.delay[d]))
        self.n_sent[:] = 0.0
        self.t_sent[:] = NAN

    def feed_outside(self, bc, es, last=None):
        """A feed outside a step into ``bc`` (10, N), in place: every blend from ``es`` and row 0 of ``bc`` as it stands
        before any store; Qs <= 0 leaves a junction as it is; a link with a line gets ``last[d]`` (the sample its line
        last delivered) where that is given.  Not counted."""
        row0 = bc[0].copy()
        for d in np.nonzero(self.link == 1.0)[0]:
            s, Qs, _ = self.sample(d, es, row0)
            if Qs is not None:
                if not Qs > 0.0:
                    continue
                if self.carry[d]:
                    bc[0, d] = Qs
            if self.delay[d] > 0 and last is not None:
                s = last[d]
            self.deliver(bc, d, s)
        return bc

    def after_step(self, bc, es, time_before, row0):
        """The feeds of the outer step that led from ``time_before`` to ``es`` under the flows ``row0`` (N,), into ``bc``
        in place, with the counters.  Returns the (N,) bool of the reactors fed."""
        live = (es.time != time_before) & ((es.status & ST_T_RANGE_POST) == 0)
        fed = np.zeros(self.N, dtype=bool)
        todo = []
        for d in np.nonzero(self.link == 1.0)[0]:
            s, Qs, us = self.sample(d, es, row0)
            if Qs is None:
                ok = bool(live[us[0]])
            else:
                ok = bool(live[us].all()) and Qs > 0.0
                if ok:
                    self.n_blend[d] += 1.0
                    self.q_last[d] = Qs
                elif live[us].any():
                    self.n_held[d] += 1.0
            if ok:
                todo.append((d, s, Qs))
        for d, s, Qs in todo:                             # every read above precedes every store below
            fed[d] = True
            self.n_fed[d] += 1.0
            self.t_last[d] = s[3]
            if self.delay[d] > 0:
                self.q[d].append(s)
                s = self.q[d].popleft()
                self.n_sent[d] += 1.0
                self.t_sent[d] = s[3]
            self.deliver(bc, d, s)
            if Qs is not None and self.carry[d]:
                bc[0, d] = Qs
        return fed

    def lines(self):
        out = np.full((int(self.delay.max(initial=0)), 4, self.N), NAN)
        for d, q in enumerate(self.q):
            for i, s in enumerate(q):
                out[i, :, d] = s
        return out

    def state(self):
        """n_fed, t_last, n_blend, n_held, q_last."""
        return self.n_fed, self.t_last, self.n_blend, self.n_held, self.q_last


def host_junction_loop(ens, K, ref, dt=10.0, base=None, before_call=None, after_call=None):
    """``host_fed_loop`` of train_ref.py with the blend: K one-step calls on a handle WITHOUT a train program.  First the
    lines are filled and every link and junction is fed from the current state (what the set calls do); before every
    call the row 0 in force is read, after it: ``state`` -> the sample of every fed link and junction, through its
    line -> rows 1..3 and the carried row 0 -> ``set_boundary``.  ``base``, ``before_call``, ``after_call`` as there."""
    blk = np.array(ens.boundary() if base is None else base, dtype=np.float64)
    es = ens.state
    ref.feed_outside(blk, es)                             # junction_set
    if ref.delay.any():                                   # pipe_set: fill, then deliver from memory again
        ref.fill(es, blk[0])
        ref.feed_outside(blk, es, last={d: q[0] for d, q in enumerate(ref.q) if q})
    ens.set_boundary(blk)
    for k in range(K):
        if before_call is not None:
            before_call(k)
        t0, row0 = es.time, ens.boundary()[0]
        es = ens.step(dt, n_steps=1)
        blk[[0, 4, 6]] = ens.boundary()[[0, 4, 6]]
        ref.after_step(blk, es, t0, row0)
        ens.set_boundary(blk)
        if after_call is not None:
            after_call(k, es)
    return ref
