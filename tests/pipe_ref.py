"""Host restatement of the pipe program (include/wtphys.h ``wt_ensemble_pipe_*``, csrc/wt_trn.hpp): the train program's
host loop (train_ref.py) with a FIFO of D samples per link between ``state`` and ``set_boundary``, and the state and the
lines the program keeps.  The loop is the definition; the fused call must give its bits."""
from collections import deque

import numpy as np

from train_ref import ROWS, TrainRef

NAN = float("nan")


def sample(es, u, stamp=None):
    """(pH, Cl, T of the outlet zone of reactor ``u``, its time or ``stamp``) in the state ``es``."""
    return (float(es.pH[u, -1]), float(es.chlorine[u, -1]), float(es.temperature[u, -1]),
            float(es.time[u]) if stamp is None else stamp)


class PipeRef:
    """The lines, n_sent / t_sent of the pipe program, and the train program's n_fed / t_last under it (``train``)."""

    def __init__(self, N, length, delay, link=None, rows=None):
        self.train = TrainRef(N, length, link, rows)
        self.N, self.link, self.rows = N, self.train.link, self.train.rows
        self.delay = np.broadcast_to(np.asarray(delay), (N,)).astype(np.int64).copy()
        self.delay[self.link != 1.0] = 0                  # a stage that is not linked (a first stage too) has no pipe
        self.q = [deque() for _ in range(N)]
        self.n_sent = np.zeros(N)
        self.t_sent = np.full(N, NAN)

    def fill(self, es):
        """Every line holds D copies of its upstream's outlet in ``es``, time stamp NaN; the pipe state starts over."""
        for d in range(self.N):
            self.q[d] = deque([sample(es, d - 1, NAN)] * int(self.delay[d]))
        self.n_sent[:] = 0.0
        self.t_sent[:] = NAN

    def deliver(self, bc, d, s):
        for bit, row, _ in ROWS:
            if self.rows[d] & bit:
                bc[row, d] = s[row - 1]

    def feed(self, bc, es, fed):
        """The feeds of one outer step that ended in ``es``, for the reactors in ``fed`` (``TrainRef.after_step``): the
        current sample goes into the line, the oldest comes out and is written into ``bc`` (10, N) as the rows mask
        says; a link with no line delivers the current sample.  In place."""
        for d in np.nonzero(fed)[0]:
            s = sample(es, d - 1)
            if self.delay[d] > 0:
                self.q[d].append(s)
                s = self.q[d].popleft()
                self.n_sent[d] += 1.0
                self.t_sent[d] = s[3]
            self.deliver(bc, d, s)
        return bc

    def lines(self):
        """(Dmax, 4, N): the samples in flight, oldest first, NaN beyond a line's own D."""
        out = np.full((int(self.delay.max(initial=0)), 4, self.N), NAN)
        for d, q in enumerate(self.q):
            for i, s in enumerate(q):
                out[i, :, d] = s
        return out

    def state(self):
        """What the comparison with the device takes: n_fed, t_last, n_sent, t_sent, lines."""
        return self.train.n_fed, self.train.t_last, self.n_sent, self.t_sent, self.lines()


def host_piped_loop(ens, K, length, delay, link=None, rows=None, dt=10.0, base=None, before_call=None, after_call=None):
    """``host_fed_loop`` of train_ref.py with a ``collections.deque`` per link.  K one-step calls on a handle WITHOUT a
    train program.  First every line is filled from the current state and every link is delivered from it (what the
    set calls do); after every call: ``state`` -> the sample of every fed link through its line -> rows 1..3 ->
    ``set_boundary``.  ``base``, ``before_call`` and ``after_call`` as in ``host_fed_loop``.  Returns the PipeRef."""
    ref = PipeRef(ens.n_reactors, length, delay, link, rows)
    blk = np.array(ens.boundary() if base is None else base, dtype=np.float64)
    es = ens.state
    ref.fill(es)
    for d in np.nonzero(ref.link == 1.0)[0]:
        ref.deliver(blk, d, sample(es, d - 1))
    ens.set_boundary(blk)
    for k in range(K):
        if before_call is not None:
            before_call(k)
        t0 = es.time
        es = ens.step(dt, n_steps=1)
        blk[[0, 4, 6]] = ens.boundary()[[0, 4, 6]]
        ref.feed(blk, es, ref.train.after_step(t0, es))
        ens.set_boundary(blk)
        if after_call is not None:
            after_call(k, es)
    return ref
