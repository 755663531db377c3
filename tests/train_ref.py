"""Host restatement of the train program (include/wtphys.h ``wt_ensemble_train_*``, csrc/wt_trn.hpp): the loop of
one-step calls with a host copy of outlets into ``set_boundary`` between them that the fused call replaces, and the
state the program keeps.  The loop is the definition; the fused call must give its bits."""
import numpy as np

ST_T_RANGE_POST = 32
ROWS = ((1, 1, "pH"), (2, 2, "chlorine"), (4, 3, "temperature"))     # (mask bit, boundary row, state field)


def params(N, length, link=None, rows=None):
    """(link, rows) as (N,) arrays: by default every stage after the first linked with rows 7; first stages never."""
    link = np.broadcast_to(np.asarray(1.0 if link is None else link, dtype=np.float64), (N,)).copy()
    rows = np.broadcast_to(np.asarray(7 if rows is None else rows), (N,)).astype(np.int64)
    link[::length] = 0.0
    return link, rows


def feed_rows(bc, es, link, rows, fed):
    """Rows 1..3 of the boundary block ``bc`` (10, N) of every linked reactor in ``fed`` from zone n - 1 of its
    upstream (reactor r - 1) in the state ``es``; the rows mask limits which.  In place."""
    for d in np.nonzero((link == 1.0) & fed)[0]:
        for bit, row, field in ROWS:
            if rows[d] & bit:
                bc[row, d] = getattr(es, field)[d - 1, -1]
    return bc


class TrainRef:
    """n_fed / t_last of the program, and which reactors an outer step feeds."""

    def __init__(self, N, length, link=None, rows=None):
        self.N, self.length = N, length
        self.link, self.rows = params(N, length, link, rows)
        self.n_fed = np.zeros(N)
        self.t_last = np.full(N, np.nan)

    def after_step(self, time_before, es):
        """(N,) bool: the reactors fed by the outer step that led from ``time_before`` to the state ``es`` -- linked,
        and the upstream stepped and did not end T_RANGE_POST (the sensor suite's test).  Counts them."""
        live = (es.time != time_before) & ((es.status & ST_T_RANGE_POST) == 0)
        fed = np.zeros(self.N, dtype=bool)
        fed[1:] = live[:-1]
        fed &= self.link == 1.0
        self.n_fed[fed] += 1.0
        self.t_last[fed] = es.time[np.nonzero(fed)[0] - 1]
        return fed


def host_fed_loop(ens, K, length, link=None, rows=None, dt=10.0, base=None, before_call=None, after_call=None):
    """K one-step calls on a handle WITHOUT a train program.  First every link is fed from the current state (what the
    set call does); after every call: ``state`` -> rows 1..3 of the fed reactors from their upstream's zone n - 1 ->
    ``set_boundary``.  The block handed to ``set_boundary`` is ``base`` (default: ``boundary()`` before the loop) with
    the fed rows, and rows 0 / 4 / 6 as the device's ``boundary()`` holds them (the command path's rows under plant
    I/O; a disturbance program recomposes its own rows from the block it is given, so it must get its base back, not
    ``boundary()``).  ``before_call(k)`` / ``after_call(k, es)``: the caller's master writes and scans.
    Returns the TrainRef with the expected n_fed / t_last."""
    ref = TrainRef(ens.n_reactors, length, link, rows)
    blk = np.array(ens.boundary() if base is None else base, dtype=np.float64)
    es = ens.state
    feed_rows(blk, es, ref.link, ref.rows, np.ones(ref.N, dtype=bool))
    ens.set_boundary(blk)
    for k in range(K):
        if before_call is not None:
            before_call(k)
        t0 = es.time
        es = ens.step(dt, n_steps=1)
        blk[[0, 4, 6]] = ens.boundary()[[0, 4, 6]]
        feed_rows(blk, es, ref.link, ref.rows, ref.after_step(t0, es))
        ens.set_boundary(blk)
        if after_call is not None:
            after_call(k, es)
    return ref
