"""Host restatement of the per-reactor model predictive controllers (include/wtphys.h, csrc/wt_mpc.hpp), vectorised over
reactors, operation for operation.

numpy fp64 never contracts a product and a sum into an fma, every expression below has the association the device code
has, and the dot product is summed as the device sums it -- a balanced tree, ``x = x[:h] + x[h:]`` -- so the results are
bit-comparable with ``ReactorEnsemble.mpc_state()`` and ``mpc_prediction()``.  ``MpcRef`` runs after the tuners and
before the PI programs; ``LoopOwners`` puts a ``TuneRef`` and an ``MpcRef`` together as the one object ``HostScan``
takes as its ``tun``, which makes ``HostScan(..., tun=LoopOwners(...))`` the host statement of the scan order
... -> loop time -> tune -> mpc -> PI -> alarm -> ...
"""
import numpy as np

from control_ref import HOLDING_WORD, float32_words

M_ENABLE, M_SENSOR, M_SETPOINT, M_EVERY, M_HORIZON, M_U0, M_OUT_MIN, M_OUT_MAX, M_DU_MAX, M_T_START = range(10)
(MS_PHASE, MS_OUTPUT, MS_COUNT, MS_BIAS, MS_MOVE, MS_T_EXEC, MS_ISE, MS_IAE, MS_DOSE, MS_N_EXEC, MS_N_HELD, MS_N_SAT,
 MS_N_RATE, MS_N_SKIPPED) = range(14)
WAITING, RUNNING = range(2)
H = 64
_UP = np.minimum(np.arange(H) + 1, H - 1)


def tree_sum(x):
    """The balanced-tree sum over axis 0 of a (64, ...) array: for half = 32 ... 1, element i takes x[i] + x[i + half]."""
    x = np.asarray(x, dtype=np.float64)
    while len(x) > 1:
        h = len(x) // 2
        x = x[:h] + x[h:]
    return x[0]


def sequential_sum(x):
    """The same terms added left to right: what a controller kept in one lane would compute."""
    x = np.asarray(x, dtype=np.float64)
    s = x[0].copy()
    for i in range(1, len(x)):
        s = s + x[i]
    return s


def order_gains():
    """(64,) gains of the p = 64 controllers in the fused-against-host test: a DMC gain row's shape, spread over three
    decades so that the order of the additions shows in the last bits of the sum (tests/test_mpc_cpu.py asserts it)."""
    i = np.arange(H, dtype=np.float64)
    return 0.02 * np.exp(-i / 9.0) * (1.0 + 0.5 * np.sin(1.7 * i + 0.3))


class MpcRef:
    """State of both controllers of N reactors.  ``params`` (2, 10, N), ``step`` and ``gain`` (2, 64, N) blocks.
    ``words``: an object whose ``holding`` (N, 6) words the controllers write into, in place (a ``ControlRef`` or a
    ``TuneRef`` that runs beside them); None: words of their own, all 0 as plant I/O starts.  ``owned`` (2, N): the loops
    the controllers owned in the last scan.  ``total``: how the 64 terms are added (the device: ``tree_sum``)."""

    def __init__(self, params, step, gain, words=None, total=tree_sum):
        self.p = np.array(params, dtype=np.float64)
        self.step, self.gain = np.array(step, dtype=np.float64), np.array(gain, dtype=np.float64)
        N = self.p.shape[2]
        self.st = np.zeros((2, 14, N))
        self.pred = np.zeros((2, H, N))
        self.holding = np.zeros((N, 6), dtype=np.uint16) if words is None else words.holding
        self.owned = np.zeros((2, N), dtype=bool)
        self.total = total

    def reset(self):
        self.st[:] = 0.0
        self.pred[:] = 0.0

    def scan(self, values, faults, t_now, stepped=None, skip=None):
        """One PLC scan: ``values`` float32 (7, N) readings as the PI sees them, ``faults`` (7, N), ``t_now`` (N,) the
        loop time the scan stores, ``stepped`` (N,) reactors that took the step (default: all), ``skip`` (2, N) the loops
        the tuners owned in this scan (default: none)."""
        N = self.p.shape[2]
        stepped = np.ones(N, dtype=bool) if stepped is None else np.asarray(stepped, dtype=bool)
        skip = np.zeros((2, N), dtype=bool) if skip is None else np.asarray(skip, dtype=bool)
        t = np.broadcast_to(np.asarray(t_now, dtype=np.float64), (N,))
        idx = np.arange(N)
        lanes = np.arange(H)[:, None]
        for l in range(2):
            p, q, P = self.p[l], self.st[l], self.pred[l]
            on = stepped & (p[M_ENABLE] == 1) & (t >= p[M_T_START])
            skipped = on & skip[l]
            q[MS_N_SKIPPED] += skipped
            own = on & ~skipped
            running = q[MS_PHASE] == RUNNING
            due = own & (q[MS_COUNT] == 0)
            s_ix = p[M_SENSOR].astype(np.int64)
            v = np.asarray(values, dtype=np.float32)[s_ix, idx]
            f = np.asarray(faults)[s_ix, idx]
            bad = ~np.isfinite(v) | (f != 0)
            held, ex = due & bad, due & ~bad
            q[MS_N_HELD] += held
            shift = held & running
            P[:, shift] = P[_UP][:, shift]
            start = ex & ~running
            vd = v.astype(np.float64)
            lo, hi, sp = p[M_OUT_MIN], p[M_OUT_MAX], p[M_SETPOINT]
            with np.errstate(invalid="ignore", over="ignore"):
                P[:, start] = vd[start]                                              # 1.
                output = np.where(start, np.fmin(np.fmax(p[M_U0], lo), hi), q[MS_OUTPUT])
                d = vd - P[0]                                                        # 2.
                s = P[_UP]                                                           # 3.
                term = np.where(lanes < p[M_HORIZON], self.gain[l] * ((sp - s) - d), 0.0)   # 4.
                du = self.total(term)                                                # 5.
                dc = np.fmin(np.fmax(du, -p[M_DU_MAX]), p[M_DU_MAX])                 # 6.
                u = output + dc                                                      # 7.
                y = np.fmin(np.fmax(u, lo), hi)
                move = y - output                                                    # 8.
                new = s + self.step[l] * move                                        # 9.
                e = sp - vd
                h = np.where(start, 0.0, t - q[MS_T_EXEC])
                upd = {MS_PHASE: np.full(N, float(RUNNING)), MS_OUTPUT: y, MS_BIAS: d, MS_MOVE: move, MS_T_EXEC: t,
                       MS_N_RATE: q[MS_N_RATE] + (dc != du), MS_N_SAT: q[MS_N_SAT] + (y != u),
                       MS_ISE: q[MS_ISE] + (e * e) * h, MS_IAE: q[MS_IAE] + np.abs(e) * h, MS_DOSE: q[MS_DOSE] + y * h,
                       MS_N_EXEC: q[MS_N_EXEC] + 1.0}
            P[:, ex] = new[:, ex]
            for k, val in upd.items():
                q[k] = np.where(ex, val, q[k])
            w = HOLDING_WORD[l]
            self.holding[ex, w:w + 2] = float32_words(y[ex])                         # 11.
            # the period counter, in every scan the controller owned and leaves running
            count = own & (q[MS_PHASE] == RUNNING)
            nxt = q[MS_COUNT] + 1.0
            q[MS_COUNT] = np.where(count, np.where(nxt >= p[M_EVERY], 0.0, nxt), q[MS_COUNT])
            self.owned[l] = own


class LoopOwners:
    """A ``TuneRef`` (or None) and an ``MpcRef`` as ``HostScan``'s ``tun``: the tuners run, then the controllers with the
    tuners' mask; ``owned`` is the union, which the PI programs skip; ``holding`` is the image the two share (build the
    ``MpcRef`` with ``words=`` the ``TuneRef``, or both on one ``ControlRef``)."""

    def __init__(self, tun, mpc):
        self.tun, self.mpc = tun, mpc
        assert tun is None or tun.holding is mpc.holding, "one holding image"
        self.owned = np.zeros_like(mpc.owned)

    @property
    def holding(self):
        return self.mpc.holding

    def scan(self, values, faults, t_now, stepped=None):
        skip = None
        if self.tun is not None:
            self.tun.scan(values, faults, t_now, stepped)
            skip = self.tun.owned
        self.mpc.scan(values, faults, t_now, stepped, skip=skip)
        self.owned = self.mpc.owned if skip is None else (skip | self.mpc.owned)
