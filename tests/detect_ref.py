"""Host restatement of the per-reactor anomaly detector programs (include/wtphys.h, csrc/wt_det.hpp), vectorised over
reactors.

numpy fp64 never contracts a product and a sum into an fma, ``np.fmax`` / ``np.abs`` / ``/`` are the IEEE operations
the device code uses, and every comparison below has the operands the device code has, so the state is bit-comparable
with ``ReactorEnsemble.detector_state()``.
"""
import numpy as np

(K_KIND, K_SENSOR, K_SOURCE, K_REF, K_REF_ARG, K_REF_SOURCE, K_MU, K_SIGMA, K_SLACK, K_LIMIT, K_T_ARM, K_ON_BAD) = range(12)
(KS_GP, KS_GN, KS_BASELINE, KS_X_PREV, KS_STAT, KS_STAT_MAX, KS_ALARM, KS_N_EVAL, KS_N_BAD, KS_N_ALARM, KS_N_RAISE,
 KS_T_FIRST, KS_T_DETECT, KS_N_TP, KS_N_FP, KS_N_FN) = range(16)
OFF, CUSUM, EWMA, FLATLINE = range(4)
IMAGE, FIELD = range(2)
CONST, SENSOR, TRACK = range(3)
HOLD, ALARM = range(2)


def _put(row, mask, value):
    row[...] = np.where(mask, value, row)


class DetectRef:
    """State of the program of N reactors.  ``params``: (4, 12, N) block of ``detector_block``; ``labels``: (2, N)
    label_start, label_end; ``loop_time``: (N,) loop time at set."""

    def __init__(self, params, labels, loop_time):
        self.p = np.array(params, dtype=np.float64)
        S, _, N = self.p.shape
        self.lab = np.array(np.broadcast_to(np.asarray(labels, dtype=np.float64), (2, N)))
        self.lt0 = None
        self.reset(loop_time)

    def reset(self, loop_time):
        """``wt_ensemble_detect_set`` / ``_reset``: the set-time state at ``loop_time``."""
        S, _, N = self.p.shape
        self.st = np.zeros((S, 16, N))
        self.st[:, [KS_BASELINE, KS_X_PREV, KS_T_FIRST, KS_T_DETECT]] = np.nan
        self.t_prev = np.array(np.broadcast_to(np.asarray(loop_time, dtype=np.float64), (N,)))

    def scan(self, v, f, t, stepped=None, image=None):
        """One PLC scan: ``v`` float32 (7, N) field readings, ``f`` (7, N) their fault codes, ``t`` (N,) the loop time
        the scan stores, ``stepped`` (N,) reactors that took the step (default: all), ``image`` the scan's (values,
        faults) after an injection program (default: the field readings)."""
        S, _, N = self.p.shape
        stepped = np.ones(N, dtype=bool) if stepped is None else np.asarray(stepped, dtype=bool)
        t = np.broadcast_to(np.asarray(t, dtype=np.float64), (N,))
        fv, ff = np.asarray(v, dtype=np.float32), np.asarray(f).astype(np.int64)
        iv, iff = (fv, ff) if image is None else (np.asarray(image[0], dtype=np.float32), np.asarray(image[1]).astype(np.int64))
        h = t - self.t_prev
        self.t_prev = np.where(stepped, t, self.t_prev)
        since = t >= self.lab[0]
        attacked = since & (t < self.lab[1])
        idx = np.arange(N)
        for s in range(S):
            p, q = self.p[s], self.st[s]
            kind, ref = p[K_KIND], p[K_REF]
            on = stepped & (kind != OFF) & (t >= p[K_T_ARM])
            si = p[K_SENSOR].astype(np.int64)
            field = p[K_SOURCE] == FIELD
            val = np.where(field, fv[si, idx], iv[si, idx])
            flt = np.where(field, ff[si, idx], iff[si, idx])
            bad = ~np.isfinite(val) | (flt != 0)
            second = ref == SENSOR
            wi = np.where(second, p[K_REF_ARG], 0.0).astype(np.int64)
            rfield = p[K_REF_SOURCE] == FIELD
            w = np.where(rfield, fv[wi, idx], iv[wi, idx])
            g = np.where(rfield, ff[wi, idx], iff[wi, idx])
            bad = bad | (second & (~np.isfinite(w) | (g != 0)))
            was = q[KS_ALARM] != 0
            _put(q[KS_N_BAD], on & bad, q[KS_N_BAD] + 1.0)
            good = on & ~bad
            with np.errstate(all="ignore"):
                x = val.astype(np.float64)
                track = ref == TRACK
                base = np.where(ref == CONST, p[K_REF_ARG],
                                np.where(second, w.astype(np.float64), np.where(np.isnan(q[KS_BASELINE]), x, q[KS_BASELINE])))
                _put(q[KS_BASELINE], good & track, base + (h / (p[K_REF_ARG] + h)) * (x - base))
                z = ((x - base) - p[K_MU]) / p[K_SIGMA]
                slack = p[K_SLACK]
                cgp = np.fmax(0.0, (q[KS_GP] + z) - slack)
                cgn = np.fmax(0.0, (q[KS_GN] - z) - slack)
                egp = q[KS_GP] + slack * (z - q[KS_GP])
                same = ~np.isnan(q[KS_X_PREV]) & (np.abs(x - q[KS_X_PREV]) <= slack)
                fgp = np.where(same, q[KS_GP] + h, 0.0)
                gp = np.where(kind == CUSUM, cgp, np.where(kind == EWMA, egp, fgp))
                stat = np.where(kind == CUSUM, np.fmax(cgp, cgn), np.where(kind == EWMA, np.abs(egp), fgp))
                _put(q[KS_GP], good, gp)
                _put(q[KS_GN], good & (kind == CUSUM), cgn)
                _put(q[KS_X_PREV], good, x)
                _put(q[KS_STAT], good, stat)
                _put(q[KS_STAT_MAX], good & (stat > q[KS_STAT_MAX]), stat)
                alarm = np.where(good, stat > p[K_LIMIT], was | (bad & (p[K_ON_BAD] == ALARM)))
            _put(q[KS_ALARM], on, alarm.astype(np.float64))
            _put(q[KS_N_EVAL], on, q[KS_N_EVAL] + 1.0)
            up = on & alarm
            _put(q[KS_N_ALARM], up, q[KS_N_ALARM] + 1.0)
            _put(q[KS_N_RAISE], up & ~was, q[KS_N_RAISE] + 1.0)
            _put(q[KS_T_FIRST], up & np.isnan(q[KS_T_FIRST]), t)
            _put(q[KS_T_DETECT], up & since & np.isnan(q[KS_T_DETECT]), t)
            _put(q[KS_N_TP], up & attacked, q[KS_N_TP] + 1.0)
            _put(q[KS_N_FN], on & ~alarm & attacked, q[KS_N_FN] + 1.0)
            _put(q[KS_N_FP], up & ~attacked, q[KS_N_FP] + 1.0)
