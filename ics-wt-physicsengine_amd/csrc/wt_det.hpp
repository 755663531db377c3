// wt_det.hpp -- gfx950 device code of the per-reactor anomaly detector programs (wt_ensemble_detect_*): the
// change-detection statistic an intrusion- or fault-detection study evaluates, at every PLC scan, judged against the
// known attack window.  A limit alarm (wt_alm.hpp) has no memory of the residual; a slot here keeps one: a two-sided
// CUSUM, an EWMA chart or a flat-line (replay) timer on the residual of a reading against a constant, a second
// reading or the slot's own tracked baseline.
//
//   evaluate   runs in the scan lane of a reactor that stepped, after wta::evaluate: every slot's statistic on an
//              IMAGE reading (the scan's copy after any injection program) or a FIELD reading (the instrument's own),
//              its alarm, and the confusion counts against the reactor's label.  The program is passive: it writes
//              its own arrays only.
//
// Device layout (array of structures, indexed by reactor like wta: placement changes nothing):
//   par  [N][SLOTS][NK] fp64   kind, sensor, source, ref, ref_arg, ref_source, mu, sigma, slack, limit, t_arm, on_bad
//                              (96-byte slots: six 16-byte loads)
//   st   [N][SLOTS][NKS] fp64  gp, gn, baseline, x_prev, stat, stat_max, alarm, n_eval, n_bad, n_alarm, n_raise,
//                              t_first, t_detect, n_tp, n_fp, n_fn (128-byte slots, read and written in 16-byte pairs)
//   lab  [N][NKR] fp64         label_start, label_end (one 16-byte load)
//   tp   [N] fp64              t_prev
// The C ABI is SoA ([SLOTS][NK][N], [SLOTS][NKS][N], [NKR][N], [N]); the host transposes.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace wtk {

constexpr int SLOTS = 4, NK = 12, NKS = 16, NKR = 2;
enum { K_KIND = 0, K_SENSOR, K_SOURCE, K_REF, K_REF_ARG, K_REF_SOURCE, K_MU, K_SIGMA, K_SLACK, K_LIMIT, K_T_ARM, K_ON_BAD };
enum { KS_GP = 0, KS_GN, KS_BASELINE, KS_X_PREV, KS_STAT, KS_STAT_MAX, KS_ALARM, KS_N_EVAL, KS_N_BAD, KS_N_ALARM, KS_N_RAISE,
       KS_T_FIRST, KS_T_DETECT, KS_N_TP, KS_N_FP, KS_N_FN };
enum { KR_LABEL_START = 0, KR_LABEL_END };
enum { D_OFF = 0, D_CUSUM, D_EWMA, D_FLATLINE, N_KINDS };
enum { SRC_IMAGE = 0, SRC_FIELD };
enum { REF_CONST = 0, REF_SENSOR, REF_TRACK, N_REFS };
enum { ON_BAD_HOLD = 0, ON_BAD_ALARM };
constexpr int PAR_DOUBLES = SLOTS * NK;     // 384 bytes per reactor
constexpr int ST_DOUBLES = SLOTS * NKS;     // 512 bytes per reactor

struct DetArgs {
    int on;                  // 0: no program (the scan section reads this flag only)
    const double *par;       // [N][PAR_DOUBLES]
    double *st;              // [N][ST_DOUBLES]
    const double *lab;       // [N][NKR]
    double *tp;              // [N]
};

// value / fault: this scan's seven readings of reactor r as the image saw them (element i at [i * stride], LDS);
// field_value / field_fault: the instruments' readings [NSENS][N] that wts::emit stored this step; t: the loop time
// the scan stores.  Spelled out in the order of tests/detect_ref.py: adds, multiplies, divides, compares, fmax and
// fabs only, nothing contracted into an fma.  The slots stay rolled and every state pair is loaded where it is needed
// and stored where it is done: one slot's record is live at a time, and of that record a pair or two.
template <class A> __device__ __forceinline__ void evaluate(const A &a, int64_t r, int64_t N, const float *value, const int *fault,
                                                           int stride, const float *field_value, const uint8_t *field_fault, double t)
{
#pragma clang fp contract(off)
    const double h = t - a.tp[r];
    a.tp[r] = t;
    const double2 lab = *reinterpret_cast<const double2 *>(a.lab + r * NKR);
    const bool since = t >= lab.x, attacked = since && t < lab.y;
#pragma unroll 1
    for (int s = 0; s < SLOTS; ++s) {
        const double2 *p2 = reinterpret_cast<const double2 *>(a.par + r * PAR_DOUBLES + s * NK);   // 16-byte aligned
        const double2 ks = p2[0];                                   // kind, sensor
        if (ks.x == (double)D_OFF) continue;
        const double2 ab = p2[5];                                   // t_arm, on_bad
        if (t < ab.x) continue;
        double2 *q2 = reinterpret_cast<double2 *>(a.st + r * ST_DOUBLES + s * NKS);
        const double2 sr = p2[1], ra = p2[2];                       // source, ref; ref_arg, ref_source
        const int si = (int)ks.y;
        float v, w = 0.0f; int f;
        if (sr.x == (double)SRC_FIELD) { v = field_value[si * N + r]; f = field_fault[si * N + r]; }
        else { v = value[si * stride]; f = fault[si * stride]; }
        bool bad = !isfinite(v) || f != 0;
        if (sr.y == (double)REF_SENSOR) {
            const int wi = (int)ra.x;
            int g;
            if (ra.y == (double)SRC_FIELD) { w = field_value[wi * N + r]; g = field_fault[wi * N + r]; }
            else { w = value[wi * stride]; g = fault[wi * stride]; }
            bad = bad || !isfinite(w) || g != 0;
        }
        double2 an = q2[KS_ALARM / 2];                              // alarm, n_eval
        const bool was = an.x != 0.0;
        bool alarm = was;
        if (bad) {
            double2 ba = q2[KS_N_BAD / 2];                          // n_bad, n_alarm
            ba.x += 1.0;
            q2[KS_N_BAD / 2] = ba;
            if (ab.y == (double)ON_BAD_ALARM) alarm = true;
        } else {
            const double x = (double)v;
            double2 bx = q2[KS_BASELINE / 2];                       // baseline, x_prev
            double base;
            if (sr.y == (double)REF_CONST) base = ra.x;
            else if (sr.y == (double)REF_SENSOR) base = (double)w;
            else {
                base = bx.x != bx.x ? x : bx.x;
                bx.x = base + (h / (ra.x + h)) * (x - base);
            }
            const double2 ms = p2[3], sl = p2[4];                   // mu, sigma; slack, limit
            const double z = ((x - base) - ms.x) / ms.y;
            double2 g = q2[KS_GP / 2];                              // gp, gn
            double stat;
            if (ks.x == (double)D_CUSUM) {
                g.x = fmax(0.0, (g.x + z) - sl.x);
                g.y = fmax(0.0, (g.y - z) - sl.x);
                stat = fmax(g.x, g.y);
            } else if (ks.x == (double)D_EWMA) {
                g.x = g.x + sl.x * (z - g.x);
                stat = fabs(g.x);
            } else {
                g.x = (bx.y == bx.y && fabs(x - bx.y) <= sl.x) ? g.x + h : 0.0;
                stat = g.x;
            }
            q2[KS_GP / 2] = g;
            bx.y = x;
            q2[KS_BASELINE / 2] = bx;
            alarm = stat > sl.y;
            double2 sm = q2[KS_STAT / 2];                           // stat, stat_max
            sm.x = stat;
            sm.y = stat > sm.y ? stat : sm.y;
            q2[KS_STAT / 2] = sm;
        }
        an.x = alarm ? 1.0 : 0.0;
        an.y += 1.0;
        q2[KS_ALARM / 2] = an;
        if (alarm) {
            double2 ba = q2[KS_N_BAD / 2];                          // n_bad, n_alarm
            ba.y += 1.0;
            q2[KS_N_BAD / 2] = ba;
            double2 rf = q2[KS_N_RAISE / 2];                        // n_raise, t_first
            if (!was) rf.x += 1.0;
            if (rf.y != rf.y) rf.y = t;
            q2[KS_N_RAISE / 2] = rf;
        }
        if (alarm || attacked) {
            double2 dt = q2[KS_T_DETECT / 2], pn = q2[KS_N_FP / 2]; // t_detect, n_tp; n_fp, n_fn
            if (alarm && since && dt.x != dt.x) dt.x = t;
            if (attacked) { if (alarm) dt.y += 1.0; else pn.y += 1.0; }
            else pn.x += 1.0;
            q2[KS_T_DETECT / 2] = dt;
            q2[KS_N_FP / 2] = pn;
        }
    }
}

} // namespace wtk
