// wt_trd.hpp -- gfx950 device code of the per-reactor trend recorder programs (wt_ensemble_trend_*): the plant's
// historian.  A fused call returns end-of-call state; the series a study plots at the scan rate -- the PI output, a
// detector's statistic, valve position against command, the alarm word -- are recorded here, inside the call, instead
// of by a host loop of one launch and one download per scan.
//
//   record   runs in the scan lane of a reactor that stepped, after wtk::evaluate, last in the scan: every slot takes
//            one value of this scan (a reading, a fault code, a command, or one entry of another program's state
//            record as that program left it earlier in this same scan and lane -- no barrier is needed), thins it by
//            `every`, a deadband and a time window, and appends (t, value) to the slot's store.  The values are copies:
//            nothing is computed from them but the deadband test.  The program is passive: it writes its own arrays only.
//
// Device layout (array of structures, indexed by reactor like wtk: placement changes nothing):
//   par   [N][SLOTS][NT] fp64          tag, index, every, deadband, t_start, t_end   (48-byte slots: three 16-byte loads)
//   st    [N][SLOTS][NTS] fp64         n_seen, n_recorded, n_dropped, last           (32-byte slots: two 16-byte pairs)
//   store [N][SLOTS][cap] (fp64, fp64) time, value of a sample, one 16-byte store
// The store is written by one lane per reactor, each at its own position (deadbands and windows make the positions of
// neighbouring reactors drift apart, and placement deals neighbouring lanes unrelated reactors), so a sample-major
// layout would not coalesce; with the samples of one (reactor, slot) contiguous, eight successive samples fill one
// 128-byte line, which the L2 merges before it goes out, and time and value leave in a single store.
// The C ABI is SoA ([SLOTS][NT][N], [SLOTS][NTS][N], [SLOTS][cap][N]); the host transposes and unwraps a ring.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "wt_ctl.hpp"
#include "wt_inj.hpp"
#include "wt_alm.hpp"
#include "wt_act.hpp"
#include "wt_det.hpp"

namespace wtt {

constexpr int SLOTS = 8, NT = 6, NTS = 4;
enum { T_TAG = 0, T_INDEX, T_EVERY, T_DEADBAND, T_T_START, T_T_END };
enum { TS_N_SEEN = 0, TS_N_RECORDED, TS_N_DROPPED, TS_LAST };
enum { G_OFF = 0, G_IMAGE_VALUE, G_IMAGE_FAULT, G_FIELD_VALUE, G_FIELD_FAULT, G_COMMAND, G_CONTROL, G_INJECT, G_ALARM,
       G_ALARM_WORD, G_ACTUATOR, G_DETECT, N_TAGS };
constexpr int PAR_DOUBLES = SLOTS * NT;     // 384 bytes per reactor
constexpr int ST_DOUBLES = SLOTS * NTS;     // 256 bytes per reactor

// entries `index` may name under each tag (0: the tag takes no index)
__host__ __device__ constexpr int index_range(int tag)
{
    return tag >= G_IMAGE_VALUE && tag <= G_FIELD_FAULT ? 7 : tag == G_COMMAND ? 3 : tag == G_CONTROL ? wtc::LOOPS * wtc::NCS
         : tag == G_INJECT ? wti::ST_DOUBLES : tag == G_ALARM ? wta::ST_DOUBLES : tag == G_ALARM_WORD ? 1
         : tag == G_ACTUATOR ? wtv::ST_DOUBLES : tag == G_DETECT ? wtk::ST_DOUBLES : 0;
}

struct TrdArgs {
    int on;                  // 0: no program (the scan section reads this flag only)
    int wrap;                // 0: a full store drops the sample; otherwise the oldest sample is overwritten
    int64_t cap;             // samples per slot and reactor, >= 1
    const double *par;       // [N][PAR_DOUBLES]
    double *st;              // [N][ST_DOUBLES]
    double2 *store;          // [N][SLOTS][cap]
};

// a: the whole argument block (read in place from the kernel arguments): the recorder's own TrdArgs and the records of
// the programs it reads; value / fault: this scan's seven readings of reactor r as the image saw them (element i at
// [i * stride], LDS); cmd: the three commands the scan hands to the reload (inlet, acid, chlorine at [k * stride], LDS);
// t: the loop time the scan stores.  Plain loads, compares and stores; the slots stay rolled and of one slot's record a
// pair or two is live at a time.
template <class A> __device__ __forceinline__ void record(const A &a, int64_t r, const float *value, const int *fault, const double *cmd,
                                                         int stride, double t)
{
#pragma clang fp contract(off)
    const int64_t N = a.sens.N, cap = a.trd.cap;
    const double capd = (double)cap;
#pragma unroll 1
    for (int s = 0; s < SLOTS; ++s) {
        const double2 *p2 = reinterpret_cast<const double2 *>(a.trd.par + r * PAR_DOUBLES + s * NT);   // 16-byte aligned
        const double2 ti = p2[0];                                   // tag, index
        if (ti.x == (double)G_OFF) continue;
        const double2 w = p2[2];                                    // t_start, t_end
        if (t < w.x || t >= w.y) continue;
        double2 *q2 = reinterpret_cast<double2 *>(a.trd.st + r * ST_DOUBLES + s * NTS);
        double2 sr = q2[0];                                         // n_seen, n_recorded
        const double2 ed = p2[1];                                   // every, deadband
        const double m = sr.x;                                      // scans seen before this one
        sr.x = m + 1.0;
        // m % every == 0 on whole numbers below 2^53: the quotient of a multiple is exact, and any other quotient,
        // rounded either way, leaves a remainder that is not zero
        if (m - floor(m / ed.x) * ed.x != 0.0) { q2[0] = sr; continue; }
        const int tag = (int)ti.x, ix = (int)ti.y;
        double x;
        if (tag == G_IMAGE_VALUE) x = (double)value[ix * stride];
        else if (tag == G_IMAGE_FAULT) x = (double)fault[ix * stride];
        else if (tag == G_FIELD_VALUE) x = (double)a.sens.out_value[ix * N + r];
        else if (tag == G_FIELD_FAULT) x = (double)a.sens.out_fault[ix * N + r];
        else if (tag == G_COMMAND) x = cmd[(ix == 2 ? 0 : ix + 1) * stride];         // acid, chlorine, inlet
        else {
            // one entry of another program's record; NaN while that program is off
            const double *rec = nullptr;
            int width = 0;
            if (tag == G_CONTROL) { if (a.ctl.on) rec = a.ctl.st; width = wtc::ST_DOUBLES; }
            else if (tag == G_INJECT) { if (a.inj.on) rec = a.inj.st; width = wti::ST_DOUBLES; }
            else if (tag == G_ALARM) { if (a.alm.on) rec = a.alm.st; width = wta::ST_DOUBLES; }
            else if (tag == G_ACTUATOR) { if (a.act.on) rec = a.act.st; width = wtv::ST_DOUBLES; }
            else if (tag == G_DETECT) { if (a.det.on) rec = a.det.st; width = wtk::ST_DOUBLES; }
            x = __builtin_nan("");
            if (tag == G_ALARM_WORD) { if (a.alm.on) x = (double)a.alm.word[r]; }
            else if (rec) x = rec[r * width + ix];
        }
        double2 dl = q2[1];                                         // n_dropped, last
        const bool changed = (x == x || dl.y == dl.y) && !(fabs(x - dl.y) <= ed.y);
        if (sr.y == 0.0 || ed.y < 0.0 || changed) {
            if (!a.trd.wrap && sr.y >= capd) dl.x += 1.0;            // full: dropped, but the deadband moves on
            else {
                const int64_t pos = (int64_t)(sr.y - floor(sr.y / capd) * capd);      // n_recorded % cap
                if ((uint64_t)pos < (uint64_t)cap) a.trd.store[(r * SLOTS + s) * cap + pos] = make_double2(t, x);
                sr.y += 1.0;
            }
            dl.y = x;
            q2[1] = dl;
        }
        q2[0] = sr;
    }
}

} // namespace wtt
