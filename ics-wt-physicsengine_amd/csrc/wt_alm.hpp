// wt_alm.hpp -- gfx950 device code of the per-reactor alarm and interlock programs (wt_ensemble_alarm_*): the safety
// side of the control layer, at every PLC scan.  The reference names "alarm logic and interlocks" in its control
// layer and lists them as missing; here they are limits on a reading with deadband, on-delay and latch, and a trip
// that forces a dosing command to a safe value while an alarm stands.
//
//   override_commands  runs in the scan lane of a reactor that stepped, right after apply_commands (and its command
//                      tamper, wt_inj.hpp) decoded and validated the holding words: a trip in force replaces the acid
//                      or chlorine command and its boundary row -- the trip wired at the final element, downstream of
//                      a man-in-the-middle.  The holding image keeps the master's words.
//   evaluate           runs in the same lane after pi_execute (wt_ctl.hpp): every slot's limit on an IMAGE reading
//                      (the scan's copy after any injection program, what the input image and the PI programs see)
//                      or a FIELD reading (the instrument's own, what wts::emit stored this step), then the trips of
//                      the next scan and the alarm word.
//
// Device layout (array of structures, indexed by reactor like wtc / wti: placement changes nothing):
//   par  [N][SLOTS][NA] fp64   kind, sensor, source, setpoint, deadband, on_delay, latch, on_bad, action, trip_value
//                              (80-byte slots: five 16-byte loads)
//   st   [N][SLOTS][NAS] fp64  active, cond, pending, n_act, t_first, t_last, time_active, n_bad
//   rst  [N][NAR] fp64         t_prev, first_out, ovr_acid, ovr_chlorine, n_ovr_acid, n_ovr_chlorine
//   word [N] uint16            bits 0-3 active, 4-7 cond, 8 acid trip, 9 chlorine trip, 12-14 first_out + 1
// The C ABI is SoA ([SLOTS][NA][N], [SLOTS][NAS][N], [NAR][N]); the host transposes.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "wt_plc.hpp"

namespace wta {

constexpr int SLOTS = 4, NA = 10, NAS = 8, NAR = 6;
enum { A_KIND = 0, A_SENSOR, A_SOURCE, A_SETPOINT, A_DEADBAND, A_ON_DELAY, A_LATCH, A_ON_BAD, A_ACTION, A_TRIP_VALUE };
enum { AS_ACTIVE = 0, AS_COND, AS_PENDING, AS_N_ACT, AS_T_FIRST, AS_T_LAST, AS_TIME_ACTIVE, AS_N_BAD };
enum { AR_T_PREV = 0, AR_FIRST_OUT, AR_OVR_ACID, AR_OVR_CHLORINE, AR_N_OVR_ACID, AR_N_OVR_CHLORINE };
enum { K_OFF = 0, K_HIGH, K_LOW, N_KINDS };
enum { SRC_IMAGE = 0, SRC_FIELD };
enum { ON_BAD_HOLD = 0, ON_BAD_ALARM };
enum { ACT_NONE = 0, ACT_TRIP_ACID, ACT_TRIP_CHLORINE, N_ACTIONS };
constexpr int PAR_DOUBLES = SLOTS * NA;     // 320 bytes per reactor
constexpr int ST_DOUBLES = SLOTS * NAS;     // 256 bytes per reactor
constexpr int RST_DOUBLES = NAR;            // 48 bytes per reactor: the trip pair sits 16-byte aligned
constexpr unsigned W_ACID = 1u << 8, W_CHLORINE = 1u << 9;
constexpr int W_FIRST_OUT_SHIFT = 12;

struct AlmArgs {
    int on;                  // 0: no program (the scan section reads this flag only)
    const double *par;       // [N][PAR_DOUBLES]
    double *st;              // [N][ST_DOUBLES]
    double *rst;             // [N][RST_DOUBLES]
    uint16_t *word;          // [N]
};

// a: AlmArgs (read in place from the kernel arguments); cmd: CommandArgs of the scan (boundary block); c: the three
// commands apply_commands returned (c[1] acid, c[2] chlorine).  The trips come from the previous evaluation.
template <class A, class C> __device__ __forceinline__ void override_commands(const A &a, const C &cmd, int64_t r, double c[3])
{
    double *rs = a.rst + r * RST_DOUBLES;
    const double2 ovr = *reinterpret_cast<const double2 *>(rs + AR_OVR_ACID);
    if (ovr.x == ovr.x) {
        c[1] = wtp::validate_flow_rate((float)ovr.x, 2.0);
        cmd.bc[4 * cmd.N + r] = c[1];
        rs[AR_N_OVR_ACID] += 1.0;
    }
    if (ovr.y == ovr.y) {
        c[2] = wtp::validate_flow_rate((float)ovr.y, 1.0);
        cmd.bc[6 * cmd.N + r] = c[2];
        rs[AR_N_OVR_CHLORINE] += 1.0;
    }
}

// value / fault: this scan's seven readings of reactor r as the image saw them (element i at [i * stride], LDS);
// field_value / field_fault: the instruments' readings [NSENS][N] that wts::emit stored this step (the barrier before
// the scan lane orders them: the step kernel's workgroup is one wavefront); t: the loop time the scan stores.  Spelled
// out in the order of tests/alarm_ref.py, nothing contracted into an fma.  The slots stay rolled: one slot's record
// is live at a time.
template <class A> __device__ __forceinline__ void evaluate(const A &a, int64_t r, int64_t N, const float *value, const int *fault,
                                                           int stride, const float *field_value, const uint8_t *field_fault, double t)
{
#pragma clang fp contract(off)
    double *rs = a.rst + r * RST_DOUBLES;
    const double h = t - rs[AR_T_PREV];
    rs[AR_T_PREV] = t;
    double first_out = rs[AR_FIRST_OUT];
    double ovr_acid = __builtin_nan(""), ovr_chlorine = __builtin_nan("");
    unsigned word = 0;
#pragma unroll 1
    for (int s = 0; s < SLOTS; ++s) {
        const double2 *p2 = reinterpret_cast<const double2 *>(a.par + r * PAR_DOUBLES + s * NA);   // 16-byte aligned
        const double2 ks = p2[0];                                   // kind, sensor
        if (ks.x == (double)K_OFF) continue;
        const double2 ss = p2[1], dd = p2[2], lb = p2[3], at = p2[4];  // source, setpoint; deadband, on_delay; latch, on_bad; action, trip
        double *q = a.st + r * ST_DOUBLES + s * NAS;
        bool active = q[AS_ACTIVE] != 0.0;
        bool cond = q[AS_COND] != 0.0;
        if (active) q[AS_TIME_ACTIVE] = q[AS_TIME_ACTIVE] + h;      // active over the interval that just ended
        const int si = (int)ks.y;
        float v; int f;
        if (ss.x == (double)SRC_FIELD) { v = field_value[si * N + r]; f = field_fault[si * N + r]; }
        else { v = value[si * stride]; f = fault[si * stride]; }
        const bool bad = !isfinite(v) || f != 0;
        if (bad) q[AS_N_BAD] += 1.0;
        if (!bad || lb.y != (double)ON_BAD_HOLD) {                 // HOLD on a bad reading: nothing else changes
            const double vd = (double)v, sp = ss.y, db = dd.x;
            if (bad) cond = true;
            else if (ks.x == (double)K_HIGH) cond = active ? !(vd < sp - db) : vd > sp;
            else cond = active ? !(vd > sp + db) : vd < sp;
            q[AS_COND] = cond ? 1.0 : 0.0;
            if (!active) {
                if (cond) {
                    double pending = q[AS_PENDING];
                    if (pending != pending) pending = t;
                    if (t - pending >= dd.y) {
                        active = true; pending = __builtin_nan("");
                        q[AS_ACTIVE] = 1.0;
                        q[AS_N_ACT] += 1.0;
                        if (q[AS_T_FIRST] != q[AS_T_FIRST]) q[AS_T_FIRST] = t;
                        if (first_out == -1.0) first_out = (double)s;
                    }
                    q[AS_PENDING] = pending;
                } else {
                    q[AS_PENDING] = __builtin_nan("");
                }
            } else if (!cond && lb.x == 0.0) {
                active = false;
                q[AS_ACTIVE] = 0.0;
            }
            if (active) q[AS_T_LAST] = t;
        }
        if (active) {
            word |= 1u << s;
            if (at.x == (double)ACT_TRIP_ACID && ovr_acid != ovr_acid) ovr_acid = at.y;
            if (at.x == (double)ACT_TRIP_CHLORINE && ovr_chlorine != ovr_chlorine) ovr_chlorine = at.y;
        }
        if (cond) word |= 1u << (4 + s);
    }
    rs[AR_FIRST_OUT] = first_out;
    *reinterpret_cast<double2 *>(rs + AR_OVR_ACID) = make_double2(ovr_acid, ovr_chlorine);
    if (ovr_acid == ovr_acid) word |= W_ACID;
    if (ovr_chlorine == ovr_chlorine) word |= W_CHLORINE;
    word |= (unsigned)((int)first_out + 1) << W_FIRST_OUT_SHIFT;
    a.word[r] = (uint16_t)word;
}

} // namespace wta
