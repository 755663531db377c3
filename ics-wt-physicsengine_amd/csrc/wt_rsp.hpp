// wt_rsp.hpp -- gfx950 device code of the per-reactor response programs (wt_ensemble_respond_*): the reaction of an
// operator or a safety PLC to what the alarm and detector programs noticed.  On a cause that has stood for the slot's
// reaction time, a slot takes a dosing loop out of automatic, holds or drives its output, and hands the loop back when
// the cause is gone.  The reference has alarms and interlocks on its list of missing parts and no reaction at all.
//
//   respond_execute  runs at a PLC scan, in the lane of a reactor that stepped, immediately AFTER tune_execute
//                    (wt_tun.hpp) and BEFORE mpc_execute (wt_mpc.hpp) and pi_execute (wt_ctl.hpp), with their inputs:
//                    the scan's (possibly wired and tampered) readings and the loop time the scan stores.  It writes the
//                    holding words as the PI does -- loop 0 chlorine (words 2-3), loop 1 acid (words 0-1) -- so its
//                    commands act from the next scan on.  It returns the mask of the loops it held in this scan; the
//                    controllers and the PI programs skip those exactly as they skip a loop a relay experiment has.
//
// One scan, slot by slot from 0 to 3 (t: the loop time the scan stores; h = t - t_prev, then t_prev = t; every slot
// whose cause is not OFF, with l its loop):
//   1. the cause c: ALARM -- the alarm program is on and its slot `index` is active; DETECTOR -- the detector program
//      is on and its slot `index` has its alarm set (both records as the previous scan left them: those programs run
//      later in the scan); BAD -- this scan's image copy of sensor `index` is not finite or carries a fault code.
//      if (c) n_cause += 1.
//   2. a slot that entered the scan engaged: time_engaged += h.  Unlatched: if (c) clearing = NaN; else { if clearing
//      is NaN, clearing = t; if (t - clearing >= clear_delay && t - t_engaged >= min_hold) the slot RELEASES:
//      phase = 0, t_released = t, clearing = NaN, and the hand-back (below). }  A latched slot stays engaged.
//   3. a slot that entered the scan idle: if (!c) pending = NaN; else { if pending is NaN, pending = t;
//      if (t - pending >= delay) the slot ENGAGES: phase = 1, pending = NaN, clearing = NaN, n_engaged += 1, t_first = t
//      if it is NaN, t_engaged = t, output = the float32 the loop's holding words decode to, widened to fp64. }  A slot
//      does not engage and release in one scan, nor release and engage.
//   4. a slot that is engaged now:
//        the tune program owned loop l in this scan: n_blocked += 1, nothing else;
//        else a lower slot owns loop l in this scan: output = the owner's output, n_tracked += 1;
//        else the slot owns the loop: HOLD y = output; MANUAL y = value; RAMP step = rate * h, d = value - output,
//        y = d > step ? output + step : d < -step ? output - step : value.  output = y, the loop's words = float32(y)
//        (high, low), n_owned += 1, and bit l of the returned mask is set.
//   Then owner[l] = the slot that owned loop l in this scan, -1 for none.
// The hand-back of a releasing slot with handback == BUMPLESS that owned its loop in the previous scan (owner[l] as the
// previous scan left it), where neither the tune program nor a lower slot has the loop in this scan: n_handback += 1;
// the PI program's loop l, if the program is on and the loop enabled, gets integral = output - (bias + kp * e) with
// e = direction * (setpoint - v) of this scan's reading v as the PI computes it, or output - bias where that reading is
// not finite or faulted; a controller of wt_mpc.hpp on loop l that is enabled and running gets its output = output.
// Both are stores of this scan lane which pi_execute and the scalar part of mpc_execute load afterwards in the same
// lane (the controllers' one-writer rule: nobody else writes `output` before the wavefront's part).
// A BUMP slot, and every other release, leaves the controllers' state alone: they continue from what they have.
//
// Device layout (array of structures, indexed by reactor like wta: placement changes nothing):
//   par  [N][SLOTS][NR]  fp64  cause, index, delay, loop, action, value, rate, latch, clear_delay, min_hold, handback
//   st   [N][SLOTS][NRS] fp64  phase (0 idle, 1 engaged), pending, clearing, output, t_first, t_engaged, t_released,
//                              n_engaged, time_engaged, n_owned, n_blocked, n_cause, n_tracked, n_handback
//   rst  [N][NRR] fp64         t_prev, owner_chlorine, owner_acid
// The C ABI is SoA ([SLOTS][NR][N], [SLOTS][NRS][N], [NRR][N]); the host transposes.  The arrays live in the plant I/O
// array group: they come and go with plant I/O, and the switch is one of its scalars.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "wt_plc.hpp"
#include "wt_ctl.hpp"
#include "wt_mpc.hpp"
#include "wt_alm.hpp"
#include "wt_det.hpp"

namespace wtrp {

constexpr int SLOTS = 4, LOOPS = wtc::LOOPS, NR = 11, NRS = 14, NRR = 3;
enum { R_CAUSE = 0, R_INDEX, R_DELAY, R_LOOP, R_ACTION, R_VALUE, R_RATE, R_LATCH, R_CLEAR_DELAY, R_MIN_HOLD, R_HANDBACK };
enum { RS_PHASE = 0, RS_PENDING, RS_CLEARING, RS_OUTPUT, RS_T_FIRST, RS_T_ENGAGED, RS_T_RELEASED, RS_N_ENGAGED, RS_TIME_ENGAGED,
       RS_N_OWNED, RS_N_BLOCKED, RS_N_CAUSE, RS_N_TRACKED, RS_N_HANDBACK };
enum { RR_T_PREV = 0, RR_OWNER_CHLORINE, RR_OWNER_ACID };
enum { C_OFF = 0, C_ALARM, C_DETECTOR, C_BAD, N_CAUSES };
enum { ACT_HOLD = 0, ACT_MANUAL, ACT_RAMP, N_ACTIONS };
enum { HB_BUMP = 0, HB_BUMPLESS };
enum { PH_IDLE = 0, PH_ENGAGED = 1 };
constexpr int PAR_DOUBLES = SLOTS * NR;     // 352 bytes per reactor
constexpr int ST_DOUBLES = SLOTS * NRS;     // 448 bytes per reactor
constexpr int RST_DOUBLES = NRR;
static_assert(RR_OWNER_ACID == RR_OWNER_CHLORINE + 1, "owner of loop l at RR_OWNER_CHLORINE + l");
static_assert(SLOTS < 15, "a loop's owner travels through the scan as slot + 1 in four bits");

struct RspArgs {
    int on;                  // 0: no program (the scan section reads this flag only)
    const double *par;       // [N][PAR_DOUBLES]
    double *st;              // [N][ST_DOUBLES]
    double *rst;             // [N][RST_DOUBLES]
};

// a: RspArgs; c: the PI program's CtlArgs (the holding image, and its records when it is on); alm, det, mpc: the alarm
// and detector programs' and the controllers' argument structs, all read in place from the kernel arguments.  value /
// fault: this scan's seven readings of reactor r as the image saw them (element i at [i * stride], LDS); t: the loop
// time the scan stores; tuned: the loops the tune program owned in this scan.  Every operation below is spelled out in
// the order of tests/respond_ref.py and nothing is contracted into an fma, so the host restatement gives the same bits.
// The slots stay rolled and every field is loaded where it is needed: one slot's record is live at a time.
template <class A, class C, class AL, class D, class M>
__device__ __forceinline__ int respond_execute(const A &a, const C &c, const AL &alm, const D &det, const M &mpc, int64_t r,
                                               const float *value, const int *fault, int stride, double t, int tuned)
{
#pragma clang fp contract(off)
    double *rs = a.rst + r * RST_DOUBLES;
    const double h = t - rs[RR_T_PREV];
    rs[RR_T_PREV] = t;
    int own = 0;                                                    // slot + 1 of this scan's owner, four bits a loop
    int held = 0;
#pragma unroll 1
    for (int s = 0; s < SLOTS; ++s) {
        const double *p = a.par + r * PAR_DOUBLES + s * NR;
        const double cause = p[R_CAUSE];
        if (cause == (double)C_OFF) continue;
        double *q = a.st + r * ST_DOUBLES + s * NRS;
        const int ix = (int)p[R_INDEX], l = (int)p[R_LOOP];
        // 1. the cause
        bool on;
        if (cause == (double)C_ALARM) on = alm.on && alm.st[r * wta::ST_DOUBLES + ix * wta::NAS + wta::AS_ACTIVE] != 0.0;
        else if (cause == (double)C_DETECTOR) on = det.on && det.st[r * wtk::ST_DOUBLES + ix * wtk::NKS + wtk::KS_ALARM] != 0.0;
        else on = !isfinite(value[ix * stride]) || fault[ix * stride] != 0;
        if (on) q[RS_N_CAUSE] = q[RS_N_CAUSE] + 1.0;
        bool engaged = q[RS_PHASE] != (double)PH_IDLE;
        const bool blocked = (tuned >> l) & 1;
        const int above = (own >> (4 * l)) & 15;                    // a lower slot that owns the loop in this scan, + 1
        uint16_t *w = c.hr + r * wtp::HR_WORDS + wtc::loop_word(l);
        if (engaged) {
            // 2. engaged over the interval that just ended; the release
            q[RS_TIME_ENGAGED] = q[RS_TIME_ENGAGED] + h;
            if (p[R_LATCH] == 0.0) {
                if (on) {
                    q[RS_CLEARING] = __builtin_nan("");
                } else {
                    double clearing = q[RS_CLEARING];
                    if (clearing != clearing) clearing = t;
                    if (t - clearing >= p[R_CLEAR_DELAY] && t - q[RS_T_ENGAGED] >= p[R_MIN_HOLD]) {
                        engaged = false; clearing = __builtin_nan("");
                        q[RS_PHASE] = (double)PH_IDLE;
                        q[RS_T_RELEASED] = t;
                        if (p[R_HANDBACK] == (double)HB_BUMPLESS && rs[RR_OWNER_CHLORINE + l] == (double)s && !blocked && above == 0) {
                            const double out = q[RS_OUTPUT];
                            q[RS_N_HANDBACK] = q[RS_N_HANDBACK] + 1.0;
                            if (c.on) {
                                const double *cp = c.par + r * wtc::PAR_DOUBLES + l * wtc::NC;
                                if (cp[wtc::C_ENABLE] != 0.0) {
                                    const int si = (int)cp[wtc::C_SENSOR];
                                    const float v = value[si * stride];
                                    double base = cp[wtc::C_BIAS];
                                    if (isfinite(v) && fault[si * stride] == 0) {
                                        const double e = cp[wtc::C_DIRECTION] * (cp[wtc::C_SETPOINT] - (double)v);
                                        base = cp[wtc::C_BIAS] + cp[wtc::C_KP] * e;
                                    }
                                    c.st[r * wtc::ST_DOUBLES + l * wtc::NCS + wtc::CS_INTEGRAL] = out - base;
                                }
                            }
                            if (mpc.on) {
                                double *mq = mpc.st + r * wtm::ST_DOUBLES + l * wtm::NMS;
                                if (mpc.par[r * wtm::PAR_DOUBLES + l * wtm::NM + wtm::M_ENABLE] != 0.0 && mq[wtm::MS_PHASE] == (double)wtm::PH_RUNNING)
                                    mq[wtm::MS_OUTPUT] = out;
                            }
                        }
                    }
                    q[RS_CLEARING] = clearing;
                }
            }
        } else if (on) {
            // 3. the reaction time; the engagement
            double pending = q[RS_PENDING];
            if (pending != pending) pending = t;
            if (t - pending >= p[R_DELAY]) {
                engaged = true; pending = __builtin_nan("");
                q[RS_PHASE] = (double)PH_ENGAGED;
                q[RS_CLEARING] = pending;
                q[RS_N_ENGAGED] = q[RS_N_ENGAGED] + 1.0;
                if (q[RS_T_FIRST] != q[RS_T_FIRST]) q[RS_T_FIRST] = t;
                q[RS_T_ENGAGED] = t;
                q[RS_OUTPUT] = (double)__uint_as_float(((uint32_t)w[0] << 16) | (uint32_t)w[1]);
            }
            q[RS_PENDING] = pending;
        } else {
            q[RS_PENDING] = __builtin_nan("");
            continue;
        }
        if (!engaged) continue;
        // 4. the loop
        if (blocked) {
            q[RS_N_BLOCKED] = q[RS_N_BLOCKED] + 1.0;
        } else if (above) {
            q[RS_OUTPUT] = a.st[r * ST_DOUBLES + (above - 1) * NRS + RS_OUTPUT];
            q[RS_N_TRACKED] = q[RS_N_TRACKED] + 1.0;
        } else {
            const double output = q[RS_OUTPUT], action = p[R_ACTION];
            double y = output;
            if (action == (double)ACT_MANUAL) {
                y = p[R_VALUE];
            } else if (action == (double)ACT_RAMP) {
                const double target = p[R_VALUE];
                const double step = p[R_RATE] * h;
                const double d = target - output;
                y = d > step ? output + step : d < -step ? output - step : target;
            }
            q[RS_OUTPUT] = y;
            const uint32_t b = wtp::f32_bits_from_double(y);
            w[0] = (uint16_t)(b >> 16); w[1] = (uint16_t)(b & 0xffffu);
            q[RS_N_OWNED] = q[RS_N_OWNED] + 1.0;
            own |= (s + 1) << (4 * l);
            held |= 1 << l;
        }
    }
    rs[RR_OWNER_CHLORINE] = (double)((own & 15) - 1);
    rs[RR_OWNER_ACID] = (double)(((own >> 4) & 15) - 1);
    return held;
}

} // namespace wtrp
