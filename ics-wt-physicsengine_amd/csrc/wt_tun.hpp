// wt_tun.hpp -- gfx950 device code of the per-reactor "tune program": a relay (Astrom-Hagglund) autotuner per PI loop
// that runs the standard commissioning experiment through the plant I/O images without leaving the step kernel
// (wt_ensemble_tune_*).  The reference's roadmap lists it as "Control tuning utilities (Ziegler-Nichols, Lambda)"; it
// has none.  The relay replaces the controller: the output is bias +- amplitude with hysteresis around the setpoint,
// the loop settles into its limit cycle, and the cycle's period and amplitude give the ultimate gain
// Ku = 4 d / (pi sqrt(a^2 - eps^2)), to which a tuning rule (two factors) is applied.
//
//   tune_execute  runs at a PLC scan, in the lane of a reactor that stepped, immediately BEFORE pi_execute (wt_ctl.hpp)
//                 and with its inputs: the scan's (possibly tampered) readings and the loop time the scan stores.  It
//                 writes the holding words as the PI does -- loop 0 chlorine (words 2-3), loop 1 acid (words 0-1) -- so
//                 its commands act from the next scan on.  It returns the mask of the loops it owned in this scan, the
//                 finishing scan included; pi_execute skips those.  With commission set, a finished experiment writes
//                 kp and ki into the PI loop's parameter record and sets the PI's integral to bias - pi_bias: the PI
//                 resumes at the next scan from the relay's centre output with the gains found.
//
// Device layout (array of structures: the scan lane reads one reactor's record with wide loads):
//   par [N][LOOPS][NU]  fp64  enable, sensor, direction, setpoint, bias, amplitude, hysteresis, t_start, t_max, settle,
//                             cycles, kp_factor, ti_factor, commission
//   st  [N][LOOPS][NUS] fp64  phase (0 waiting, 1 running, 2 done, 3 failed), relay, output, n_up, t_up, e_max, e_min,
//                             sum_period, sum_amp, n_cycles, period, amplitude, ku, kp, ki, t_begin, t_done, n_exec,
//                             n_held, commissioned
// The C ABI is SoA ([LOOPS][NU][N], [LOOPS][NUS][N]) like the control blocks; the host transposes.  The records live in
// the plant I/O array group: they come and go with plant I/O, and the switch is one of its scalars.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "wt_lanes.hpp"
#include "wt_plc.hpp"
#include "wt_ctl.hpp"

namespace wtu {

constexpr int LOOPS = wtc::LOOPS, NU = 14, NUS = 20;
enum { U_ENABLE = 0, U_SENSOR, U_DIRECTION, U_SETPOINT, U_BIAS, U_AMPLITUDE, U_HYSTERESIS, U_T_START, U_T_MAX, U_SETTLE,
       U_CYCLES, U_KP_FACTOR, U_TI_FACTOR, U_COMMISSION };
enum { US_PHASE = 0, US_RELAY, US_OUTPUT, US_N_UP, US_T_UP, US_E_MAX, US_E_MIN, US_SUM_PERIOD, US_SUM_AMP, US_N_CYCLES,
       US_PERIOD, US_AMPLITUDE, US_KU, US_KP, US_KI, US_T_BEGIN, US_T_DONE, US_N_EXEC, US_N_HELD, US_COMMISSIONED };
enum { PH_WAITING = 0, PH_RUNNING = 1, PH_DONE = 2, PH_FAILED = 3 };
constexpr int MAX_CYCLES = 4096;
constexpr int PAR_DOUBLES = LOOPS * NU;             // 224 bytes per reactor
constexpr int ST_DOUBLES = LOOPS * NUS;             // 320 bytes per reactor
static_assert(NU % 2 == 0 && NUS % 2 == 0, "the tuner's records are read in 16-byte pairs");
static_assert(U_SENSOR == U_ENABLE + 1 && U_SETPOINT == U_DIRECTION + 1 && U_AMPLITUDE == U_BIAS + 1 && U_T_START == U_HYSTERESIS + 1 &&
              U_SETTLE == U_T_MAX + 1 && U_KP_FACTOR == U_CYCLES + 1 && U_COMMISSION == U_TI_FACTOR + 1 && U_ENABLE % 2 == 0,
              "the parameter pairs tune_execute reads");
static_assert(US_RELAY == US_PHASE + 1 && US_N_UP == US_OUTPUT + 1 && US_E_MAX == US_T_UP + 1 && US_SUM_PERIOD == US_E_MIN + 1 &&
              US_N_CYCLES == US_SUM_AMP + 1 && US_AMPLITUDE == US_PERIOD + 1 && US_KP == US_KU + 1 && US_T_BEGIN == US_KI + 1 &&
              US_N_EXEC == US_T_DONE + 1 && US_COMMISSIONED == US_N_HELD + 1 && US_PHASE % 2 == 0,
              "the state pairs tune_execute reads and writes");

struct TunArgs {
    int on;                  // 0: no tune program (the scan section reads this flag only)
    const double *par;       // [N][PAR_DOUBLES]
    double *st;              // [N][ST_DOUBLES]
};

// a: TunArgs, c: the PI program's CtlArgs (its holding image, and its records when it is on), both read in place from
// the kernel arguments; value / fault: this scan's seven readings of reactor r (element i at [i * stride], LDS); t: the
// loop time the scan stores.  Every operation below is spelled out in the order of tests/tune_ref.py and nothing is
// contracted into an fma, so the host restatement gives the same bits; the divisions are IEEE divisions and the square
// root is wt::sqrt_k, the library's correctly rounded iteration without its rescaling of arguments below 2^-767 (an
// amplitude of 1e-115, which no reading of this plant resolves).  The library's own sqrt, and a literal -inf, each keep
// a constant live across the whole work item, which the n = 17...32 kernel pays for with a private segment.
template <class A, class C> __device__ __forceinline__ int tune_execute(const A &a, const C &c, int64_t r, const float *value, const int *fault, int stride, double t)
{
#pragma clang fp contract(off)
    int owned = 0;
#pragma unroll 1
    for (int l = 0; l < LOOPS; ++l) {
        // Both records in 16-byte pairs, each fetched where it is needed and stored where it changes: the scan lane has
        // few registers to spare (the n = 17...32 kernel none at all), so only the phase and the relay are held throughout.
        const double2 *p2 = reinterpret_cast<const double2 *>(a.par + r * PAR_DOUBLES + l * NU);
        double2 *q2 = reinterpret_cast<double2 *>(a.st + r * ST_DOUBLES + l * NUS);
        const double2 es = p2[U_ENABLE / 2];                        // enable, sensor
        if (es.x == 0.0) continue;
        double2 pr = q2[US_PHASE / 2];                              // phase, relay
        if (pr.x >= (double)PH_DONE) continue;
        bool write = false;                                         // the holding words get the output at the end of this scan
        double inf = INFINITY;
        asm volatile("" : "+v"(inf));                               // (-inf is then a source modifier, not a second literal)
        if (pr.x == (double)PH_WAITING) {
            if (t < p2[U_T_START / 2].y) continue;
            pr.x = (double)PH_RUNNING; pr.y = 0.0;                  // the experiment starts at this scan, output = bias
            double2 kb = q2[US_T_BEGIN / 2]; kb.y = t; q2[US_T_BEGIN / 2] = kb;          // ki, t_begin
            double2 tm = q2[US_E_MAX / 2]; tm.y = -inf; q2[US_E_MAX / 2] = tm;      // t_up, e_max
            double2 ms = q2[US_E_MIN / 2]; ms.x = inf; q2[US_E_MIN / 2] = ms;       // e_min, sum_period
            write = true;
        }
        owned |= 1 << l;
        const int si = (int)es.y;
        const float v = value[si * stride];
        if (!isfinite(v) || fault[si * stride] != 0) {
            double2 hc = q2[US_N_HELD / 2]; hc.x += 1.0; q2[US_N_HELD / 2] = hc;         // hold: relay and output stay
        } else {
            const double2 ds = p2[U_DIRECTION / 2];                 // direction, setpoint
            const double e = ds.x * (ds.y - (double)v);
            const double eps = p2[U_HYSTERESIS / 2].x;
            { double2 dn = q2[US_N_EXEC / 2]; dn.y += 1.0; q2[US_N_EXEC / 2] = dn; }     // t_done, n_exec
            if (pr.y == 0.0) pr.y = (e >= 0.0) ? 1.0 : -1.0;
            double2 tm = q2[US_E_MAX / 2], ms = q2[US_E_MIN / 2];   // t_up, e_max; e_min, sum_period
            tm.y = fmax(tm.y, e); ms.x = fmin(ms.x, e);
            if (pr.y < 0.0 && e > eps) {                            // an up-switch: the second and every later one closes a cycle
                pr.y = 1.0;
                double2 on = q2[US_N_UP / 2]; on.y += 1.0; q2[US_N_UP / 2] = on;         // output, n_up
                if (on.y >= 2.0 && on.y - 1.0 > p2[U_SETTLE / 2].y) {
                    double2 ac = q2[US_SUM_AMP / 2];                // sum_amp, n_cycles
                    ms.y += t - tm.x;
                    ac.x += (tm.y - ms.x) * 0.5;
                    ac.y += 1.0;
                    q2[US_SUM_AMP / 2] = ac;
                }
                tm.x = t; tm.y = -inf; ms.x = inf;
            } else if (pr.y > 0.0 && e < -eps) {
                pr.y = -1.0;
            }
            q2[US_E_MAX / 2] = tm; q2[US_E_MIN / 2] = ms;
            write = true;
            asm volatile("" ::: "memory");                          // the finish reads what it needs again
            const double2 ck = p2[U_CYCLES / 2];                    // cycles, kp_factor
            if (q2[US_N_CYCLES / 2].y == ck.x) {                    // finish: the cycle averages, Ku and the rule's gains
                const double2 ac = q2[US_SUM_AMP / 2];
                const double period = q2[US_SUM_PERIOD / 2].y / ac.y, amplitude = ac.x / ac.y;
                const double h = p2[U_HYSTERESIS / 2].x;
                const double arg = amplitude * amplitude - h * h;
                q2[US_PERIOD / 2] = make_double2(period, amplitude);
                if (!(arg > 0.0)) {
                    pr.x = (double)PH_FAILED;
                } else {
                    const double ku = (4.0 * p2[U_AMPLITUDE / 2].y) / (3.141592653589793 * wt::sqrt_k(arg));
                    const double kp = ck.y * ku;
                    const double2 tc = p2[U_TI_FACTOR / 2];         // ti_factor, commission
                    const double ki = tc.x > 0.0 ? kp / (tc.x * period) : 0.0;
                    q2[US_KU / 2] = make_double2(ku, kp);
                    { double2 kb = q2[US_KI / 2]; kb.x = ki; q2[US_KI / 2] = kb; }       // ki, t_begin
                    pr.x = (double)PH_DONE;
                    if (tc.y == 1.0 && c.on) {                      // hand the loop to the PI program with the gains found
                        double *cp = const_cast<double *>(c.par) + r * wtc::PAR_DOUBLES + l * wtc::NC;
                        if (cp[wtc::C_ENABLE] == 1.0) {
                            cp[wtc::C_KP] = kp; cp[wtc::C_KI] = ki;
                            c.st[r * wtc::ST_DOUBLES + l * wtc::NCS + wtc::CS_INTEGRAL] = p2[U_BIAS / 2].x - cp[wtc::C_BIAS];
                            double2 hc = q2[US_COMMISSIONED / 2]; hc.y = 1.0; q2[US_COMMISSIONED / 2] = hc;   // n_held, commissioned
                        }
                    }
                }
                double2 dn = q2[US_T_DONE / 2]; dn.x = t; q2[US_T_DONE / 2] = dn;        // t_done, n_exec
            }
        }
        // time-out: the experiment fails
        if (pr.x == (double)PH_RUNNING && t - q2[US_T_BEGIN / 2].y >= p2[U_T_MAX / 2].x) {
            pr.x = (double)PH_FAILED;
            double2 dn = q2[US_T_DONE / 2]; dn.x = t; q2[US_T_DONE / 2] = dn;
            write = true;
        }
        q2[US_PHASE / 2] = pr;
        if (write) {
            // bias + relay * d while the experiment runs (relay 0 before the first valid reading: the bias itself), and the
            // relay's centre once it has finished or failed
            const double2 ba = p2[U_BIAS / 2];                      // bias, amplitude
            const double output = pr.x == (double)PH_RUNNING ? ba.x + pr.y * ba.y : ba.x;
            double2 on = q2[US_OUTPUT / 2]; on.x = output; q2[US_OUTPUT / 2] = on;       // output, n_up
            const uint32_t b = wtp::f32_bits_from_double(output);
            uint16_t *w = c.hr + r * wtp::HR_WORDS + wtc::loop_word(l);
            w[0] = (uint16_t)(b >> 16); w[1] = (uint16_t)(b & 0xffffu);
        }
    }
    return owned;
}

} // namespace wtu
