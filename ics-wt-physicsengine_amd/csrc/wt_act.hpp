// wt_act.hpp -- gfx950 device code of the per-reactor actuator programs (wt_ensemble_actuator_*): the final elements
// between the command path and the plant.  The reference's roadmap lists "actuator dynamics (valves, pumps)" next to
// its PID module; here each of the three dosing / inlet channels may carry a pump or valve with dead time, a
// first-order lag, a rate limit, backlash and a STUCK or FAIL_TO fault window.
//
//   actuate  runs in the scan lane of a reactor that stepped, right after apply_commands (and its command tamper,
//            wt_inj.hpp) and override_commands (alarm trips, wt_alm.hpp): the validated command of an enabled
//            channel is the pump's demand, its position (clamped to the channel's limit) becomes the boundary row
//            and the command the next step integrates under.  A PI output, a tampered command and a trip all reach
//            the plant through it.
//
// Device layout (array of structures, indexed by reactor like wtc / wti / wta: placement changes nothing):
//   par [N][CH][NV] fp64       enable, tau, rate, backlash, delay, fault, t_fault, t_repair, fail_value
//   st  [N][CH][NVS] fp64      position, applied, play, demand, delivered, travel, n_exec, n_rate, n_fault
//   q   [N][CH][MAX_DELAY]     the last MAX_DELAY demands, newest first
//   tp  [N] fp64               loop time of the last evaluation
// The C ABI is SoA ([CH][NV][N], [CH][NVS][N], [CH][MAX_DELAY][N]); the host transposes.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace wtv {

constexpr int CH = 3, NV = 9, NVS = 9, MAX_DELAY = 8;
enum { CH_ACID = 0, CH_CHLORINE, CH_INLET };
enum { V_ENABLE = 0, V_TAU, V_RATE, V_BACKLASH, V_DELAY, V_FAULT, V_T_FAULT, V_T_REPAIR, V_FAIL_VALUE };
enum { VS_POSITION = 0, VS_APPLIED, VS_PLAY, VS_DEMAND, VS_DELIVERED, VS_TRAVEL, VS_N_EXEC, VS_N_RATE, VS_N_FAULT };
enum { F_NONE = 0, F_STUCK, F_FAIL_TO, N_FAULTS };
constexpr int PAR_DOUBLES = CH * NV;        // 216 bytes per reactor
constexpr int ST_DOUBLES = CH * NVS;        // 216 bytes per reactor
constexpr int Q_DOUBLES = CH * MAX_DELAY;   // 192 bytes per reactor
constexpr double INLET_MIN = 0.1;           // "only update inlet flow if command is significant"

__host__ __device__ constexpr double limit_of(int k) { return k == CH_ACID ? 2.0 : k == CH_CHLORINE ? 1.0 : 20.0; }
__host__ __device__ constexpr int row_of(int k) { return k == CH_ACID ? 4 : k == CH_CHLORINE ? 6 : 0; }

struct ActArgs {
    int on;                  // 0: no program (the scan section reads this flag only)
    const double *par;       // [N][PAR_DOUBLES]
    double *st;              // [N][ST_DOUBLES]
    double *q;               // [N][Q_DOUBLES]
    double *tp;              // [N]
};

// a: ActArgs (read in place from the kernel arguments); cmd: CommandArgs of the scan (boundary block); c: the three
// commands the command path left (c[0] inlet, c[1] acid, c[2] chlorine), rewritten with what the plant receives;
// inlet_v: the validated inlet word apply_commands decoded; row0: boundary row 0 before apply_commands; t: the loop
// time the scan stores.  Spelled out in the order of tests/actuator_ref.py, nothing contracted into an fma.  The
// channels stay rolled: one channel's record is live at a time.  The scan lane is a single lane whose reactor waits on
// it, so what costs is the chain of memory round trips, not the arithmetic: the three enable flags come with t_prev,
// and an enabled channel's parameters, state and queue are all loaded before any of them is stored.
template <class A, class C> __device__ __forceinline__ void actuate(const A &a, const C &cmd, int64_t r, double c[3], double inlet_v,
                                                                    double row0, double t)
{
#pragma clang fp contract(off)
    const double *pr = a.par + r * PAR_DOUBLES;
    const double en0 = pr[V_ENABLE], en1 = pr[NV + V_ENABLE], en2 = pr[2 * NV + V_ENABLE];
    const double h = t - a.tp[r];
    a.tp[r] = t;
#pragma unroll 1
    for (int k = 0; k < CH; ++k) {
        if ((k == CH_ACID ? en0 : k == CH_CHLORINE ? en1 : en2) == 0.0) continue;
        const double *p = pr + k * NV;
        double *s = a.st + r * ST_DOUBLES + k * NVS;
        double2 *q2 = reinterpret_cast<double2 *>(a.q + r * Q_DOUBLES + k * MAX_DELAY);   // 64-byte aligned
        const double tau = p[V_TAU], rate = p[V_RATE], backlash = p[V_BACKLASH], delay = p[V_DELAY], fault = p[V_FAULT];
        const double t_fault = p[V_T_FAULT], t_repair = p[V_T_REPAIR], fail_value = p[V_FAIL_VALUE];
        const double position = s[VS_POSITION], applied0 = s[VS_APPLIED], play0 = s[VS_PLAY], demand0 = s[VS_DEMAND];
        const double delivered = s[VS_DELIVERED], travel = s[VS_TRAVEL], n_exec = s[VS_N_EXEC], n_rate = s[VS_N_RATE];
        const double n_fault = s[VS_N_FAULT];
        const double2 q01 = q2[0], q23 = q2[1], q45 = q2[2], q67 = q2[3];
        const double u = k == CH_ACID ? c[1] : k == CH_CHLORINE ? c[2] : (inlet_v > INLET_MIN ? inlet_v : demand0);
        // the queue before the shift: q[delay - 1] by selects (a dynamic index into registers would go to scratch)
        const double ud = delay == 0.0 ? u : delay == 1.0 ? q01.x : delay == 2.0 ? q01.y : delay == 3.0 ? q23.x
                        : delay == 4.0 ? q23.y : delay == 5.0 ? q45.x : delay == 6.0 ? q45.y : delay == 7.0 ? q67.x : q67.y;
        const double half = backlash * 0.5;
        const double play = fmax(ud - half, fmin(ud + half, play0));                    // play operator
        const double pl = tau > 0.0 ? (tau * position + h * play) / (tau + h) : play;   // backward-Euler lag
        const double lim = rate * h, d = pl - position;
        double pn = d > lim ? position + lim : d < -lim ? position - lim : pl;
        const bool cut = pn != pl;
        const bool hit = fault != (double)F_NONE && t_fault <= t && t < t_repair;
        if (hit) pn = fault == (double)F_STUCK ? position : fail_value;
        const double av = fmin(fmax(pn, 0.0), limit_of(k));
        double applied = applied0;
        if (k == CH_ACID) { applied = av; c[1] = av; }
        else if (k == CH_CHLORINE) { applied = av; c[2] = av; }
        else { if (av > INLET_MIN) applied = av; c[0] = av > INLET_MIN ? av : row0; }   // otherwise the row stays
        s[VS_POSITION] = pn;
        s[VS_APPLIED] = applied;
        s[VS_PLAY] = play;
        s[VS_DEMAND] = u;
        s[VS_DELIVERED] = delivered + applied0 * h;
        s[VS_TRAVEL] = travel + fabs(pn - position);
        s[VS_N_EXEC] = n_exec + 1.0;
        s[VS_N_RATE] = cut ? n_rate + 1.0 : n_rate;
        s[VS_N_FAULT] = hit ? n_fault + 1.0 : n_fault;
        q2[0] = make_double2(u, q01.x); q2[1] = make_double2(q01.y, q23.x);
        q2[2] = make_double2(q23.y, q45.x); q2[3] = make_double2(q45.y, q67.x);
        cmd.bc[row_of(k) * cmd.N + r] = k == CH_INLET ? c[0] : applied;
    }
}

} // namespace wtv
