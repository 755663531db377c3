// wt_ctl.hpp -- gfx950 device code of the per-reactor "virtual PLC program": up to two PI dosing loops that close the
// loop through the plant I/O images without leaving the step kernel (wt_ensemble_control_*).  It stands in for the
// master side of the reference's loop body (__main__.py:227-271): whatever a Modbus master would compute from the
// input image and write into the holding registers between two scans.  The reference has no controller of its own.
//
//   pi_execute   runs at a PLC scan, in the lane of a reactor that stepped, AFTER pack_inputs and apply_commands of
//                that scan (wt_plc.hpp): its output acts from the next scan on, exactly like a host master's
//                write_commands between two calls.  Loop 0 doses chlorine (holding words 2-3), loop 1 acid (words 0-1).
//                skip: bit l set -- the tune program (wt_tun.hpp) owned loop l in this scan: the loop changes no state
//                and writes no word; the shared t_prev still advances.  0: every enabled loop runs.
//
// Device layout (array of structures: the scan lane reads one reactor's record with wide loads):
//   par [N][LOOPS][NC] fp64   enable, sensor, direction, setpoint, kp, ki, bias, out_min, out_max
//   st  [N][ST_DOUBLES] fp64  [LOOPS][NCS] integral, output, ise, iae, dose, n_exec, n_held, n_sat; then t_prev
// The C ABI is SoA ([LOOPS][NC][N], [LOOPS][NCS][N]) like the boundary and constant blocks; the host transposes.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "wt_plc.hpp"

namespace wtc {

constexpr int LOOPS = 2, NC = 9, NCS = 8;
enum { C_ENABLE = 0, C_SENSOR, C_DIRECTION, C_SETPOINT, C_KP, C_KI, C_BIAS, C_OUT_MIN, C_OUT_MAX };
enum { CS_INTEGRAL = 0, CS_OUTPUT, CS_ISE, CS_IAE, CS_DOSE, CS_N_EXEC, CS_N_HELD, CS_N_SAT };
constexpr int PAR_DOUBLES = LOOPS * NC;             // 144 bytes per reactor: 16-byte aligned records
constexpr int T_PREV = LOOPS * NCS;                 // shared by both loops
constexpr int ST_DOUBLES = T_PREV + 2;              // padded to 16 bytes
// first holding word of each loop's output (float32 as high word, low word)
__host__ __device__ constexpr int loop_word(int loop) { return loop == 0 ? 2 : 0; }

struct CtlArgs {
    int on;                  // 0: no controller (the scan section reads this flag only)
    const double *par;       // [N][PAR_DOUBLES]
    double *st;              // [N][ST_DOUBLES]
    uint16_t *hr;            // [N][HR_WORDS] holding image (the one apply_commands decodes at the next scan)
};

// a: CtlArgs (read in place from the kernel arguments); value / fault: this scan's seven raw readings of reactor r
// (element i at [i * stride], LDS); t_now: the loop time the scan stores.  Every operation below is spelled out in the
// order of tests/control_ref.py and nothing is contracted into an fma, so the host restatement gives the same bits.
template <class A> __device__ __forceinline__ void pi_execute(const A &a, int64_t r, const float *value, const int *fault, int stride, double t_now, int skip = 0)
{
#pragma clang fp contract(off)
    double *s = a.st + r * ST_DOUBLES;
    const double h = t_now - s[T_PREV];
    s[T_PREV] = t_now;
#pragma unroll
    for (int l = 0; l < LOOPS; ++l) {          // unrolled: l, and with it every index into p, is a constant
        const double2 *p2 = reinterpret_cast<const double2 *>(a.par + r * PAR_DOUBLES + l * NC - l);   // 16-byte aligned
        double p[NC + 1];
#pragma unroll
        for (int i = 0; i < (NC + 1) / 2; ++i) { const double2 q = p2[i]; p[2 * i] = q.x; p[2 * i + 1] = q.y; }
        const double *c = p + l;   // loop 1's record starts one double into its first pair
        if (c[C_ENABLE] == 0.0 || ((skip >> l) & 1)) continue;
        double *q = s + l * NCS;
        const int si = (int)c[C_SENSOR];
        const float v = value[si * stride];
        if (!isfinite(v) || fault[si * stride] != 0) { q[CS_N_HELD] += 1.0; continue; }   // hold: write nothing
        const double e = c[C_DIRECTION] * (c[C_SETPOINT] - (double)v);
        const double integral = q[CS_INTEGRAL];
        double Ic = integral + (c[C_KI] * e) * h;
        double u = (c[C_BIAS] + c[C_KP] * e) + Ic;
        if ((u > c[C_OUT_MAX] && e > 0.0) || (u < c[C_OUT_MIN] && e < 0.0)) {     // conditional integration
            Ic = integral;
            u = (c[C_BIAS] + c[C_KP] * e) + Ic;
        }
        const double y = fmin(fmax(u, c[C_OUT_MIN]), c[C_OUT_MAX]);
        q[CS_INTEGRAL] = Ic; q[CS_OUTPUT] = y;
        const uint32_t b = wtp::f32_bits_from_double(y);
        uint16_t *w = a.hr + r * wtp::HR_WORDS + loop_word(l);
        w[0] = (uint16_t)(b >> 16); w[1] = (uint16_t)(b & 0xffffu);
        q[CS_ISE] = q[CS_ISE] + (e * e) * h;
        q[CS_IAE] = q[CS_IAE] + fabs(e) * h;
        q[CS_DOSE] = q[CS_DOSE] + y * h;
        q[CS_N_EXEC] += 1.0;
        if (y != u) q[CS_N_SAT] += 1.0;
    }
}

} // namespace wtc
