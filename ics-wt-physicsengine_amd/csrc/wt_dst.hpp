// wt_dst.hpp -- gfx950 device code of the per-reactor disturbance programs (wt_ensemble_disturb_*): a plant that
// moves on its own.  Each reactor carries up to SLOTS disturbances of its raw-water side or its chemical stocks (a
// step, a ramp, a diurnal sine, Ornstein-Uhlenbeck wandering) on the boundary rows the command path does not own.
//
//   evaluate  runs in the end-of-outer-step section of run_item (one lane per reactor that stepped, before the sensor
//             and plant-I/O section), and in wt_ensemble_disturb_set at set time: it advances every slot to the
//             reactor's time and composes the targeted rows into the boundary block -- the boundary of the reactor's
//             next outer step (zero-order hold).
//   compose   writes the targeted rows from the base block and the slots' current offsets (wt_ensemble_set_boundary
//             with a program set: a new base, no draw).
//
// Device layout (array of structures, indexed by reactor like wtv / wta: placement changes nothing):
//   par  [N][SLOTS][ND] fp64     kind, row, t_start, t_end, a, b, c
//   st   [N][ST_DOUBLES] fp64    [SLOTS][NDS] value, x, n_eval, n_draw; then [SLOTS][NC] the OU cache h, phi, s
//   base [NB][N] fp64            the boundary the offsets are added to (a boundary block, like bc)
//   tp   [N] fp64                ReactorState.time of the last evaluation
//   hist [N][hist_cap][SLOTS]    offsets after evaluation j (optional)
// The C ABI is SoA ([SLOTS][ND][N], [SLOTS][NDS][N], [cap][SLOTS][N]); the host transposes.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "wt_sensors.hpp"

namespace wtd {

constexpr int SLOTS = 4, ND = 7, NDS = 4, NC = 3, NB = 10;
enum { K_OFF = 0, K_STEP, K_RAMP, K_SINE, K_OU, N_KINDS };
enum { D_KIND = 0, D_ROW, D_T_START, D_T_END, D_A, D_B, D_C };
enum { DS_VALUE = 0, DS_X, DS_N_EVAL, DS_N_DRAW };
enum { C_H = 0, C_PHI, C_S };
constexpr int PAR_DOUBLES = SLOTS * ND;               // 224 bytes per reactor
constexpr int ST_DOUBLES = SLOTS * NDS + SLOTS * NC;  // 224 bytes per reactor
constexpr double PI = 3.141592653589793, LOG10_E = 0.4342944819032518;

// the rows a slot may target: not 0, 4, 6 (inlet, acid and chlorine flow belong to the command path or the master)
__host__ __device__ constexpr bool row_allowed(int row) { return row == 1 || row == 2 || row == 3 || row == 5 || row == 7 || row == 8 || row == 9; }

// pH to [0, 14], inlet temperature to [0, 100], ambient temperature free, the other rows (chlorine, concentrations,
// heat-loss coefficient) >= 0
__host__ __device__ inline double clamp_row(int row, double v)
{
    return row == 1 ? fmin(fmax(v, 0.0), 14.0) : row == 3 ? fmin(fmax(v, 0.0), 100.0) : row == 8 ? v : fmax(v, 0.0);
}

// sin(pi v).  The reduction to a quarter turn is exact (v - k/2), so there is no large-argument path: OCML's sin and
// sinpi carry one, and its registers cost the step kernels scratch.  Then fdlibm's kernel polynomials on
// [-pi/4, pi/4] (k_sin.c, k_cos.c): within a few ulp of sin.
__device__ __forceinline__ double sinpi_k(double v)
{
#pragma clang fp contract(off)
    const double k = __builtin_rint(v * 2.0);
    const double x = (v - k * 0.5) * PI, z = x * x;
    const double rs = 8.33333333332248946124e-03 + z * (-1.98412698298579493134e-04 + z * (2.75573137070700676789e-06 +
                      z * (-2.50507602534068634195e-08 + z * 1.58969099521155010221e-10)));
    const double sn = x + (z * x) * (-1.66666666666666324348e-01 + z * rs);
    const double rc = z * (4.16666666666666019037e-02 + z * (-1.38888888888741095749e-03 + z * (2.48015872894767294178e-05 +
                      z * (-2.75573143513906633035e-07 + z * (2.08757232129817482790e-09 + z * -1.13596475577881948265e-11)))));
    const double hz = 0.5 * z, w = 1.0 - hz;
    const double cs = w + (((1.0 - w) - hz) + z * rc);
    const int q = (int)(k - 4.0 * __builtin_floor(k * 0.25));    // quadrant 0..3
    const double y = (q & 1) ? cs : sn;
    return (q & 2) ? -y : y;
}

struct DstArgs {
    int on;                  // 0: no program (the step kernel's section reads this flag only)
    int hist_cap;            // entries per reactor of hist (0: none)
    uint32_t seed_lo, seed_hi;
    int64_t reactor_base;    // global index of reactor 0 (sharded ensembles keep distinct streams)
    const double *par;       // [N][PAR_DOUBLES]
    double *st;              // [N][ST_DOUBLES]
    double *base;            // [NB][N]
    double *tp;              // [N]
    double *hist;            // [N][hist_cap][SLOTS] or nullptr
};

// The targeted rows of reactor r: row = clamp(base + d_s0 + d_s1 + ...) over the non-OFF slots on that row, in
// ascending slot order, written once, by the lowest such slot.  Rows no slot targets are not touched.
template <class A> __device__ __forceinline__ void compose(const A &a, int64_t r, double *bc, int64_t N)
{
#pragma clang fp contract(off)
    const double *p = a.par + r * PAR_DOUBLES;
    const double *s = a.st + r * ST_DOUBLES;
#pragma unroll 1
    for (int k = 0; k < SLOTS; ++k) {
        if (p[k * ND + D_KIND] == (double)K_OFF) continue;
        const double row = p[k * ND + D_ROW];
        bool first = true;
#pragma unroll 1
        for (int j = 0; j < k; ++j) first = first && !(p[j * ND + D_KIND] != (double)K_OFF && p[j * ND + D_ROW] == row);
        if (!first) continue;
        const int64_t o = (int64_t)row * N + r;
        double v = a.base[o];
#pragma unroll 1
        for (int j = k; j < SLOTS; ++j)
            if (p[j * ND + D_KIND] != (double)K_OFF && p[j * ND + D_ROW] == row) v = v + s[j * NDS + DS_VALUE];
        bc[o] = clamp_row((int)row, v);
    }
}

// Advances every slot of reactor r to t (its ReactorState.time), records the offsets, composes the rows.  Spelled out
// in the order of tests/disturb_ref.py, in fp64 without fused multiply-adds; z is the sensor suite's Box-Muller
// deviate (fp32) on counter (reactor_base + r, slot, n_draw, 1) -- word 3 = 1 keeps it off every sensor stream.
// The slots stay rolled and their offsets go through memory (the record is the reactor's own), so the section holds
// one slot's values at a time.  (h, phi, s) of an OU slot are cached: with a fixed dt they are computed once.
// wt_exp: e^y (wt::ExpK, the step kernel's own exp).
template <class A, class E> __device__ __forceinline__ void evaluate(const A &a, int64_t r, double t, double *bc, int64_t N, const E &wt_exp)
{
#pragma clang fp contract(off)
    const double *p = a.par + r * PAR_DOUBLES;
    double *s = a.st + r * ST_DOUBLES;
    const double h = t - a.tp[r];
    a.tp[r] = t;
    const double j = s[DS_N_EVAL];                        // this evaluation's history entry
    const bool keep = a.hist != nullptr && j < (double)a.hist_cap;
#pragma unroll 1
    for (int k = 0; k < SLOTS; ++k) {
        const double *q = p + k * ND;
        double *sk = s + k * NDS;
        double *ck = s + SLOTS * NDS + k * NC;
        const double kind = q[D_KIND], t0 = q[D_T_START], t1 = q[D_T_END], ka = q[D_A], kb = q[D_B], kc = q[D_C];
        const bool in = t0 <= t && t < t1;
        double d = 0.0, x = sk[DS_X], nd = sk[DS_N_DRAW];
        if (kind == (double)K_STEP) {
            d = in ? ka : 0.0;
        } else if (kind == (double)K_RAMP) {
            d = t < t0 ? 0.0 : ka + kb * (fmin(t, t1) - t0);
        } else if (kind == (double)K_SINE) {
            d = in ? ka * sinpi_k((2.0 * (t - t0)) / kb + kc / PI) : 0.0;   // sin(2 pi (t - t_start) / b + c)
        } else if (kind == (double)K_OU) {
            if (in) {
                if (h > 0.0) {
                    double phi = ck[C_PHI], sc = ck[C_S];
                    if (ck[C_H] != h) {
                        // the kernel's own exp (exp10_k, the inlet pH's): e^y = 10^(y log10 e)
                        phi = wt_exp(-h / kb);
                        sc = ka * sqrt(1.0 - wt_exp((-2.0 * h) / kb));
                        ck[C_H] = h; ck[C_PHI] = phi; ck[C_S] = sc;
                    }
                    uint32_t w[4];
                    wts::philox4x32_10((uint32_t)(a.reactor_base + r), (uint32_t)k, (uint32_t)nd, 1u, a.seed_lo, a.seed_hi, w);
                    const double z = (double)wts::box_muller(w);
                    x = x * phi + sc * z;
                    nd = nd + 1.0;
                }
                d = x;
            }
        }
        sk[DS_VALUE] = d; sk[DS_X] = x; sk[DS_N_EVAL] = j + 1.0; sk[DS_N_DRAW] = nd;
        if (keep) a.hist[(r * a.hist_cap + (int64_t)j) * SLOTS + k] = d;
    }
    compose(a, r, bc, N);
}

// The host calls' kernel, one thread per reactor: SET evaluates at ReactorState.time (t_prev = that time: nothing is
// drawn), COMPOSE recomposes from a new base, RESTORE writes the base back into the targeted rows.
enum { OP_SET = 0, OP_COMPOSE, OP_RESTORE };
struct HostOpArgs { DstArgs d; double *bc; const double *time; int64_t N; int op; };
template <class E> __global__ __launch_bounds__(256) void host_op_kernel(const HostOpArgs a)
{
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= a.N) return;
    if (a.op == OP_SET) {
        evaluate(a.d, r, a.time[r], a.bc, a.N, E());
    } else if (a.op == OP_COMPOSE) {
        compose(a.d, r, a.bc, a.N);
    } else {
        const double *p = a.d.par + r * PAR_DOUBLES;
#pragma unroll 1
        for (int k = 0; k < SLOTS; ++k)
            if (p[k * ND + D_KIND] != (double)K_OFF) {
                const int64_t o = (int64_t)p[k * ND + D_ROW] * a.N + r;
                a.bc[o] = a.d.base[o];
            }
    }
}

} // namespace wtd
