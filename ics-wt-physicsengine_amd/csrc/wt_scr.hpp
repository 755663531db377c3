// wt_scr.hpp -- gfx950 device code of the per-reactor score programs (wt_ensemble_score_*): what happened to the
// water.  Each reactor carries up to SLOTS bands on its true state (pH, chlorine or temperature of one zone, or the
// minimum, maximum or mean over its zones); after every outer step the time below and above the band, the deficit and
// excess areas, the exposure integral and the excursion runs accumulate per reactor, and an ensemble curve counts per
// outer step how many reactors were scored, below and above (optionally a coarse histogram of the value: the fan).
//
//   evaluate  runs in the end-of-outer-step section of run_item, called by every lane of the wavefront: the lanes
//             stage their zone's state in the LDS of the dead factor store, lane z = 0 of every reactor that stepped
//             scores its slots, and the curve takes one atomic add per wavefront, slot and counter (ballot + popcount)
//             and one per scored reactor for the fan.  It reads y0 and t_out and writes only the program's own arrays:
//             the plant computes the same bits with or without it, and f(y0) stays valid.
//
// Device layout (array of structures, indexed by reactor like wtd / wtv: placement changes nothing):
//   par    [N][SLOTS][NSP] fp64       kind, quantity, reduce, zone, lo, hi, t_start, t_end
//   st     [N][SLOTS][NSS] fp64       n_eval, time, integral, t_low, t_high, area_low, area_high, v_min, v_max, last,
//                                     out, n_exc, t_first_out, run, run_max
//   tp     [N] fp64                   ReactorState.time of the last evaluation
//   counts [cap][SLOTS][3] int32      scored, low, high per outer step since set / reset (optional)
//   fan    [cap][SLOTS][bins + 2]     int32 histogram of the scored value (optional)
// The C ABI is SoA ([SLOTS][NSP][N], [SLOTS][NSS][N]); the host transposes.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace wtsc {

constexpr int SLOTS = 4, NSP = 8, NSS = 15, MAX_BINS = 32, STAGE_DOUBLES = 3 * 64;
enum { K_OFF = 0, K_BAND, N_KINDS };
enum { Q_PH = 0, Q_CL, Q_T, N_QUANTITIES };
enum { R_ZONE = 0, R_MIN, R_MAX, R_MEAN, N_REDUCES };
enum { P_KIND = 0, P_QUANTITY, P_REDUCE, P_ZONE, P_LO, P_HI, P_T_START, P_T_END };
enum { S_N_EVAL = 0, S_TIME, S_INTEGRAL, S_T_LOW, S_T_HIGH, S_AREA_LOW, S_AREA_HIGH, S_V_MIN, S_V_MAX, S_LAST, S_OUT,
       S_N_EXC, S_T_FIRST_OUT, S_RUN, S_RUN_MAX };
constexpr int PAR_DOUBLES = SLOTS * NSP;              // 256 bytes per reactor
constexpr int ST_DOUBLES = SLOTS * NSS;               // 480 bytes per reactor

struct ScrArgs {
    int on;                  // 0: no program (the step kernel's section reads this flag only)
    int curve_cap;           // outer steps the curve holds (0: none)
    int bins;                // fan bins between fan_lo and fan_hi (0: no fan); the fan has bins + 2 counters per slot
    int step0;               // outer steps taken since set / reset before this call (make_args)
    const double *par;       // [N][PAR_DOUBLES]
    double *st;              // [N][ST_DOUBLES]
    double *tp;              // [N]
    int32_t *counts;         // [curve_cap][SLOTS][3] or nullptr (also once the curve is full)
    int32_t *fan;            // [curve_cap][SLOTS][bins + 2] or nullptr
    double fan_lo[SLOTS], fan_hi[SLOTS], fan_scale[SLOTS];   // scale = bins / (fan_hi - fan_lo), computed on the host
};

// bins + 2 counters: 0 below fan_lo, bins + 1 at or above fan_hi
__host__ __device__ inline int fan_bin(double v, double lo, double hi, double scale, int bins)
{
#pragma clang fp contract(off)
    if (v < lo) return 0;
    if (v >= hi) return bins + 1;
    const int b = (int)((v - lo) * scale);
    return 1 + (b < bins - 1 ? b : bins - 1);
}

__device__ __forceinline__ void add_relaxed(int32_t *p, int v)
{
    __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// One outer step's evaluation, called by all 64 lanes in uniform control flow.  live: this lane's reactor stepped (the
// sensor section's test); z, n: the lane's zone and the zone count; base: lane of zone 0 of its reactor; y: the
// lane's (pH, chlorine, temperature) after the step and its clamps; stage: STAGE_DOUBLES of LDS nothing else uses
// now; j: the outer step's index since set / reset.  Spelled out in the order of tests/score_ref.py, in fp64 without
// fused multiply-adds.  The slots stay rolled and their accumulators go through memory (the record is the reactor's
// own), so the section holds one slot's values at a time.
template <class A>
__device__ __forceinline__ void evaluate(const A &a, bool live, int z, int n, int lane, int base, int64_t r, double t,
                                         const double (&y)[3], double *stage, int j)
{
#pragma clang fp contract(off)
    __syncthreads();                         // the factor store is dead now
    stage[lane] = y[0]; stage[64 + lane] = y[1]; stage[128 + lane] = y[2];
    __syncthreads();
    const bool me = live && z == 0;          // one lane per reactor
    const double *p = a.par + r * PAR_DOUBLES;
    double *s = a.st + r * ST_DOUBLES;
    double h = 0.0;
    if (me) { h = t - a.tp[r]; a.tp[r] = t; }
    const bool curve = a.counts != nullptr && (unsigned)j < (unsigned)a.curve_cap;   // wave-uniform
#pragma unroll 1
    for (int k = 0; k < SLOTS; ++k) {
        bool scored = false, low = false, high = false;
        double v = 0.0;
        if (me) {
            const double *q = p + k * NSP;
            if (q[P_KIND] != (double)K_OFF && q[P_T_START] <= t && t < q[P_T_END]) {
                const double *x = stage + (int)q[P_QUANTITY] * 64 + base;
                const int red = (int)q[P_REDUCE], zone = (int)q[P_ZONE];
                if (red == R_ZONE) {
                    v = x[zone < 0 ? n - 1 : zone];
                } else {
                    v = x[0];
#pragma unroll 1
                    for (int i = 1; i < n; ++i) {
                        const double xi = x[i];
                        v = red == R_MIN ? (xi < v ? xi : v) : red == R_MAX ? (xi > v ? xi : v) : v + xi;
                    }
                    if (red == R_MEAN) v = v / (double)n;
                }
                double *sk = s + k * NSS;
                const double lo = q[P_LO], hi = q[P_HI];
                const double ne = sk[S_N_EVAL] + 1.0;
                sk[S_N_EVAL] = ne;
                sk[S_TIME] = sk[S_TIME] + h;
                sk[S_INTEGRAL] = sk[S_INTEGRAL] + v * h;
                sk[S_LAST] = v;
                const double vmin = sk[S_V_MIN], vmax = sk[S_V_MAX];
                sk[S_V_MIN] = ne == 1.0 ? v : (v < vmin ? v : vmin);
                sk[S_V_MAX] = ne == 1.0 ? v : (v > vmax ? v : vmax);
                low = v < lo; high = v > hi;
                if (low) { sk[S_T_LOW] = sk[S_T_LOW] + h; sk[S_AREA_LOW] = sk[S_AREA_LOW] + (lo - v) * h; }
                if (high) { sk[S_T_HIGH] = sk[S_T_HIGH] + h; sk[S_AREA_HIGH] = sk[S_AREA_HIGH] + (v - hi) * h; }
                if (low || high) {
                    if (sk[S_OUT] == 0.0) sk[S_N_EXC] = sk[S_N_EXC] + 1.0;
                    const double tf = sk[S_T_FIRST_OUT];
                    if (tf != tf) sk[S_T_FIRST_OUT] = t;
                    sk[S_OUT] = 1.0;
                    const double run = sk[S_RUN] + h, rmax = sk[S_RUN_MAX];
                    sk[S_RUN] = run;
                    sk[S_RUN_MAX] = run > rmax ? run : rmax;
                } else {
                    sk[S_OUT] = 0.0; sk[S_RUN] = 0.0;
                }
                scored = true;
            }
        }
        if (curve) {
            // integer counters: their values do not depend on the order of the additions
            const int ns = __popcll(__ballot(scored)), nl = __popcll(__ballot(low)), nh = __popcll(__ballot(high));
            int32_t *c = a.counts + ((int64_t)j * SLOTS + k) * 3;
            if (lane == 0) {
                if (ns) add_relaxed(c + 0, ns);
                if (nl) add_relaxed(c + 1, nl);
                if (nh) add_relaxed(c + 2, nh);
            }
            if (a.fan != nullptr && scored) {
                const int bins = a.bins;
                add_relaxed(a.fan + ((int64_t)j * SLOTS + k) * (bins + 2) + fan_bin(v, a.fan_lo[k], a.fan_hi[k], a.fan_scale[k], bins), 1);
            }
        }
    }
    __syncthreads();                         // staged values read; the next step's factors may overwrite them
}

// The host calls' kernel, one thread per reactor: the accumulators of set and reset.  Everything zero, except v_min,
// v_max, last and t_first_out NaN and t_prev = ReactorState.time; nothing is evaluated.
struct HostOpArgs { double *st; double *tp; const double *time; int64_t N; };
__global__ __launch_bounds__(256) void host_op_kernel(const HostOpArgs a)
{
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= a.N) return;
    double *s = a.st + r * ST_DOUBLES;
#pragma unroll 1
    for (int k = 0; k < SLOTS; ++k)
#pragma unroll 1
        for (int i = 0; i < NSS; ++i)
            s[k * NSS + i] = (i == S_V_MIN || i == S_V_MAX || i == S_LAST || i == S_T_FIRST_OUT) ? __builtin_nan("") : 0.0;
    a.tp[r] = a.time[r];
}

} // namespace wtsc
