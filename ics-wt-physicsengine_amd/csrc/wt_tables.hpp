// wt_tables.hpp -- what the step kernel computes WITH: tolerances and status bits, scipy's Radau IIA / num_jac
// constants (rc::, radau.py:11-40, common.py:248-253), the fp64 constant tables that reach the kernels as scalar
// loads from the kernel-argument block (KTab: RHS sections, RTab: solver sections) with their loaders, and the
// project's own exp / exp10: OCML's algorithm with OCML's coefficients taken from those tables
// (checked bit for bit against the library's: tools/ubench/expcheck.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "wt_dst.hpp"

namespace wt {

constexpr int SPH = 0, SCL = 1, STT = 2;  // species index inside a lane
// Branch weights matter beyond the branch: the register allocator keeps in VGPRs what the frequent blocks use
// and parks the rest in AGPRs, so the rare paths of the solver loop are marked as such.
#define WT_RARE(x) __builtin_expect(!!(x), 0)
#define WT_USUAL(x) __builtin_expect(!!(x), 1)
constexpr double RTOL = 1e-6, ATOL = 1e-8; // reactor.py:481-483
constexpr int NEWTON_MAXITER = 6;          // radau.py:43
constexpr double MIN_FACTOR = 0.2, MAX_FACTOR = 10.0;

// status bits (include/wtphys.h)
constexpr uint32_t ST_T_RANGE = 1, ST_SOLVER_FAILED = 2, ST_CLAMP_PH = 4, ST_CLAMP_CL = 8,
                   ST_CLAMP_T = 16, ST_T_RANGE_POST = 32, ST_NONFINITE = 64, ST_STEP_LIMIT = 128;

// Radau IIA / num_jac constants with the values scipy's module-level expressions
// produce (radau.py:11-40, common.py:248-253), as exact hex literals.
namespace rc {
constexpr double C0 = 0x1.3d8b64657caeap-3;       // (4 - sqrt6)/10
constexpr double C1 = 0x1.4a36c0803a6dfp-1;       // (4 + sqrt6)/10
constexpr double E0 = -0x1.418fd8baffe05p+3, E1 = 0x1.61d41b2d54580p+0, E2 = -0x1.5555555555555p-2;
constexpr double MU_REAL = 0x1.d1a48d83e731dp+1;  // 3.637834252744496
constexpr double MU_CR = 0x1.572db93e0c672p+1;    // 2.6810828736277523
constexpr double MU_CI = -0x1.86747f2c3fcb6p+1;   // -3.050430199247411
constexpr double T00 = 0.09443876248897524, T01 = -0.14125529502095421, T02 = 0.03002919410514742;
constexpr double T10 = 0.25021312296533332, T11 = 0.20412935229379994, T12 = -0.38294211275726192;
// T[2] = [1, 1, 0]
constexpr double TI00 = 4.17871859155190428, TI01 = 0.32768282076106237, TI02 = 0.52337644549944951;
constexpr double TI10 = -4.17871859155190428, TI11 = -0.32768282076106237, TI12 = 0.47662355450055044;
constexpr double TI20 = 0.50287263494578682, TI21 = -2.57192694985560522, TI22 = 0.59603920482822492;
constexpr double P00 = 0x1.418fd8baffe05p+3, P01 = -0x1.9a12ce7b30915p+4, P02 = 0x1.f295c43b61425p+3;
constexpr double P10 = -0x1.61d41b2d54580p+0, P11 = 0x1.497af24bb677ep+3, P12 = -0x1.1d406ee60becfp+3;
constexpr double P20 = 0x1.5555555555555p-2, P21 = -0x1.5555555555555p+1, P22 = 0x1.aaaaaaaaaaaabp+1;
constexpr double NJ_REJECT = 0x1.6a09e667f3bcdp-46; // EPS**0.875
constexpr double NJ_SMALL = 0x1.0p-39;             // EPS**0.75
constexpr double NJ_BIG = 0x1.0p-13;               // EPS**0.25
constexpr double NJ_MINF = 0x1.f4p-43;             // 1e3*EPS
constexpr double NJ_F0 = 0x1.0p-26;                // EPS**0.5
constexpr double NEWTON_TOL = 0x1.0624dd2f1a9fcp-10; // max(10 EPS/rtol, min(0.03, sqrt(rtol))) = 1e-3
constexpr double LN10 = 0x1.26bb1bbb55516p+1;      // np.log(10)
constexpr double K_ARR = -0x1.5248ea03d1718p+12;   // -(45000/8.314)  thermodynamics.py:188
constexpr double INV_TREF = 0x1.bf1da5ca77e69p-9;  // 1/293.15
} // namespace rc

// ---------------------------------------------------------------- fp64 constants of the RHS as scalar loads
// A VALU instruction on gfx950 cannot carry a 64-bit literal: every fp64 constant that is not an inline constant
// reaches it through an SGPR pair, i.e. two s_mov_b32 -- and with one wavefront per SIMD a scalar move costs the
// same issue slot as an fp64 FMA (measured: tools/ubench/issue.hip).  The exponential's polynomial alone is ten
// such pairs per inlined copy of the RHS.  So the constants of a section sit in the kernel-argument block
// (filled by the host, wtphys.hip: make_args) and are fetched at the top of the section with s_load_dwordx16:
// eight constants per issue slot instead of half a constant.
// exp / exp10 follow OCML's algorithm with OCML's coefficients (checked bit for bit against the library's on the
// device over 4M arguments each: tools/ubench/expcheck.hip), so nothing changes numerically.
typedef double d8 __attribute__((ext_vector_type(8)));
struct alignas(64) KTab {
    // section P -- pH properties: 24 doubles
    double pc[10];                                                   // exp polynomial, degree-11 term first
    double log2_10, lg2_hi, lg2_lo, ln10_hi, ln10_lo, t_hi, t_lo;    // exp10 argument reduction and range
    double c2303, ln10, c002, pad_p[4];
    // section T -- temperature properties: 32 doubles
    double tc[10];
    double log2e, ln2_hi, ln2_lo, e_hi, e_lo;                        // exp argument reduction and range
    double k_arr, inv_tref, c27315, c1em4;                           // Arrhenius (thermodynamics.py:160-193)
    double rho_max, rho_an, rho20, rho_sl, c20, c8, c100;            // density branches (spatial.py:177-189), T range
    double dense_bias;                                               // developer knob WT_DENSE_COUPLING: 1.0 = every Jacobian counts as coupling rows to neighbours' T
    double pad_t[5];
};
static_assert(sizeof(KTab) == 56 * 8, "KTab layout");

__host__ __device__ constexpr KTab default_ktab()
{
    KTab k{};
    constexpr double c[10] = {0x1.ade156a5dcb37p-26, 0x1.28af3fca7ab0cp-22, 0x1.71dee623fde64p-19, 0x1.a01997c89e6b0p-16,
                              0x1.a01a014761f6ep-13, 0x1.6c16c1852b7b0p-10, 0x1.1111111122322p-7, 0x1.55555555502a1p-5,
                              0x1.5555555555511p-3, 0x1.000000000000bp-1};
    for (int i = 0; i < 10; ++i) { k.pc[i] = c[i]; k.tc[i] = c[i]; }
    k.log2_10 = 0x1.a934f0979a371p+1; k.lg2_hi = 0x1.34413509f79ffp-2; k.lg2_lo = -0x1.9dc1da994fd21p-59;
    k.ln10_hi = 0x1.26bb1bbb55516p+1; k.ln10_lo = -0x1.f48ad494ea3e9p-53;
    k.t_hi = 0x1.34413509f79ffp+8; k.t_lo = -0x1.439b746e36b52p+8;   // 10^x overflows above / is 0 below
    k.c2303 = 2.303; k.ln10 = rc::LN10; k.c002 = 0.02;
    k.log2e = 0x1.71547652b82fep+0; k.ln2_hi = 0x1.62e42fefa39efp-1; k.ln2_lo = 0x1.abc9e3b39803fp-56;
    k.e_hi = 0x1.62e42fefa39efp+9; k.e_lo = -0x1.74910d52d3051p+9;
    k.k_arr = rc::K_ARR; k.inv_tref = rc::INV_TREF; k.c27315 = 273.15; k.c1em4 = 0.0001;
    k.rho_max = 999.97; k.rho_an = -0.008; k.rho20 = 998.2; k.rho_sl = -2.1e-4 * 998.2; k.c20 = 20.0; k.c8 = 8.0; k.c100 = 100.0;
    return k;
}

// the constants a section works with, as plain doubles (SGPR pairs after the loads below)
struct KP { double c[10], log2_10, lg2_hi, lg2_lo, ln10_hi, ln10_lo, t_hi, t_lo, c2303, ln10, c002; };
struct KT { double c[10], log2e, ln2_hi, ln2_lo, e_hi, e_lo, k_arr, inv_tref, c27315, c1em4, rho_max, rho_an, rho20, rho_sl, c20, c8, c100, dense_bias; };

__host__ __device__ constexpr KP kp_of(const KTab &t)
{
    KP k{};
    for (int i = 0; i < 10; ++i) k.c[i] = t.pc[i];
    k.log2_10 = t.log2_10; k.lg2_hi = t.lg2_hi; k.lg2_lo = t.lg2_lo; k.ln10_hi = t.ln10_hi; k.ln10_lo = t.ln10_lo;
    k.t_hi = t.t_hi; k.t_lo = t.t_lo; k.c2303 = t.c2303; k.ln10 = t.ln10; k.c002 = t.c002;
    return k;
}
__host__ __device__ constexpr KT kt_of(const KTab &t)
{
    KT k{};
    for (int i = 0; i < 10; ++i) k.c[i] = t.tc[i];
    k.log2e = t.log2e; k.ln2_hi = t.ln2_hi; k.ln2_lo = t.ln2_lo; k.e_hi = t.e_hi; k.e_lo = t.e_lo;
    k.k_arr = t.k_arr; k.inv_tref = t.inv_tref; k.c27315 = t.c27315; k.c1em4 = t.c1em4;
    k.rho_max = t.rho_max; k.rho_an = t.rho_an; k.rho20 = t.rho20; k.rho_sl = t.rho_sl; k.c20 = t.c20; k.c8 = t.c8; k.c100 = t.c100; k.dense_bias = t.dense_bias;
    return k;
}

typedef const __attribute__((address_space(4))) d8 *KVec;
// three / four s_load_dwordx16 from the kernel-argument segment
__device__ __forceinline__ KP load_kp(const __attribute__((address_space(4))) KTab *t)
{
    KVec q = (KVec)t;
    const d8 a = q[0], b = q[1], c = q[2];
    KP k;
#pragma unroll
    for (int i = 0; i < 8; ++i) k.c[i] = a[i];
    k.c[8] = b[0]; k.c[9] = b[1];
    k.log2_10 = b[2]; k.lg2_hi = b[3]; k.lg2_lo = b[4]; k.ln10_hi = b[5]; k.ln10_lo = b[6]; k.t_hi = b[7];
    k.t_lo = c[0]; k.c2303 = c[1]; k.ln10 = c[2]; k.c002 = c[3];
    return k;
}
__device__ __forceinline__ KT load_kt(const __attribute__((address_space(4))) KTab *t)
{
    KVec q = (KVec)t + 3;
    const d8 a = q[0], b = q[1], c = q[2], d = q[3];
    KT k;
#pragma unroll
    for (int i = 0; i < 8; ++i) k.c[i] = a[i];
    k.c[8] = b[0]; k.c[9] = b[1];
    k.log2e = b[2]; k.ln2_hi = b[3]; k.ln2_lo = b[4]; k.e_hi = b[5]; k.e_lo = b[6]; k.k_arr = b[7];
    k.inv_tref = c[0]; k.c27315 = c[1]; k.c1em4 = c[2]; k.rho_max = c[3]; k.rho_an = c[4]; k.rho20 = c[5]; k.rho_sl = c[6]; k.c20 = c[7];
    k.c8 = d[0]; k.c100 = d[1]; k.dense_bias = d[2];
    return k;
}

// e^t for the reduced argument t, times 2^dn (the tail both exponentials share)
__device__ __forceinline__ double exp_tail(const double c[10], double t, double dn)
{
    double p = c[0];
#pragma unroll
    for (int i = 1; i < 10; ++i) p = __builtin_fma(t, p, c[i]);
    p = __builtin_fma(t, p, 1.0);
    p = __builtin_fma(t, p, 1.0);
    return __builtin_amdgcn_ldexp(p, (int)dn);
}
__device__ __forceinline__ double exp_k(const KT &k, double x)
{
    const double dn = __builtin_rint(x * k.log2e);
    const double t = __builtin_fma(-dn, k.ln2_lo, __builtin_fma(-dn, k.ln2_hi, x));
    double z = exp_tail(k.c, t, dn);
    z = (x > k.e_hi) ? __builtin_inf() : z;
    return (x < k.e_lo) ? 0.0 : z;
}
__device__ __forceinline__ double exp10_k(const KP &k, double x)
{
    const double dn = __builtin_rint(x * k.log2_10);
    const double u = __builtin_fma(-dn, k.lg2_lo, __builtin_fma(-dn, k.lg2_hi, x));
    const double t = __builtin_fma(u, k.ln10_hi, u * k.ln10_lo);
    double z = exp_tail(k.c, t, dn);
    z = (x > k.t_hi) ? __builtin_inf() : z;
    return (x < k.t_lo) ? 0.0 : z;
}

// e^y by exp10_k with literal constants: the disturbance programs' exp (wt_dst.hpp)
struct ExpK { __device__ __forceinline__ double operator()(double y) const { return exp10_k(kp_of(default_ktab()), y * wtd::LOG10_E); } };

// The junction program's pH arithmetic (wt_trn.hpp): H+ = 10^-pH as load_reactor takes the inlet's, and pH of a blended
// H+.  The device library's log10, inlined into the step kernel, keeps 10 to 18 more registers alive across the solver
// loop (its fp64 literals are hoisted out of the outer-step loop) and costs the n = 9..32 kernels 12 and 44 B of
// scratch; so -log10(H) is the root p of 10^-p = H by Newton's method on exp10_k, whose literals the kernel holds
// already: p <- p + (1 - H / 10^-p) / ln 10 from the hardware's fp32 log2.  The error squares per step (1e-6, 1e-12,
// then the floor); the floor is exp10_k's relative error over ln 10 plus the last sum's rounding, under 1 ulp(14).
struct JctK {
    __device__ __forceinline__ double exp10(double x) const { return exp10_k(kp_of(default_ktab()), x); }
    __device__ __forceinline__ double pH_of(double H) const
    {
        const KP k = kp_of(default_ktab());
        double p = -(double)(__builtin_amdgcn_logf((float)H) * 0.30103f);
#pragma unroll 1
        for (int i = 0; i < 4; ++i) p = p + (1.0 - H / exp10_k(k, -p)) / k.ln10_hi;
        return p;
    }
};

// The Radau constants of the solver sections, fetched the same way (radau.py:11-40 values, see rc::)
struct alignas(64) RTab {
    double T00, T01, T02, T10, T11, T12, rtol, atol;                 // section Z: Z = T W, norm scales
    double TI[9], mu_r, mu_cr, mu_ci, newton_tol, pad_n[3];           // section N: one Newton iteration
    double E0, E1, E2, pad_e[5];                                      // section E: error estimate
    double P[9], pad_a[7];                                            // section A: dense output of an accepted step
    double C0, C1, pad_g[6];                                          // section G: initial guess of an attempt
};
static_assert(sizeof(RTab) == 56 * 8, "RTab layout");
__host__ __device__ constexpr RTab default_rtab()
{
    RTab r{};
    r.T00 = rc::T00; r.T01 = rc::T01; r.T02 = rc::T02; r.T10 = rc::T10; r.T11 = rc::T11; r.T12 = rc::T12; r.rtol = RTOL; r.atol = ATOL;
    constexpr double ti[9] = {rc::TI00, rc::TI01, rc::TI02, rc::TI10, rc::TI11, rc::TI12, rc::TI20, rc::TI21, rc::TI22};
    constexpr double pm[9] = {rc::P00, rc::P01, rc::P02, rc::P10, rc::P11, rc::P12, rc::P20, rc::P21, rc::P22};
    for (int i = 0; i < 9; ++i) { r.TI[i] = ti[i]; r.P[i] = pm[i]; }
    r.mu_r = rc::MU_REAL; r.mu_cr = rc::MU_CR; r.mu_ci = rc::MU_CI; r.newton_tol = rc::NEWTON_TOL;
    r.E0 = rc::E0; r.E1 = rc::E1; r.E2 = rc::E2;
    r.C0 = rc::C0; r.C1 = rc::C1;
    return r;
}
struct KZ { double T00, T01, T02, T10, T11, T12, rtol, atol; };
struct KN { double TI[9], mu_r, mu_cr, mu_ci, newton_tol; };
struct KE { double E0, E1, E2; };
struct KA { double P[9]; };
struct KG { double C0, C1; };
typedef const __attribute__((address_space(4))) RTab *RTabPtr;
__device__ __forceinline__ KZ load_kz(RTabPtr t) { const d8 a = ((KVec)t)[0]; return {a[0], a[1], a[2], a[3], a[4], a[5], a[6], a[7]}; }
__device__ __forceinline__ KN load_kn(RTabPtr t)
{
    const d8 a = ((KVec)t)[1], b = ((KVec)t)[2];
    return {{a[0], a[1], a[2], a[3], a[4], a[5], a[6], a[7], b[0]}, b[1], b[2], b[3], b[4]};
}
__device__ __forceinline__ KE load_ke(RTabPtr t) { const d8 a = ((KVec)t)[3]; return {a[0], a[1], a[2]}; }
__device__ __forceinline__ KA load_ka(RTabPtr t)
{
    const d8 a = ((KVec)t)[4], b = ((KVec)t)[5];
    return {{a[0], a[1], a[2], a[3], a[4], a[5], a[6], a[7], b[0]}};
}
__device__ __forceinline__ KG load_kg(RTabPtr t) { const d8 a = ((KVec)t)[6]; return {a[0], a[1]}; }
// Literal constants for the error estimate and the accept block where loaded_constants_in_estimate_and_accept
// (wt_step.hpp) is off: with loaded ones and the expressions as written the compiler stops sharing their common
// subexpressions and fuses the remaining ones differently (last-bit changes; measured, tools/bits_check.py).  Where the
// switch is on the roundings are spelled out (z_of_w_spelled ... in wt_step.hpp) and the constants are loaded.
constexpr RTab RT0 = default_rtab();
__device__ __forceinline__ KZ lit_kz() { return {RT0.T00, RT0.T01, RT0.T02, RT0.T10, RT0.T11, RT0.T12, RT0.rtol, RT0.atol}; }
__device__ __forceinline__ KE lit_ke() { return {RT0.E0, RT0.E1, RT0.E2}; }
__device__ __forceinline__ KA lit_ka() { return {{RT0.P[0], RT0.P[1], RT0.P[2], RT0.P[3], RT0.P[4], RT0.P[5], RT0.P[6], RT0.P[7], RT0.P[8]}}; }
// Z = T W (radau.py:124) of species q: Z[2] = W0 + W1.  The caller brings the constants, literal or loaded (see above).
struct ZRow { double z0, z1, z2; };
__device__ __forceinline__ ZRow z_of_w(const KZ &kz, const double (&W)[3][3], int q)
{
    return {kz.T00 * W[0][q] + kz.T01 * W[1][q] + kz.T02 * W[2][q],
            kz.T10 * W[0][q] + kz.T11 * W[1][q] + kz.T12 * W[2][q],
            W[0][q] + W[1][q]};
}

} // namespace wt
