// wt_rhs.hpp -- the right-hand side, the reference's derivatives(): reactor.py:272-448 with thermodynamics.py:160-193,
// chemistry.py:400-437,483-523 and spatial.py:142-320.  The per-reactor constants (RK) and where they wait between
// evaluations (park_reactor / fetch_reactor), the zone-local properties for NS points at once, the pieces of a row,
// and the row-triple of one zone (rhs_rows, rhs_full).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "wt_tables.hpp"
#include "wt_lanes.hpp"

namespace wt {

// ---------------------------------------------------------------- reactor constants
struct RK {
    // chemistry.py:116-132 constants (frozen at configuration temperature)
    double Kw, Ka1, Ka1Ka2, KaH, cbeta;
    // transport / spatial: Richardson number (g drho dz) / (rho_avg u^2) against Ri_crit (spatial.py:262-277,293)
    double Kex, dz, u2, ricrit, rihulp, supp, unsupp;   // rihulp: half an ulp of Ri_crit
    // boundary-derived (reactor.py:336,349-368,385-395,426-443)
    double Qv, H_in, Cl_in, T_in, acid_dH, cl_dose, UAr, T_amb;
    double flowsum;   // inlet + acid + chlorine flow: ReactorState.flow_rate (reactor.py:497-501)
    bool has_acid, has_cl, has_heat;
    // the same, pre-masked for this lane's zone so the RHS needs no per-term selects:
    // inlet / dosing terms act on zone 0 only, the outlet sink on zone n-1 only
    double Kex_hi;    // Kex if this zone has an upper neighbour else 0
    double Qv_in;     // Qv in zone 0 else 0
    double Qv_out;    // Qv in zone n-1 else 0
    double acid0;     // acid dosing dH/dt in zone 0 (0 elsewhere / when off)
    double dose0;     // chlorine dosing in zone 0 (0 elsewhere / when off)
    double UAr_on;    // heat-loss coefficient (0 when off)
};

__device__ __forceinline__ double ulp_above_pos(double t) { return __longlong_as_double(__double_as_longlong(t) + 1) - t; }

// cmd != nullptr: boundary rows 0 / 4 / 6 (inlet, acid, chlorine flow) as the command path has just set them
__device__ __forceinline__ void load_reactor(const double *par, const double *bc, int64_t N, int64_t r, int n, RK &k,
                                             const double *cmd = nullptr, int cmd_stride = 0)
{
    auto P = [&](int row) { return par[(int64_t)row * N + r]; };
    auto B = [&](int row) {
        if (cmd && row == 0) return cmd[0 * cmd_stride];
        if (cmd && row == 4) return cmd[1 * cmd_stride];
        if (cmd && row == 6) return cmd[2 * cmd_stride];
        return bc[(int64_t)row * N + r];
    };
    const double V = P(0), height = P(1), diam = P(2);
    k.Kw = P(3); k.Ka1 = P(4); k.Ka1Ka2 = P(4) * P(5); k.KaH = P(6);
    k.cbeta = 2.303 * P(7);                    // chemistry.py:431-433
    k.Kex = P(8);
    const double u = P(9);
    k.dz = height / n;                          // spatial.py:119
    k.u2 = u * u;                               // velocity_scale ** 2
    // the three cases of the stratification switch folded into the two outcomes of one branch-free test
    // (rhs_rows): stratification off (reactor.py:310-315) -> factor 1 either way; velocity scale <= 1e-6 -> Ri = +inf,
    // stable either way (spatial.py:270-275); else Ri against Ri_crit picks between the two
    const int strat_mode = (P(10) != 0.0) ? ((u > 1e-6) ? 1 : 2) : 0;
    k.ricrit = P(11);
    k.rihulp = 0.5 * ulp_above_pos(k.ricrit);
    k.supp = (strat_mode != 0) ? P(12) : 1.0;        // interface factor where the Richardson test says "stable"
    k.unsupp = (strat_mode == 2) ? P(12) : 1.0;      // ... and where it does not
    const double Q_in = B(0);
    k.Qv = (Q_in / 60.0) / V;                   // reactor.py:336
    k.H_in = exp10_k(kp_of(default_ktab()), -B(1));   // reactor.py:363
    k.Cl_in = B(2); k.T_in = B(3);
    const double zone_volume_L = V / n;
    k.has_acid = B(4) > 0;
    k.acid_dH = ((B(4) / 60.0) * B(5)) / zone_volume_L; // reactor.py:350-354
    k.has_cl = B(6) > 0;
    k.cl_dose = ((B(6) / 60.0) * B(7)) / zone_volume_L; // reactor.py:388-392
    k.has_heat = B(9) > 0;
    const double PI = 3.141592653589793;
    const double rr = diam / 2;
    const double A_tot = PI * diam * height + 2 * PI * (rr * rr);  // reactor.py:429-431
    k.UAr = (B(9) * A_tot) / (998.2 * 4184 * (V / 1000));          // reactor.py:433-443
    k.T_amb = B(8);
    k.flowsum = B(0) + B(4) + B(6);
}

__device__ __forceinline__ void mask_reactor_for_lane(const Lane &L, RK &k)
{
    k.Kex_hi = L.has_hi ? k.Kex : 0.0;
    k.Qv_in = L.has_lo ? 0.0 : k.Qv;
    k.Qv_out = L.has_hi ? 0.0 : k.Qv;
    k.acid0 = (!L.has_lo && k.has_acid) ? k.acid_dH : 0.0;
    k.dose0 = (!L.has_lo && k.has_cl) ? k.cl_dose : 0.0;
    k.UAr_on = k.has_heat ? k.UAr : 0.0;
}

// The constants are needed by the RHS evaluations only.  Between them (factorisation, Newton solve, error
// estimate) they would occupy 38 VGPRs of a register file that is already oversubscribed, so they are parked
// in LDS and fetched at the top of every RHS block: 14 per-reactor words (one copy per reactor, broadcast to
// its lanes) and 5 per-lane ones (the inlet / outlet / neighbour masks applied once, at parking time).  Where LDS is
// short (n > 8: every slot is wanted for tridiagonal factors) the per-lane words are not parked but re-masked from
// four more per-reactor words at every fetch: ten v_and instead of three LDS reads.
constexpr int RK_UNI = 20, RK_LANE = 5, RK_MAXR = 32;   // up to 32 reactors per wavefront (n = 2)
// reactors per wavefront a kernel instantiation can meet: LV levels serve n in (2^(LV-1), 2^LV]
constexpr int rk_maxr(int LV) { return LV <= 1 ? 32 : 64 / ((1 << (LV - 1)) + 1); }
constexpr bool rk_lane_in_lds(int LV) { return LV < 4; }
constexpr int rk_lane_doubles(int LV) { return rk_lane_in_lds(LV) ? RK_LANE * 64 : 0; }
// uni[c * stride], lane[c * 64]: already offset for this lane; lane == nullptr: no per-lane words, use the masks
struct RKStore { double *uni; double *lane; int stride; uint32_t m_has_lo, m_has_hi; bool lane_lds; };   // lane_lds: a compile-time constant of the kernel
__device__ __forceinline__ double mask64(uint32_t m, double x) { return __hiloint2double(__double2hiint(x) & (int)m, __double2loint(x) & (int)m); }

__device__ __forceinline__ void park_reactor(const RKStore &st, const RK &k)
{
    const double u[RK_UNI] = {k.Kw, k.Ka1, k.Ka1Ka2, k.KaH, k.cbeta, k.dz, k.u2, k.supp, k.H_in, k.Cl_in, k.T_in, k.T_amb, k.UAr_on,
                              k.unsupp, k.ricrit, k.flowsum,
                              k.Kex, k.Qv, k.has_acid ? k.acid_dH : 0.0, k.has_cl ? k.cl_dose : 0.0};   // (rihulp is re-derived from ricrit)
    const double l[RK_LANE] = {k.Kex_hi, k.Qv_in, k.Qv_out, k.acid0, k.dose0};
#pragma unroll
    for (int c = 0; c < RK_UNI; ++c) st.uni[c * st.stride] = u[c];   // every lane of the reactor stores the same value
    if (st.lane_lds) {
#pragma unroll
        for (int c = 0; c < RK_LANE; ++c) st.lane[c * 64] = l[c];
    }
}

__device__ __forceinline__ RK fetch_reactor(const RKStore &st)
{
    RK k;
    k.Kw = st.uni[0 * st.stride]; k.Ka1 = st.uni[1 * st.stride]; k.Ka1Ka2 = st.uni[2 * st.stride]; k.KaH = st.uni[3 * st.stride];
    k.cbeta = st.uni[4 * st.stride]; k.dz = st.uni[5 * st.stride]; k.u2 = st.uni[6 * st.stride]; k.supp = st.uni[7 * st.stride];
    k.H_in = st.uni[8 * st.stride]; k.Cl_in = st.uni[9 * st.stride]; k.T_in = st.uni[10 * st.stride]; k.T_amb = st.uni[11 * st.stride];
    k.UAr_on = st.uni[12 * st.stride]; k.unsupp = st.uni[13 * st.stride]; k.ricrit = st.uni[14 * st.stride]; k.rihulp = 0.5 * ulp_above_pos(k.ricrit);
    if (st.lane_lds) {
        k.Kex_hi = st.lane[0 * 64]; k.Qv_in = st.lane[1 * 64]; k.Qv_out = st.lane[2 * 64]; k.acid0 = st.lane[3 * 64]; k.dose0 = st.lane[4 * 64];
    } else {   // the same values as mask_reactor_for_lane() made: zero where the zone has no such term
        const double Kex = st.uni[16 * st.stride], Qv = st.uni[17 * st.stride];
        k.Kex_hi = mask64(st.m_has_hi, Kex);
        k.Qv_in = mask64(~st.m_has_lo, Qv); k.Qv_out = mask64(~st.m_has_hi, Qv);
        k.acid0 = mask64(~st.m_has_lo, st.uni[18 * st.stride]); k.dose0 = mask64(~st.m_has_lo, st.uni[19 * st.stride]);
    }
    return k;
}

// ---------------------------------------------------------------- zone-local properties
struct PropPH { double H, iw, phi; bool bpos; }; // iw = 1/(beta*ln10)
struct PropT { double kT, rho; bool bad; };

// The RHS is inlined at several places of the solver (stage points, single points, the deferred f(y_new),
// the finite-difference passes) and the same state must give the same bits at each of them -- f(y0) of an outer
// step may come from any of them depending on the schedule.  So nothing here is left to the compiler's choice of
// which products to fuse: contraction is off and every fused multiply-add is spelled out.

// H = 10^-pH, buffering capacity beta (chemistry.py:400-437), HOCl/OCl- decay
// factor (chemistry.py:483-523).

// ---- the same arithmetic for NS points at once, step by step: consecutive instructions belong to different points and
// are independent (a dependent fp64 instruction issues after 8 cycles, an independent one after 5: tools/ubench/issue.hip)
#define WT_EACH _Pragma("unroll") for (int s = 0; s < NS; ++s)
// The compiler, short of registers, pulls each point's chain together again; an empty asm that "uses and redefines"
// the step's results makes every step complete for all points before the next one starts (NS = 1: nothing to do).
// BAR: the fence of a single-point evaluation is a scheduling barrier without operands.  The asm form takes the step's
// results as operands, and the hazard recognizer then puts an `s_nop 0` in front of it whenever the instruction before
// defines one of them: in a single-point evaluation that is after every step of the exponential's Horner chain.  One
// point has nothing to interleave and needs the fence only to keep its sections apart, which the barrier does too.
// (For two and more points the barrier lets the compiler pull the chains together again and spills SGPRs inside the
// trip loop: they always keep the asm form.)  The caller chooses: single_point_fence_is_barrier in wt_step.hpp.
template <bool BAR, int NS> __device__ __forceinline__ void row_fence(double (&v)[NS])
{
    // (one point: nothing to interleave, but the fence keeps the compiler from merging this section with the next)
    if constexpr (BAR && NS == 1) __builtin_amdgcn_sched_barrier(0);
    else if constexpr (NS == 1) asm volatile("" : "+v"(v[0]));
    if constexpr (NS == 2) asm volatile("" : "+v"(v[0]), "+v"(v[1]));
    if constexpr (NS == 3) asm volatile("" : "+v"(v[0]), "+v"(v[1]), "+v"(v[2]));
    if constexpr (NS == 4) asm volatile("" : "+v"(v[0]), "+v"(v[1]), "+v"(v[2]), "+v"(v[3]));
}
template <int NS, bool BAR = false> __device__ __forceinline__ void rcp_n(const double (&x)[NS], double (&r)[NS])
{
    double e[NS];
    WT_EACH r[s] = __builtin_amdgcn_rcp(x[s]); row_fence<BAR>(r);
    WT_EACH e[s] = __builtin_fma(-x[s], r[s], 1.0); row_fence<BAR>(e);
    WT_EACH r[s] = __builtin_fma(r[s], e[s], r[s]); row_fence<BAR>(r);
    WT_EACH e[s] = __builtin_fma(-x[s], r[s], 1.0); row_fence<BAR>(e);
    WT_EACH r[s] = __builtin_fma(r[s], e[s], r[s]); row_fence<BAR>(r);
}
template <int NS, bool BAR = false> __device__ __forceinline__ void exp_tail_n(const double c[10], const double (&t)[NS], const double (&dn)[NS], double (&z)[NS])
{
    double p[NS];
    WT_EACH p[s] = c[0];
#pragma unroll
    for (int i = 1; i < 10; ++i) { WT_EACH p[s] = __builtin_fma(t[s], p[s], c[i]); row_fence<BAR>(p); }
    WT_EACH p[s] = __builtin_fma(t[s], p[s], 1.0); row_fence<BAR>(p);
    WT_EACH p[s] = __builtin_fma(t[s], p[s], 1.0); row_fence<BAR>(p);
    WT_EACH z[s] = __builtin_amdgcn_ldexp(p[s], (int)dn[s]); row_fence<BAR>(z);
}
template <int NS, bool BAR = false> __device__ __forceinline__ void prop_pH_n(const KP &c, const RK &k, const double (&pH)[NS], PropPH (&p)[NS])
{
#pragma clang fp contract(off)
    double x[NS], dn[NS], u[NS], t[NS], H[NS];
    WT_EACH x[s] = -pH[s];
    WT_EACH dn[s] = __builtin_rint(x[s] * c.log2_10); row_fence<BAR>(dn);
    WT_EACH u[s] = __builtin_fma(-dn[s], c.lg2_hi, x[s]); row_fence<BAR>(u);
    WT_EACH u[s] = __builtin_fma(-dn[s], c.lg2_lo, u[s]); row_fence<BAR>(u);
    WT_EACH t[s] = u[s] * c.ln10_lo; row_fence<BAR>(t);
    WT_EACH t[s] = __builtin_fma(u[s], c.ln10_hi, t[s]); row_fence<BAR>(t);
    exp_tail_n<NS, BAR>(c.c, t, dn, H);
    WT_EACH H[s] = (x[s] > c.t_hi) ? __builtin_inf() : H[s];
    WT_EACH H[s] = (x[s] < c.t_lo) ? 0.0 : H[s];
    double iH[NS], H2[NS], D[NS], iD[NS], HK[NS], iHK[NS];
    WT_EACH H2[s] = H[s] * H[s];
    WT_EACH D[s] = __builtin_fma(k.Ka1, H[s], H2[s]) + k.Ka1Ka2;
    WT_EACH HK[s] = H[s] + k.KaH;
    rcp_n<NS, BAR>(H, iH); rcp_n<NS, BAR>(D, iD); rcp_n<NS, BAR>(HK, iHK);
    double bw[NS], a0[NS], a1[NS], a2[NS], mix[NS], beta[NS], bl[NS], ib[NS];
    WT_EACH bw[s] = c.c2303 * __builtin_fma(k.Kw, iH[s], H[s]);
    WT_EACH a0[s] = H2[s] * iD[s];
    WT_EACH a1[s] = (k.Ka1 * H[s]) * iD[s];
    WT_EACH a2[s] = k.Ka1Ka2 * iD[s];
    WT_EACH mix[s] = __builtin_fma(a0[s], a2[s], __builtin_fma(4 * a1[s], a2[s], a0[s] * a1[s]));
    WT_EACH beta[s] = __builtin_fma(k.cbeta, mix[s], bw[s]);
    WT_EACH bl[s] = beta[s] * c.ln10;
    rcp_n<NS, BAR>(bl, ib);
    WT_EACH {
        p[s].bpos = beta[s] > 0;                    // reactor.py:358,367,375 guards: no pH change unless beta > 0
        p[s].iw = p[s].bpos ? ib[s] : 0.0;
        p[s].phi = __builtin_fma(k.KaH * iHK[s], c.c002, H[s] * iHK[s]);
        p[s].H = H[s];
    }
}
template <int NS, bool BAR = false> __device__ __forceinline__ void prop_T_n(const KT &c, const double (&T)[NS], PropT (&p)[NS])
{
#pragma clang fp contract(off)
    double tk[NS], itk[NS], ex[NS], dn[NS], t[NS], z[NS];
    WT_EACH tk[s] = T[s] + c.c27315;
    rcp_n<NS, BAR>(tk, itk);
    WT_EACH ex[s] = c.k_arr * (itk[s] - c.inv_tref);
    WT_EACH dn[s] = __builtin_rint(ex[s] * c.log2e); row_fence<BAR>(dn);
    WT_EACH t[s] = __builtin_fma(-dn[s], c.ln2_hi, ex[s]); row_fence<BAR>(t);
    WT_EACH t[s] = __builtin_fma(-dn[s], c.ln2_lo, t[s]); row_fence<BAR>(t);
    exp_tail_n<NS, BAR>(c.c, t, dn, z);
    WT_EACH z[s] = (ex[s] > c.e_hi) ? __builtin_inf() : z[s];
    WT_EACH z[s] = (ex[s] < c.e_lo) ? 0.0 : z[s];
    WT_EACH {
        p[s].bad = (T[s] < 0.0) || (T[s] > c.c100);
        p[s].kT = c.c1em4 * z[s];
        const double d = T[s] - 4.0;
        const double cold = c.rho_max + (c.rho_an * (d * d));
        const double warm = c.rho20 + (c.rho_sl * (T[s] - c.c20));
        p[s].rho = (T[s] <= c.c8) ? cold : warm;
    }
}

// H = 10^-pH, buffering capacity beta (chemistry.py:400-437), HOCl/OCl- decay factor (chemistry.py:483-523).
template <bool BAR = false> __device__ __forceinline__ PropPH prop_pH(const KP &c, const RK &k, double pH)
{
    const double x[1] = {pH}; PropPH p[1];
    prop_pH_n<1, BAR>(c, k, x, p);
    return p[0];
}

// Arrhenius decay rate (thermodynamics.py:160-193) with its [0,100] C check
// (:146-157) and water density (spatial.py:177-189).  The density feeds the stratification switch, so it
// is formed with the reference's roundings: products and sums separately, never fused.
template <bool BAR = false> __device__ __forceinline__ PropT prop_T(const KT &c, double T)
{
    const double x[1] = {T}; PropT p[1];
    prop_T_n<1, BAR>(c, x, p);
    return p[0];
}

// One row-triple (dpH, dCl, dT) of derivatives() for this lane's zone, given the
// lane's own (possibly perturbed / stage) values; neighbour values come from the
// adjacent lanes' arguments to the same call.  reactor.py:304-443.
// Cross-lane moves are executed by every lane of the segment, then masked.
// The pieces of a row, shared by rhs_rows and the finite-difference passes (one rounding behaviour per expression).
// Interface factor above this zone: K[i,i+1] = Kex * suppression(rho_i, rho_{i+1})  (spatial.py:239-320, reactor.py:321-325).
// The reference compares the correctly rounded quotient Ri = num / den, num = (g drho) dz, den = rho_avg u^2 > 0, with
// Ri_crit.  fl(num / den) > c  <=>  num / den > c + ulp(c)/2  <=>  num - c den > (ulp(c)/2) den, and the left side is
// exact in one fma whenever the two sides are close enough for rounding to matter: the same decision as the
// reference's on the same bits, without a division.  Stratification off / velocity scale <= 1e-6 (Ri = +inf) are
// folded into the two outcomes (load_reactor).
__device__ __forceinline__ double k_above(const RK &k, double rho, double rho_hi)
{
#pragma clang fp contract(off)
    const double drho = rho_hi - rho;
    const double ravg = 0.5 * (rho + rho_hi);
    const double num = (9.81 * drho) * k.dz, den = ravg * k.u2;
    const double s = (__builtin_fma(-k.ricrit, den, num) > k.rihulp * den) ? k.supp : k.unsupp;
    return k.Kex_hi * s;                                   // 0 above the top zone
}
// K @ x the way OpenBLAS' dgemv accumulates it inside the reference: neighbours first, diagonal last, every product
// rounded before it is added (pinned by tests/golden/g2_rhs_*.npz: temperature rows bit-identical).
__device__ __forceinline__ double k_diag(const RK &k, double k_lo, double k_hi)
{
#pragma clang fp contract(off)
    return -(k_lo + k_hi) - k.Qv_out;                      // reactor.py:329-337
}
__device__ __forceinline__ double mix3(double k_lo, double k_hi, double kd, double x_lo, double x_hi, double x)
{
#pragma clang fp contract(off)
    return (k_lo * x_lo + k_hi * x_hi) + kd * x;
}
// zone-0 dosing and inlet (reactor.py:349-368,388-395,420) through pre-masked coefficients; iw is 0 when the
// reference's `beta > 0` guard fails
__device__ __forceinline__ double row_pH(const RK &k, double mixH, double H, double iw)
{
#pragma clang fp contract(off)
    return -(__builtin_fma(k.Qv_in, k.H_in - H, k.acid0) + mixH) * iw;                        // reactor.py:349-376
}
__device__ __forceinline__ double row_Cl(const RK &k, double mixC, double Cl, double kphi)
{
#pragma clang fp contract(off)
    return __builtin_fma(-kphi, Cl, __builtin_fma(k.Qv_in, k.Cl_in - Cl, k.dose0) + mixC);    // reactor.py:385-411
}
__device__ __forceinline__ double row_T(const RK &k, double mixT, double T)
{
#pragma clang fp contract(off)
    return __builtin_fma(-k.UAr_on, T - k.T_amb, k.Qv_in * (k.T_in - T) + mixT);               // reactor.py:420-443
}

// One row-triple (dpH, dCl, dT) of derivatives() for this lane's zone, given the
// lane's own (possibly stage) values; neighbour values come from the
// adjacent lanes' arguments to the same call.  reactor.py:304-443.
// Cross-lane moves are executed by every lane of the segment, then masked.
template <bool ROW>
__device__ __forceinline__ void rhs_rows(const Lane &L, const RK &k, double H, double iw, bool bpos, double kphi,
                                         double rho, double Cl, double T, double f[3])
{
    const double k_hi = k_above(k, rho, from_hi<ROW, 1>(L, rho));       // K[i,i+1]
    const double k_lo = keep_m(L.m_lo[0], from_lo<ROW, 1>(L, k_hi));    // K[i,i-1] (bound_ctrl gives 0 below zone 0 of lane 0)
    const double kd = k_diag(k, k_lo, k_hi);
    const double H_lo = keep_m(L.m_lo[0], from_lo<ROW, 1>(L, H)), H_hi = keep_m(L.m_hi[0], from_hi<ROW, 1>(L, H));
    const double C_lo = keep_m(L.m_lo[0], from_lo<ROW, 1>(L, Cl)), C_hi = keep_m(L.m_hi[0], from_hi<ROW, 1>(L, Cl));
    const double T_lo = keep_m(L.m_lo[0], from_lo<ROW, 1>(L, T)), T_hi = keep_m(L.m_hi[0], from_hi<ROW, 1>(L, T));
    // k_lo / k_hi are exactly 0 where there is no neighbour, and what was read there is finite (keep_m)
    (void)bpos;
    f[SPH] = row_pH(k, mix3(k_lo, k_hi, kd, H_lo, H_hi, H), H, iw);
    f[SCL] = row_Cl(k, mix3(k_lo, k_hi, kd, C_lo, C_hi, Cl), Cl, kphi);
    f[STT] = row_T(k, mix3(k_lo, k_hi, kd, T_lo, T_hi, T), T);
}

template <bool ROW>
__device__ __forceinline__ bool rhs_full(const Lane &L, const KP &cp, const KT &ct, const RK &k, const double y[3], double f[3])
{
    const PropPH pp = prop_pH(cp, k, y[SPH]);
    const PropT pt = prop_T(ct, y[STT]);
    rhs_rows<ROW>(L, k, pp.H, pp.iw, pp.bpos, pt.kT * pp.phi, pt.rho, y[SCL], y[STT], f);
    return pt.bad;
}

} // namespace wt
