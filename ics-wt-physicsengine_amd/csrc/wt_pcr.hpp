// wt_pcr.hpp -- the linear algebra of a Newton iteration (radau.py:84-134).  With unknowns ordered [T | pH | Cl] the
// Jacobian is block lower-triangular with tridiagonal diagonal blocks, so (mu/h I - J) x = b is three tridiagonal
// solves: the Jacobian bands (Jac, and JacA: the same held in accumulation registers), the store of the factors
// (FStore: LDS, registers for what does not fit), the parallel-cyclic-reduction factorisation of the real-shift and
// the complex-shift systems, and the two solves (solve_real, solve_rc).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "wt_tables.hpp"
#include "wt_lanes.hpp"
#include "wt_rhs.hpp"

namespace wt {

// ---------------------------------------------------------------- Jacobian bands
// Non-zero structure of d(dpH,dCl,dT)_i / d(pH,Cl,T)_j, j in {i-1,i,i+1}
// (index rel+1).  dT rows see only T; dpH rows see pH and (through the
// stratification switch only) T; dCl rows see Cl, own-zone pH and T.
struct Jac {
    double pp[3], cc[3], tt[3], pt[3], ct[3], cp;
};
// Loop-carried state that is written rarely and read rarely, held in ACCUMULATION registers by name: the register
// file of a lone wavefront has 512 registers of which the VALU addresses 256, and what the allocator keeps beyond
// them it shuffles through `v_accvgpr` copies at the head of the solver loop -- on EVERY trip, whether the value is
// touched or not.  A value that lives in an AGPR by constraint costs its copies where it is written and where it is
// read, nothing in between.  (Writes are VALU instructions: under a lane mask they update the active lanes only.)
// (A = false: an ordinary variable -- the n > 16 kernels, at 480-512 registers, answer 74 pinned AGPRs with scratch;
// the n = 17...32 kernel takes the 42 of everything but the Jacobian)
template <bool A> struct Held;
template <> struct Held<false> {
    double v;
    __device__ __forceinline__ void init() { v = 0.0; }
    __device__ __forceinline__ void set(double x) { v = x; }
    __device__ __forceinline__ double get() const { return v; }
};
template <> struct Held<true> {
    int lo, hi;
    __device__ __forceinline__ void init() { asm volatile("" : "=a"(lo), "=a"(hi)); }     // (defined, value irrelevant)
    __device__ __forceinline__ void set(double x)
    {
        asm volatile("v_accvgpr_write_b32 %0, %2\n\tv_accvgpr_write_b32 %1, %3" : "+a"(lo), "+a"(hi) : "v"(__double2loint(x)), "v"(__double2hiint(x)));
    }
    __device__ __forceinline__ double get() const
    {
        int l, h;
        asm("v_accvgpr_read_b32 %0, %2\n\tv_accvgpr_read_b32 %1, %3" : "=v"(l), "=v"(h) : "a"(lo), "a"(hi));
        return __hiloint2double(h, l);
    }
};
template <bool A> struct JacA {
    Held<A> e[16];     // tt[3], pp[3], cc[3] | pt[3], ct[3], cp
    __device__ __forceinline__ void init() {
#pragma unroll
        for (int i = 0; i < 16; ++i) e[i].init();
    }
    __device__ __forceinline__ void put(const Jac &J)
    {
#pragma unroll
        for (int r = 0; r < 3; ++r) { e[r].set(J.tt[r]); e[3 + r].set(J.pp[r]); e[6 + r].set(J.cc[r]); e[9 + r].set(J.pt[r]); e[12 + r].set(J.ct[r]); }
        e[15].set(J.cp);
    }
    __device__ __forceinline__ void bands(Jac &J) const
    {
#pragma unroll
        for (int r = 0; r < 3; ++r) { J.tt[r] = e[r].get(); J.pp[r] = e[3 + r].get(); J.cc[r] = e[6 + r].get(); }
    }
    __device__ __forceinline__ void coupling(Jac &J) const
    {
#pragma unroll
        for (int r = 0; r < 3; ++r) { J.pt[r] = e[9 + r].get(); J.ct[r] = e[12 + r].get(); }
        J.cp = e[15].get();
    }
};

// The inter-zone exchange depends on temperature through the stratification switch only, a step function: unless a
// finite-difference perturbation happens to flip a switch, the pH rows do not see T at all and the Cl rows see their
// own zone's T only (the Arrhenius rate) -- exact zeros, column by column.  A wavefront whose lanes all find them zero
// skips the neighbours' T increments in every solve (12 cross-lane moves and 15 fused multiply-adds of a Newton
// iteration): adding the exact zeros would not change a bit.
__device__ __forceinline__ bool jac_t_dense(const Jac &J)
{
    return (J.pt[0] != 0.0) || (J.pt[1] != 0.0) || (J.pt[2] != 0.0) || (J.ct[0] != 0.0) || (J.ct[2] != 0.0);
}

// PCR-factored tridiagonal systems (real and complex shift) live in LDS, not in registers: pair-major
// [pair of slots][64 lanes] 16-byte cells (FStore below), conflict-free ds_read_b128 / ds_write_b128.
// A factor is written once per (h, J) and read once per solve.
// For n > 16 (LV >= 5) the store outgrows what a wavefront may have of the CU's 160 KiB at four wavefronts per CU:
// the first NREG slots (real-shift factors) stay in registers instead -- exactly as many as do not fit.  All of them
// in LDS means three wavefronts per CU and 0.55-0.6x the throughput (measured at n = 20 and n = 40); all real-shift
// factors in registers costs scratch spills (n <= 32) or more of them (n > 32: 292 B against 176 B, -1 %).
constexpr int fstore_total_slots(int LV) { return 3 * (2 * LV) + 3 * (4 * LV); }
constexpr int fstore_lds_slots(int LV)
{
    const int budget = 40960;                                  // bytes per wavefront at four per CU
    const int fixed = ((RK_UNI * rk_maxr(LV) + rk_lane_doubles(LV) + rk_maxr(LV) + 64 + 1) & ~1) * 8;   // LdsMap: reactor constants, history base, reactor indices, exchange row (F_OFF)
    const int fit = ((budget - fixed) / 512) & ~1;                 // slots are stored as pairs
    return fit < fstore_total_slots(LV) ? fit : fstore_total_slots(LV);
}
typedef double __attribute__((ext_vector_type(2))) double2v;
typedef __attribute__((address_space(3))) double2v LdsDouble2;
template <int LV> struct FStore {
    static constexpr int NREG = fstore_total_slots(LV) - fstore_lds_slots(LV);   // slots [0, NREG) in registers
    static_assert(NREG % 2 == 0, "slots come in pairs");
    double reg[NREG > 0 ? NREG : 1];
    // Slots live in LDS as PAIRS (2j, 2j + 1) -- (alpha, gamma) of a level, (re, im) of a complex factor, (top factor,
    // 1/d) -- one 16-byte cell per pair and lane, pair-major: cell[(pair) * 64 + lane].  A pair is written and read
    // together with one ds_write_b128 / ds_read_b128: the read costs half of a two-address ds_read2st64_b64
    // (16 vs 32 cycles per wavefront with the CU's four wavefronts on its LDS pipe: tools/ubench/lds.hip).
    LdsDouble2 *cell;   // this lane's column of pairs: cell[pair * 64]
    // `slot` is a compile-time constant at every call site after inlining / unrolling
    __device__ __forceinline__ double ld(int slot) const
    {
        if (slot < NREG) return reg[slot < NREG ? slot : 0];
        const LdsDouble *p = (const LdsDouble *)(cell + ((slot - NREG) >> 1) * 64);
        return p[(slot - NREG) & 1];
    }
    __device__ __forceinline__ void ld2(int slot, double &a, double &b) const      // slot even
    {
        if (slot < NREG) { a = reg[slot < NREG ? slot : 0]; b = reg[slot + 1 < NREG ? slot + 1 : 0]; return; }
        const double2v v = cell[((slot - NREG) >> 1) * 64];
        a = v.x; b = v.y;
    }
    __device__ __forceinline__ void st2(int slot, double a, double b)             // slot even
    {
        if (slot < NREG) { reg[slot < NREG ? slot : 0] = a; reg[slot + 1 < NREG ? slot + 1 : 0] = b; return; }
        double2v v; v.x = a; v.y = b;
        cell[((slot - NREG) >> 1) * 64] = v;
    }
};
// slot map: real system k (0..2): [k RS + 2l] = alpha_l, [+2l+1] = gamma_l for the levels l < LV-1 below the top one,
//           [+2(LV-1)] = the top level's one factor (alpha for zones >= 2^(LV-1), gamma below: never both), [+2LV-1] = 1/d
//           complex system k: CB + k CS + 4l + {0,1,2,3} = al.r, al.i, ga.r, ga.i; [+4(LV-1), +1] = top factor, [+2, +3] = 1/d
template <int LV> struct FSlots {
    static constexpr int RS = 2 * LV, CS = 4 * LV, CB = 3 * RS, TOTAL = 3 * RS + 3 * CS;
    static constexpr int LDS_SLOTS = TOTAL - FStore<LV>::NREG;
};

struct cplx { double r, i; };
// (which product is fused is spelled out: the same solve is inlined in alternative paths -- the systems one by one or
// two in lock step -- and a reactor must get the same bits whichever its wavefront takes)
__device__ __forceinline__ cplx cmul(cplx a, cplx b)
{
#pragma clang fp contract(off)
    return {__builtin_fma(a.r, b.r, -(a.i * b.i)), __builtin_fma(a.r, b.i, a.i * b.r)};
}
__device__ __forceinline__ cplx cinv(cplx a)
{
#pragma clang fp contract(off)
    const double q = rcp(__builtin_fma(a.r, a.r, a.i * a.i));
    return {a.r * q, -a.i * q};
}

template <bool ROW, int S> __device__ __forceinline__ cplx cfrom_lo(const Lane &L, cplx a) { return {from_lo<ROW, S>(L, a.r), from_lo<ROW, S>(L, a.i)}; }
template <bool ROW, int S> __device__ __forceinline__ cplx cfrom_hi(const Lane &L, cplx a) { return {from_hi<ROW, S>(L, a.r), from_hi<ROW, S>(L, a.i)}; }
template <bool ROW, int S> __device__ __forceinline__ void cboth(const Lane &L, cplx a, cplx &lo, cplx &hi)
{
    both<ROW, S>(L, a.r, lo.r, hi.r); both<ROW, S>(L, a.i, lo.i, hi.i);
}

// One cyclic-reduction level of all six systems (three real, three complex shift) at once: the
// six eliminations are independent, so issuing them together hides the reciprocal / DPP latency
// of each behind the others.
template <bool ROW, int LV, int l>
__device__ __forceinline__ void pcr_factor_level_all(const Lane &L, double ar[3], double dr[3], double cr[3],
                                                     cplx ac[3], cplx dc[3], cplx cc[3], FStore<LV> &F)
{
    using S = FSlots<LV>;
    constexpr int s = 1 << l;
    if constexpr (l == 0) {
        // Level 0: the off-diagonals of the complex-shift systems are still the real ones (-J's bands, imaginary part
        // exactly 0), so their neighbours' values are the real systems' (moved once, not three times) and every
        // product with a zero imaginary part drops out -- the same bits with 16 cross-lane moves and 14 fp64
        // instructions less per system.
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const double a0 = ar[k], c0 = cr[k];
            const double id = rcp(dr[k]);
            const double id_lo = from_lo<ROW, s>(L, id), id_hi = from_hi<ROW, s>(L, id);
            const double a_lo = keep_m(L.m_lo[l], from_lo<ROW, s>(L, a0)), c_lo = keep_m(L.m_lo[l], from_lo<ROW, s>(L, c0));
            const double a_hi = keep_m(L.m_hi[l], from_hi<ROW, s>(L, a0)), c_hi = keep_m(L.m_hi[l], from_hi<ROW, s>(L, c0));
            const double al = a0 * keep_m(L.m_lo[l], id_lo);
            const double ga = c0 * keep_m(L.m_hi[l], id_hi);
            dr[k] = dr[k] - al * c_lo - ga * a_hi;
            ar[k] = -al * a_lo;
            cr[k] = -ga * c_hi;
            F.st2(k * S::RS + 2 * l, al, ga);
            // complex shift: alpha = a / d_lo, gamma = c / d_hi with real a, c
            const cplx cid = cinv(dc[k]);
            const cplx i_lo = cfrom_lo<ROW, s>(L, cid), i_hi = cfrom_hi<ROW, s>(L, cid);
            const cplx il = {keep_m(L.m_lo[l], i_lo.r), keep_m(L.m_lo[l], i_lo.i)};
            const cplx ih = {keep_m(L.m_hi[l], i_hi.r), keep_m(L.m_hi[l], i_hi.i)};
            const cplx cal = {a0 * il.r, a0 * il.i};
            const cplx cga = {c0 * ih.r, c0 * ih.i};
            double dre = dc[k].r, dim = dc[k].i;
            dre = __builtin_fma(-cal.r, c_lo, dre); dim = __builtin_fma(-cal.i, c_lo, dim);
            dre = __builtin_fma(-cga.r, a_hi, dre); dim = __builtin_fma(-cga.i, a_hi, dim);
            dc[k] = {dre, dim};
            ac[k] = {-(cal.r * a_lo), -(cal.i * a_lo)};
            cc[k] = {-(cga.r * c_hi), -(cga.i * c_hi)};
            const int c0s = S::CB + k * S::CS + 4 * l;
            F.st2(c0s, cal.r, cal.i); F.st2(c0s + 2, cga.r, cga.i);
        }
        if constexpr (l + 2 < LV) pcr_factor_level_all<ROW, LV, l + 1>(L, ar, dr, cr, ac, dc, cc, F);
        return;
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        // real shift.  Every lane inverts its own diagonal once and the neighbours fetch the reciprocal (the same
        // bits as inverting the fetched diagonal on both sides, half the reciprocals)
        const double id = rcp(dr[k]);
        double id_lo, id_hi, a_lo, a_hi, c_lo, c_hi;
        both<ROW, s>(L, id, id_lo, id_hi); both<ROW, s>(L, ar[k], a_lo, a_hi); both<ROW, s>(L, cr[k], c_lo, c_hi);
        // a == 0 where there is no lower neighbour (c likewise), so alpha/gamma vanish there by
        // themselves once the foreign operands are finite (keep_m folds into the cross-lane move)
        const double al = ar[k] * keep_m(L.m_lo[l], id_lo);
        const double ga = cr[k] * keep_m(L.m_hi[l], id_hi);
        dr[k] = dr[k] - al * keep_m(L.m_lo[l], c_lo) - ga * keep_m(L.m_hi[l], a_hi);
        ar[k] = -al * keep_m(L.m_lo[l], a_lo);
        cr[k] = -ga * keep_m(L.m_hi[l], c_hi);
        F.st2(k * S::RS + 2 * l, al, ga);
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        // complex shift, likewise
        const cplx cid = cinv(dc[k]);
        cplx i_lo, i_hi, a_lo, a_hi, c_lo, c_hi;
        cboth<ROW, s>(L, cid, i_lo, i_hi); cboth<ROW, s>(L, ac[k], a_lo, a_hi); cboth<ROW, s>(L, cc[k], c_lo, c_hi);
        const cplx il = {keep_m(L.m_lo[l], i_lo.r), keep_m(L.m_lo[l], i_lo.i)};
        const cplx ih = {keep_m(L.m_hi[l], i_hi.r), keep_m(L.m_hi[l], i_hi.i)};
        const cplx al = cmul(ac[k], il);
        const cplx ga = cmul(cc[k], ih);
        {   // d -= al * c_lo + ga * a_hi, eight fused multiply-adds
            const cplx cl = {keep_m(L.m_lo[l], c_lo.r), keep_m(L.m_lo[l], c_lo.i)};
            const cplx ah = {keep_m(L.m_hi[l], a_hi.r), keep_m(L.m_hi[l], a_hi.i)};
            double dre = dc[k].r, dim = dc[k].i;
            dre = __builtin_fma(-al.r, cl.r, dre); dim = __builtin_fma(-al.r, cl.i, dim);
            dre = __builtin_fma(al.i, cl.i, dre);  dim = __builtin_fma(-al.i, cl.r, dim);
            dre = __builtin_fma(-ga.r, ah.r, dre); dim = __builtin_fma(-ga.r, ah.i, dim);
            dre = __builtin_fma(ga.i, ah.i, dre);  dim = __builtin_fma(-ga.i, ah.r, dim);
            dc[k] = {dre, dim};
        }
        const cplx na = cmul(al, {keep_m(L.m_lo[l], a_lo.r), keep_m(L.m_lo[l], a_lo.i)});
        const cplx nc = cmul(ga, {keep_m(L.m_hi[l], c_hi.r), keep_m(L.m_hi[l], c_hi.i)});
        ac[k] = {-na.r, -na.i};
        cc[k] = {-nc.r, -nc.i};
        const int c0 = S::CB + k * S::CS + 4 * l;
        F.st2(c0, al.r, al.i); F.st2(c0 + 2, ga.r, ga.i);
    }
    if constexpr (l + 2 < LV) pcr_factor_level_all<ROW, LV, l + 1>(L, ar, dr, cr, ac, dc, cc, F);
}

// The top level (stride 2^(LV-1) >= n/2): a zone couples to its one partner only -- `a` is zero below the stride, `c`
// at and above it, so a + c is whichever is there (exactly), and the partner's a + c the coefficient that couples
// back.  One factor and a third of the cross-lane moves of a regular level; the same bits.
template <bool ROW, int LV>
__device__ __forceinline__ void pcr_factor_top_all(const Lane &L, double ar[3], double dr[3], double cr[3],
                                                   cplx ac[3], cplx dc[3], cplx cc[3], FStore<LV> &F, double ftop[3])
{
    using S = FSlots<LV>;
    constexpr int s = 1 << (LV - 1);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double id = rcp(dr[k]), w = ar[k] + cr[k];
        const double p_id = from_partner<ROW, s>(L, id), p_w = from_partner<ROW, s>(L, w);
        const double f = w * p_id;
        dr[k] = dr[k] - f * p_w;
        ftop[k] = f;                                  // stored with 1/d, its pair (factorize)
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const cplx cid = cinv(dc[k]), w = {ac[k].r + cc[k].r, ac[k].i + cc[k].i};
        const cplx p_id = {from_partner<ROW, s>(L, cid.r), from_partner<ROW, s>(L, cid.i)};
        const cplx p_w = {from_partner<ROW, s>(L, w.r), from_partner<ROW, s>(L, w.i)};
        const cplx f = cmul(w, p_id);
        double dre = dc[k].r, dim = dc[k].i;
        dre = __builtin_fma(-f.r, p_w.r, dre); dim = __builtin_fma(-f.r, p_w.i, dim);
        dre = __builtin_fma(f.i, p_w.i, dre);  dim = __builtin_fma(-f.i, p_w.r, dim);
        dc[k] = {dre, dim};
        const int c0 = S::CB + k * S::CS + 4 * (LV - 1);
        F.st2(c0, f.r, f.i);
    }
}

// The six factored systems of one (h, J) pair: scipy's LU_real / LU_complex.
template <bool ROW, int LV>
__device__ __forceinline__ void factorize(const Lane &L, const Jac &J, double h, FStore<LV> &F)
{
    using S = FSlots<LV>;
    // radau.py:454-456: MU_REAL / h * I - J ; MU_COMPLEX / h * I - J   (systems: 0 = T, 1 = pH, 2 = Cl)
    const double ih = rcp(h);
    const double mr = rc::MU_REAL * ih, mcr = rc::MU_CR * ih, mci = rc::MU_CI * ih;
    double ar[3] = {-J.tt[0], -J.pp[0], -J.cc[0]};
    double dr[3] = {mr - J.tt[1], mr - J.pp[1], mr - J.cc[1]};
    double cr[3] = {-J.tt[2], -J.pp[2], -J.cc[2]};
    cplx ac[3] = {{ar[0], 0.0}, {ar[1], 0.0}, {ar[2], 0.0}};
    cplx dc[3] = {{mcr - J.tt[1], mci}, {mcr - J.pp[1], mci}, {mcr - J.cc[1], mci}};
    cplx cc[3] = {{cr[0], 0.0}, {cr[1], 0.0}, {cr[2], 0.0}};
    if constexpr (LV > 1) pcr_factor_level_all<ROW, LV, 0>(L, ar, dr, cr, ac, dc, cc, F);
    double ftop[3];
    pcr_factor_top_all<ROW, LV>(L, ar, dr, cr, ac, dc, cc, F, ftop);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        F.st2(k * S::RS + 2 * (LV - 1), ftop[k], rcp(dr[k]));
        const cplx inv = cinv(dc[k]);
        F.st2(S::CB + k * S::CS + 4 * LV - 2, inv.r, inv.i);
    }
}

// x = (mu_real/h I - J)^-1 b, in place, b indexed by species.  The factors of all three systems are
// fetched from LDS in one batch up front (one exposed LDS round trip instead of one per level).
template <int LV> struct RealFactors { double a[LV > 1 ? LV - 1 : 1], g[LV > 1 ? LV - 1 : 1], f, inv; };

template <int LV>
__device__ __forceinline__ void load_real(const FStore<LV> &F, int k, RealFactors<LV> &s)
{
    using S = FSlots<LV>;
#pragma unroll
    for (int l = 0; l + 1 < LV; ++l) F.ld2(k * S::RS + 2 * l, s.a[l], s.g[l]);
    F.ld2(k * S::RS + 2 * (LV - 1), s.f, s.inv);
}

template <bool ROW, int LV, int l>
__device__ __forceinline__ void pcr_real_level(const Lane &L, const RealFactors<LV> &s, double &b)
{
    if constexpr (l + 1 < LV) {
        constexpr int st = 1 << l;
        double b_lo, b_hi;
        both<ROW, st>(L, b, b_lo, b_hi);
        b = b - s.a[l] * keep_m(L.m_lo[l], b_lo) - s.g[l] * keep_m(L.m_hi[l], b_hi);
        pcr_real_level<ROW, LV, l + 1>(L, s, b);
    } else {
        b = b - s.f * from_partner<ROW, (1 << (LV - 1))>(L, b);     // top level: one partner
    }
}

// A product that must be rounded on its own (the general path adds J_cT x_T as a finished sum; the t_local path's lone
// product must not be fused into the addition that follows, or the two paths differ in the last bit and a reactor's
// result would depend on its wavefront's other reactors).
__device__ __forceinline__ double rounded(double x) { asm volatile("" : "+v"(x)); return x; }

// Row-straddling zone counts, no coupling to a neighbour's temperature (t_local): the T and the pH system are
// independent, so they go through the levels in lock step -- both systems' neighbours in one batch of exchanges (one LDS
// round trip per level instead of two) and the level's factors fetched along with them (never more than one level of
// factors in registers).  The arithmetic per system is that of the one-system levels.
template <int LV, int l>
__device__ __forceinline__ void pcr_real_pair(const Lane &L, const FStore<LV> &F, double &b0, double &b1)
{
    using S = FSlots<LV>;
    if constexpr (l + 1 < LV) {
        constexpr int st = 1 << l;
        double lo0, hi0, lo1, hi1;
        both<false, st>(L, b0, lo0, hi0); both<false, st>(L, b1, lo1, hi1);
        double a0, g0, a1, g1;
        F.ld2(2 * l, a0, g0); F.ld2(S::RS + 2 * l, a1, g1);
        b0 = b0 - a0 * keep_m(L.m_lo[l], lo0) - g0 * keep_m(L.m_hi[l], hi0);
        b1 = b1 - a1 * keep_m(L.m_lo[l], lo1) - g1 * keep_m(L.m_hi[l], hi1);
        pcr_real_pair<LV, l + 1>(L, F, b0, b1);
    } else {
        constexpr int st = 1 << (LV - 1);
        const double p0 = from_partner<false, st>(L, b0), p1 = from_partner<false, st>(L, b1);
        const double f0 = F.ld(2 * (LV - 1)), f1 = F.ld(S::RS + 2 * (LV - 1));
        b0 = b0 - f0 * p0;
        b1 = b1 - f1 * p1;
    }
}

template <bool ROW, int LV>
__device__ __forceinline__ void solve_real(const Lane &L, const Jac &J, const FStore<LV> &F, double b[3], bool t_local)
{
    if constexpr (!ROW && LV >= 2) {
        if (t_local) {
            using S = FSlots<LV>;
            double xT = b[STT], xP = b[SPH];
            pcr_real_pair<LV, 0>(L, F, xT, xP);
            xT *= F.ld(2 * LV - 1); xP *= F.ld(S::RS + 2 * LV - 1);
            RealFactors<LV> fC;
            load_real<LV>(F, 2, fC);
            const double tC = rounded(J.ct[1] * xT);
            double xC = b[SCL] + tC + J.cp * xP;
            pcr_real_level<ROW, LV, 0>(L, fC, xC);
            xC *= fC.inv;
            b[SPH] = xP; b[SCL] = xC; b[STT] = xT;
            return;
        }
    }
    // (many levels: a system's factors are fetched when its turn comes, or the three sets together crowd the register file)
    RealFactors<LV> fT, fP, fC;
    load_real<LV>(F, 0, fT);
    if constexpr (LV < 4) { load_real<LV>(F, 1, fP); load_real<LV>(F, 2, fC); }
    double xT = b[STT];
    pcr_real_level<ROW, LV, 0>(L, fT, xT);
    xT *= fT.inv;
    if constexpr (LV >= 4) load_real<LV>(F, 1, fP);
    double xP, tC;
    if (t_local) {      // (wave-uniform) no row of this wavefront couples to a neighbour's temperature: see jac_t_local
        xP = b[SPH];
        tC = rounded(J.ct[1] * xT);
    } else {
        const double xT_lo_r = from_lo<ROW, 1>(L, xT), xT_hi_r = from_hi<ROW, 1>(L, xT);
        const double xT_lo = keep_m(L.m_lo[0], xT_lo_r), xT_hi = keep_m(L.m_hi[0], xT_hi_r); // J.pt/ct[0,2] are 0 there
        xP = b[SPH] + (J.pt[0] * xT_lo + J.pt[1] * xT + J.pt[2] * xT_hi);
        tC = J.ct[0] * xT_lo + J.ct[1] * xT + J.ct[2] * xT_hi;
    }
    pcr_real_level<ROW, LV, 0>(L, fP, xP);
    xP *= fP.inv;
    if constexpr (LV >= 4) load_real<LV>(F, 2, fC);
    double xC = b[SCL] + tC + J.cp * xP;
    pcr_real_level<ROW, LV, 0>(L, fC, xC);
    xC *= fC.inv;
    b[SPH] = xP; b[SCL] = xC; b[STT] = xT;
}

// Real and complex solve of one Newton iteration, level by level in lock step: the two
// cyclic-reduction chains are independent, so interleaving them doubles the instruction-level
// parallelism of what is otherwise one long dependent chain, and each system's factors are
// fetched from LDS in one batch (one wait per system instead of one per level).
template <int LV> struct SysFactors {
    static constexpr int NL = LV > 1 ? LV - 1 : 1;
    double ra[NL], rg[NL], rf, rinv; cplx ca[NL], cg[NL], cf, cinv;
};

template <int LV>
__device__ __forceinline__ void load_sys(const FStore<LV> &F, int k, SysFactors<LV> &s)
{
    using S = FSlots<LV>;
    const int r0 = k * S::RS, c0 = S::CB + k * S::CS;
#pragma unroll
    for (int l = 0; l + 1 < LV; ++l) {
        F.ld2(r0 + 2 * l, s.ra[l], s.rg[l]);
        F.ld2(c0 + 4 * l, s.ca[l].r, s.ca[l].i);
        F.ld2(c0 + 4 * l + 2, s.cg[l].r, s.cg[l].i);
    }
    F.ld2(r0 + 2 * (LV - 1), s.rf, s.rinv);
    F.ld2(c0 + 4 * (LV - 1), s.cf.r, s.cf.i);
    F.ld2(c0 + 4 * LV - 2, s.cinv.r, s.cinv.i);
}

// one level of a real + complex pair of systems, given the (masked) neighbours' values and the level's factors
__device__ __forceinline__ void rc_apply(double ra, double rg, cplx ca, cplx cg, double b_lo, double b_hi, cplx c_lo, cplx c_hi,
                                         double &b, cplx &c)
{
    b = b - ra * b_lo - rg * b_hi;
    // c -= ca * c_lo + cg * c_hi as eight fused multiply-adds (no separate products and subtractions)
    double cr = c.r, ci = c.i;
    cr = __builtin_fma(-ca.r, c_lo.r, cr); ci = __builtin_fma(-ca.r, c_lo.i, ci);
    cr = __builtin_fma(ca.i, c_lo.i, cr);  ci = __builtin_fma(-ca.i, c_lo.r, ci);
    cr = __builtin_fma(-cg.r, c_hi.r, cr); ci = __builtin_fma(-cg.r, c_hi.i, ci);
    cr = __builtin_fma(cg.i, c_hi.i, cr);  ci = __builtin_fma(-cg.i, c_hi.r, ci);
    c = {cr, ci};
}
// the top level: one partner, one factor
__device__ __forceinline__ void rc_apply_top(double rf, cplx cf, double b_p, cplx c_p, double &b, cplx &c)
{
    b = b - rf * b_p;
    double cr = c.r, ci = c.i;
    cr = __builtin_fma(-cf.r, c_p.r, cr); ci = __builtin_fma(-cf.r, c_p.i, ci);
    cr = __builtin_fma(cf.i, c_p.i, cr);  ci = __builtin_fma(-cf.i, c_p.r, ci);
    c = {cr, ci};
}
template <bool ROW, int LV, int l>
__device__ __forceinline__ void rc_neighbours(const Lane &L, double b, cplx c, double &b_lo, double &b_hi, cplx &c_lo, cplx &c_hi)
{
    constexpr int st = 1 << l;
    both<ROW, st>(L, b, b_lo, b_hi); cboth<ROW, st>(L, c, c_lo, c_hi);
    b_lo = keep_m(L.m_lo[l], b_lo); b_hi = keep_m(L.m_hi[l], b_hi);
    c_lo = {keep_m(L.m_lo[l], c_lo.r), keep_m(L.m_lo[l], c_lo.i)};
    c_hi = {keep_m(L.m_hi[l], c_hi.r), keep_m(L.m_hi[l], c_hi.i)};
}

template <bool ROW, int LV, int l>
__device__ __forceinline__ void pcr_rc_level(const Lane &L, const SysFactors<LV> &s, double &b, cplx &c)
{
    if constexpr (l + 1 < LV) {
        double b_lo, b_hi; cplx c_lo, c_hi;
        rc_neighbours<ROW, LV, l>(L, b, c, b_lo, b_hi, c_lo, c_hi);
        rc_apply(s.ra[l], s.rg[l], s.ca[l], s.cg[l], b_lo, b_hi, c_lo, c_hi, b, c);
        pcr_rc_level<ROW, LV, l + 1>(L, s, b, c);
    } else {
        constexpr int st = 1 << (LV - 1);
        const double b_p = from_partner<ROW, st>(L, b);
        const cplx c_p = {from_partner<ROW, st>(L, c.r), from_partner<ROW, st>(L, c.i)};
        rc_apply_top(s.rf, s.cf, b_p, c_p, b, c);
    }
}

// T and pH systems in lock step (see pcr_real_pair)
template <int LV, int l>
__device__ __forceinline__ void pcr_rc_pair(const Lane &L, const FStore<LV> &F, double &b0, cplx &c0, double &b1, cplx &c1)
{
    using S = FSlots<LV>;
    constexpr int r0 = 0, r1 = S::RS, q0 = S::CB, q1 = S::CB + S::CS;
    if constexpr (l + 1 < LV) {
        double bl0, bh0, bl1, bh1; cplx cl0, ch0, cl1, ch1;
        rc_neighbours<false, LV, l>(L, b0, c0, bl0, bh0, cl0, ch0);
        rc_neighbours<false, LV, l>(L, b1, c1, bl1, bh1, cl1, ch1);
        double ra0, rg0, ra1, rg1; cplx ca0, cg0, ca1, cg1;
        F.ld2(r0 + 2 * l, ra0, rg0); F.ld2(r1 + 2 * l, ra1, rg1);
        F.ld2(q0 + 4 * l, ca0.r, ca0.i); F.ld2(q0 + 4 * l + 2, cg0.r, cg0.i);
        F.ld2(q1 + 4 * l, ca1.r, ca1.i); F.ld2(q1 + 4 * l + 2, cg1.r, cg1.i);
        rc_apply(ra0, rg0, ca0, cg0, bl0, bh0, cl0, ch0, b0, c0);
        rc_apply(ra1, rg1, ca1, cg1, bl1, bh1, cl1, ch1, b1, c1);
        pcr_rc_pair<LV, l + 1>(L, F, b0, c0, b1, c1);
    } else {
        constexpr int st = 1 << (LV - 1);
        const double p0 = from_partner<false, st>(L, b0), p1 = from_partner<false, st>(L, b1);
        const cplx cp0 = {from_partner<false, st>(L, c0.r), from_partner<false, st>(L, c0.i)};
        const cplx cp1 = {from_partner<false, st>(L, c1.r), from_partner<false, st>(L, c1.i)};
        const double rf0 = F.ld(r0 + 2 * (LV - 1)), rf1 = F.ld(r1 + 2 * (LV - 1));
        cplx cf0, cf1;
        F.ld2(q0 + 4 * (LV - 1), cf0.r, cf0.i); F.ld2(q1 + 4 * (LV - 1), cf1.r, cf1.i);
        rc_apply_top(rf0, cf0, p0, cp0, b0, c0);
        rc_apply_top(rf1, cf1, p1, cp1, b1, c1);
    }
}

template <bool ROW, int LV>
__device__ __forceinline__ void solve_rc(const Lane &L, const Jac &J, const FStore<LV> &F,
                                         double br[3], double cr[3], double ci[3], bool t_local)
{
    // Few levels: all three systems' factors are fetched ahead of their use (one exposed LDS round trip instead
    // of three).  Many levels (n > 8): 6 LV + 3 doubles per system -- fetched system by system, or the three sets
    // together overflow the register file into scratch.
    SysFactors<LV> sT, sP, sC;
    if constexpr (!ROW && LV >= 2) {
        if (t_local) {
            using S = FSlots<LV>;
            double xT = br[STT], xP = br[SPH]; cplx zT = {cr[STT], ci[STT]}, zP = {cr[SPH], ci[SPH]};
            pcr_rc_pair<LV, 0>(L, F, xT, zT, xP, zP);
            xT *= F.ld(2 * LV - 1); zT = cmul(zT, {F.ld(S::CB + 4 * LV - 2), F.ld(S::CB + 4 * LV - 1)});
            xP *= F.ld(S::RS + 2 * LV - 1); zP = cmul(zP, {F.ld(S::CB + S::CS + 4 * LV - 2), F.ld(S::CB + S::CS + 4 * LV - 1)});
            load_sys<LV>(F, 2, sC);
            const double tC = rounded(J.ct[1] * xT); const cplx uC = {rounded(J.ct[1] * zT.r), rounded(J.ct[1] * zT.i)};
            double xC = br[SCL] + tC + J.cp * xP;
            cplx zC = {cr[SCL] + uC.r + J.cp * zP.r, ci[SCL] + uC.i + J.cp * zP.i};
            pcr_rc_level<ROW, LV, 0>(L, sC, xC, zC);
            xC *= sC.rinv; zC = cmul(zC, sC.cinv);
            br[SPH] = xP; br[SCL] = xC; br[STT] = xT;
            cr[SPH] = zP.r; ci[SPH] = zP.i; cr[SCL] = zC.r; ci[SCL] = zC.i; cr[STT] = zT.r; ci[STT] = zT.i;
            return;
        }
    }
    load_sys<LV>(F, 0, sT);
    if constexpr (LV < 4) load_sys<LV>(F, 1, sP);
    // temperature block
    double xT = br[STT]; cplx zT = {cr[STT], ci[STT]};
    pcr_rc_level<ROW, LV, 0>(L, sT, xT, zT);
    xT *= sT.rinv; zT = cmul(zT, sT.cinv);
    if constexpr (LV < 4) load_sys<LV>(F, 2, sC); else load_sys<LV>(F, 1, sP);
    double xP, tC; cplx zP, uC;
    if (t_local) {      // (wave-uniform) no row of this wavefront couples to a neighbour's temperature: see jac_t_local
        xP = br[SPH]; zP = {cr[SPH], ci[SPH]};
        tC = rounded(J.ct[1] * xT); uC = {rounded(J.ct[1] * zT.r), rounded(J.ct[1] * zT.i)};
    } else {
        const double xT_lo = keep_m(L.m_lo[0], from_lo<ROW, 1>(L, xT)), xT_hi = keep_m(L.m_hi[0], from_hi<ROW, 1>(L, xT));
        const cplx zT_lo = {keep_m(L.m_lo[0], from_lo<ROW, 1>(L, zT.r)), keep_m(L.m_lo[0], from_lo<ROW, 1>(L, zT.i))};
        const cplx zT_hi = {keep_m(L.m_hi[0], from_hi<ROW, 1>(L, zT.r)), keep_m(L.m_hi[0], from_hi<ROW, 1>(L, zT.i))};
        // pH block: rhs += J_pT x_T
        xP = br[SPH] + (J.pt[0] * xT_lo + J.pt[1] * xT + J.pt[2] * xT_hi);
        zP = {cr[SPH] + (J.pt[0] * zT_lo.r + J.pt[1] * zT.r + J.pt[2] * zT_hi.r),
              ci[SPH] + (J.pt[0] * zT_lo.i + J.pt[1] * zT.i + J.pt[2] * zT_hi.i)};
        tC = J.ct[0] * xT_lo + J.ct[1] * xT + J.ct[2] * xT_hi;
        uC = {J.ct[0] * zT_lo.r + J.ct[1] * zT.r + J.ct[2] * zT_hi.r, J.ct[0] * zT_lo.i + J.ct[1] * zT.i + J.ct[2] * zT_hi.i};
    }
    pcr_rc_level<ROW, LV, 0>(L, sP, xP, zP);
    xP *= sP.rinv; zP = cmul(zP, sP.cinv);
    if constexpr (LV >= 4) load_sys<LV>(F, 2, sC);
    // chlorine block: rhs += J_cT x_T + J_cp x_p
    double xC = br[SCL] + tC + J.cp * xP;
    cplx zC = {cr[SCL] + uC.r + J.cp * zP.r, ci[SCL] + uC.i + J.cp * zP.i};
    pcr_rc_level<ROW, LV, 0>(L, sC, xC, zC);
    xC *= sC.rinv; zC = cmul(zC, sC.cinv);
    br[SPH] = xP; br[SCL] = xC; br[STT] = xT;
    cr[SPH] = zP.r; ci[SPH] = zP.i; cr[SCL] = zC.r; ci[SCL] = zC.i; cr[STT] = zT.r; ci[STT] = zT.i;
}

} // namespace wt
