// wt_numjac.hpp -- scipy's finite-difference Jacobian (common.py:257-382) restated for the banded structure of this
// RHS: three colours per species, the perturbed zone-local properties evaluated once per species, scipy's step-size
// bookkeeping.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "wt_tables.hpp"
#include "wt_lanes.hpp"
#include "wt_rhs.hpp"
#include "wt_pcr.hpp"

namespace wt {

// ---------------------------------------------------------------- num_jac (common.py:257-382)
// Forward differences restated for the banded structure: perturbing zone j only
// changes rows of zones j-1..j+1, so zones of equal (j mod 3) are perturbed
// together (three colours per species) and each lane attributes the change of its
// rows to the single perturbed zone in its stencil.  The perturbed zone-local
// properties are evaluated once per species.  Per column this reproduces
// common.py's f(y + h e_j) - f(y) for the rows that can change; the step-size
// bookkeeping (factor growth/shrink, the one retry with 10x factor) is scipy's.
struct FdCols { double D[3][3]; double S[3][3]; }; // [row species][rel+1]: diff and max(|f|,|f_new|)

struct ZoneProps { double H, iw, phi, kT, rho; bool bpos; };

// What the rows of this lane see of their neighbourhood at the unperturbed state (once per Jacobian)
struct FdBase { double k_lo, k_hi, kd, H_lo, H_hi, C_lo, C_hi, T_lo, T_hi, rho_hi; };

template <bool ROW>
__device__ __forceinline__ FdBase fd_base(const Lane &L, const RK &k, const double y[3], const ZoneProps &b)
{
    FdBase n;
    n.rho_hi = from_hi<ROW, 1>(L, b.rho);
    n.k_hi = k_above(k, b.rho, n.rho_hi);
    n.k_lo = keep_m(L.m_lo[0], from_lo<ROW, 1>(L, n.k_hi));
    n.kd = k_diag(k, n.k_lo, n.k_hi);
    n.H_lo = keep_m(L.m_lo[0], from_lo<ROW, 1>(L, b.H)); n.H_hi = keep_m(L.m_hi[0], from_hi<ROW, 1>(L, b.H));
    n.C_lo = keep_m(L.m_lo[0], from_lo<ROW, 1>(L, y[SCL])); n.C_hi = keep_m(L.m_hi[0], from_hi<ROW, 1>(L, y[SCL]));
    n.T_lo = keep_m(L.m_lo[0], from_lo<ROW, 1>(L, y[STT])); n.T_hi = keep_m(L.m_hi[0], from_hi<ROW, 1>(L, y[STT]));
    return n;
}

// The columns of one species: every zone's own value perturbed by its own step.  A row of zone i changes with the
// columns of zones i-1, i, i+1 only, and which of its inputs a column reaches is known: so each row is evaluated
// three times -- with its own zone's perturbed values, with what its lower neighbour exports when perturbed, with what
// its upper neighbour exports -- everything else at the base values.  This is f(y + h e_j) - f(y) of common.py:331-333
// restricted to the rows that can change; rows that cannot depend on a column are structural zeros there too.
// out.D[q][r] is the change of this lane's row q when the zone at offset r-1 was perturbed.
// colmask (retry pass, common.py:343-361): only the flagged columns are perturbed.
template <bool ROW, int SP, bool BAR, class KC>
__device__ __forceinline__ void fd_species_pass(const Lane &L, const KC &kc, const RK &k, const double y[3], const double f[3],
                                                const ZoneProps &b, const FdBase &n, double hcol, bool colmask, bool all_cols,
                                                FdCols &out, bool &bad, double &badval)
{
    const double ypert = y[SP] + hcol;
#pragma unroll
    for (int q = 0; q < 3; ++q)
#pragma unroll
        for (int r = 0; r < 3; ++r) { out.D[q][r] = 0.0; out.S[q][r] = 0.0; }
    auto put = [&](int q, int r, double fn) { out.D[q][r] = fn - f[q]; out.S[q][r] = fmax(fabs(f[q]), fabs(fn)); };
    const double kphi = b.kT * b.phi;
    if constexpr (SP == SPH) {
        PropPH p = prop_pH<BAR>(kc, k, ypert);
        if (!all_cols && !colmask) { p.H = b.H; p.iw = b.iw; p.phi = b.phi; }        // this column is not part of the retry
        const double Hx_lo = keep_m(L.m_lo[0], from_lo<ROW, 1>(L, p.H)), Hx_hi = keep_m(L.m_hi[0], from_hi<ROW, 1>(L, p.H));
        put(SPH, 1, row_pH(k, mix3(n.k_lo, n.k_hi, n.kd, n.H_lo, n.H_hi, p.H), p.H, p.iw));
        put(SCL, 1, row_Cl(k, mix3(n.k_lo, n.k_hi, n.kd, n.C_lo, n.C_hi, y[SCL]), y[SCL], b.kT * p.phi));
        put(SPH, 0, row_pH(k, mix3(n.k_lo, n.k_hi, n.kd, Hx_lo, n.H_hi, b.H), b.H, b.iw));
        put(SPH, 2, row_pH(k, mix3(n.k_lo, n.k_hi, n.kd, n.H_lo, Hx_hi, b.H), b.H, b.iw));
    }
    if constexpr (SP == SCL) {
        const double cx = (all_cols || colmask) ? ypert : y[SCL];
        const double Cx_lo = keep_m(L.m_lo[0], from_lo<ROW, 1>(L, cx)), Cx_hi = keep_m(L.m_hi[0], from_hi<ROW, 1>(L, cx));
        put(SCL, 1, row_Cl(k, mix3(n.k_lo, n.k_hi, n.kd, n.C_lo, n.C_hi, cx), cx, kphi));
        put(SCL, 0, row_Cl(k, mix3(n.k_lo, n.k_hi, n.kd, Cx_lo, n.C_hi, y[SCL]), y[SCL], kphi));
        put(SCL, 2, row_Cl(k, mix3(n.k_lo, n.k_hi, n.kd, n.C_lo, Cx_hi, y[SCL]), y[SCL], kphi));
    }
    if constexpr (SP == STT) {
        PropT p = prop_T<BAR>(kc, ypert);
        if (colmask && p.bad && !bad) { bad = true; badval = ypert; }   // the reference raises on this perturbed column
        double tx = ypert;
        if (!all_cols && !colmask) { p.kT = b.kT; p.rho = b.rho; tx = y[STT]; }
        const double Tx_lo = keep_m(L.m_lo[0], from_lo<ROW, 1>(L, tx)), Tx_hi = keep_m(L.m_hi[0], from_hi<ROW, 1>(L, tx));
        // the two interfaces of a zone move with its density: K[i,i+1] with this zone / with the zone above perturbed
        const double khi_own = k_above(k, p.rho, n.rho_hi);
        const double khi_up = k_above(k, b.rho, from_hi<ROW, 1>(L, p.rho));
        const double klo_own = keep_m(L.m_lo[0], from_lo<ROW, 1>(L, khi_up));    // K[i,i-1] with this zone perturbed
        const double klo_dn = keep_m(L.m_lo[0], from_lo<ROW, 1>(L, khi_own));    // ... with the zone below perturbed
        {   // own zone
            const double kd = k_diag(k, klo_own, khi_own);
            put(SPH, 1, row_pH(k, mix3(klo_own, khi_own, kd, n.H_lo, n.H_hi, b.H), b.H, b.iw));
            put(SCL, 1, row_Cl(k, mix3(klo_own, khi_own, kd, n.C_lo, n.C_hi, y[SCL]), y[SCL], p.kT * b.phi));
            put(STT, 1, row_T(k, mix3(klo_own, khi_own, kd, n.T_lo, n.T_hi, tx), tx));
        }
        {   // zone below
            const double kd = k_diag(k, klo_dn, n.k_hi);
            put(SPH, 0, row_pH(k, mix3(klo_dn, n.k_hi, kd, n.H_lo, n.H_hi, b.H), b.H, b.iw));
            put(SCL, 0, row_Cl(k, mix3(klo_dn, n.k_hi, kd, n.C_lo, n.C_hi, y[SCL]), y[SCL], kphi));
            put(STT, 0, row_T(k, mix3(klo_dn, n.k_hi, kd, Tx_lo, n.T_hi, y[STT]), y[STT]));
        }
        {   // zone above
            const double kd = k_diag(k, n.k_lo, khi_up);
            put(SPH, 2, row_pH(k, mix3(n.k_lo, khi_up, kd, n.H_lo, n.H_hi, b.H), b.H, b.iw));
            put(SCL, 2, row_Cl(k, mix3(n.k_lo, khi_up, kd, n.C_lo, n.C_hi, y[SCL]), y[SCL], kphi));
            put(STT, 2, row_T(k, mix3(n.k_lo, khi_up, kd, n.T_lo, Tx_hi, y[STT]), y[STT]));
        }
    }
}

// For the column owned by this lane (species SP): max |diff| over its rows with
// numpy argmax tie-breaking (first row in [pH.., Cl.., T..] order) and the
// matching scale (common.py:335-339).
template <bool ROW, int SP>
__device__ __forceinline__ void fd_col_reduce(const Lane &L, const FdCols &c, double &maxd, double &scale)
{
    maxd = -1.0; scale = 0.0;
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        // rows of species q that can depend on a column of species SP
        const bool dep_nb = (q == SP) || (SP == STT);           // neighbour-zone rows
        const bool dep_own = dep_nb || (q == SCL && SP == SPH); // own-zone row
        if (!dep_own) continue;
        double d_lo = 0, s_lo = 0, d_hi = 0, s_hi = 0;
        if (dep_nb) {
            d_lo = from_lo<ROW, 1>(L, c.D[q][2]); s_lo = from_lo<ROW, 1>(L, c.S[q][2]); // lane z-1 saw this column at rel=+1
            d_hi = from_hi<ROW, 1>(L, c.D[q][0]); s_hi = from_hi<ROW, 1>(L, c.S[q][0]); // lane z+1 saw it at rel=-1
        }
        if (dep_nb && L.has_lo && fabs(d_lo) > maxd) { maxd = fabs(d_lo); scale = s_lo; }
        if (fabs(c.D[q][1]) > maxd) { maxd = fabs(c.D[q][1]); scale = c.S[q][1]; }
        if (dep_nb && L.has_hi && fabs(d_hi) > maxd) { maxd = fabs(d_hi); scale = s_hi; }
    }
}

__device__ __forceinline__ double fd_step(double y, double fac, double ysc)
{
    // h = (y + factor*y_scale) - y, evaluated without fusing (common.py:323)
    return __dadd_rn(__dadd_rn(y, __dmul_rn(fac, ysc)), -y);
}

// One species' columns: perturb, reduce, optional retry, factor update.  Leaves
// the finished difference quotients of this species' columns in `cols.D`
// (already divided by the column's h).
template <bool ROW, int SP, bool BAR, class KC>
__device__ __forceinline__ void num_jac_species(const Lane &L, const KC &kc, const RK &k, const double y[3], const double f[3],
                                                const ZoneProps &b, const FdBase &nb, double &fac, FdCols &cols, bool &bad, double &badval)
{
    const double fs = (f[SP] >= 0) ? 1.0 : -1.0;
    const double ysc = fs * fmax(ATOL, fabs(y[SP]));
    double h = fd_step(y[SP], fac, ysc);
    while (WT_RARE(h == 0)) { fac *= 10; h = fd_step(y[SP], fac, ysc); }    // common.py:327-330
    fd_species_pass<ROW, SP, BAR>(L, kc, k, y, f, b, nb, h, true, true, cols, bad, badval);
    double maxd, scl;
    fd_col_reduce<ROW, SP>(L, cols, maxd, scl);
    const bool small = maxd < rc::NJ_REJECT * scl;                  // common.py:341
    if (WT_RARE(__ballot(small) != 0ull)) {                         // rare: one retry with 10x factor
        const double nf = 10 * fac;
        const double hn = fd_step(y[SP], nf, ysc);
        FdCols c2;
        fd_species_pass<ROW, SP, BAR>(L, kc, k, y, f, b, nb, hn, small, false, c2, bad, badval);
        double md2, sc2;
        fd_col_reduce<ROW, SP>(L, c2, md2, sc2);
        const bool upd = small && (maxd * sc2 < md2 * scl);         // common.py:354
        if (upd) { fac = nf; h = hn; maxd = md2; scl = sc2; }
        const int iu = upd ? 1 : 0;
        const int iu_lo = __shfl_up(iu, 1, 64), iu_hi = __shfl_down(iu, 1, 64);
        const bool upd_lo = L.has_lo && (iu_lo != 0), upd_hi = L.has_hi && (iu_hi != 0);
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            if (upd_lo) cols.D[q][0] = c2.D[q][0];
            if (upd) cols.D[q][1] = c2.D[q][1];
            if (upd_hi) cols.D[q][2] = c2.D[q][2];
        }
    }
    // diff /= h (column-wise; the column's h lives in the column's lane)
    const double h_lo = from_lo<ROW, 1>(L, h), h_hi = from_hi<ROW, 1>(L, h);
    const double ih0 = L.has_lo ? rcp(h_lo) : 0.0, ih1 = rcp(h), ih2 = L.has_hi ? rcp(h_hi) : 0.0;
#pragma unroll
    for (int q = 0; q < 3; ++q) { cols.D[q][0] *= ih0; cols.D[q][1] *= ih1; cols.D[q][2] *= ih2; }
    // factor adaptation common.py:363-365
    const bool sm = maxd < rc::NJ_SMALL * scl, bg = maxd > rc::NJ_BIG * scl;
    if (sm) fac *= 10;
    if (bg) fac *= 0.1;
    fac = fmax(fac, rc::NJ_MINF);
}

// The three species' passes are sections like those of rhs_points: each fetches the constants it works with.
// KTP: pointer to the constant table (kernel-argument segment in the step kernel).
template <bool ROW, bool BAR = false, class KTP>   // BAR: see row_fence (wt_rhs.hpp)
__device__ __forceinline__ void num_jac(const Lane &L, const RKStore &ks, KTP ktab, const double y[3], const double f[3],
                                        double fac[3], bool &have_fac, Jac &J, bool &bad, double &badval, bool &t_dense,
                                        const ZoneProps *held = nullptr, bool have_held = false)
{
    if (!have_fac) { fac[0] = fac[1] = fac[2] = rc::NJ_F0; have_fac = true; }
    FdCols cols;
    ZoneProps b;
    FdBase nb;
    // The zone-local properties at y.  A caller that evaluated the RHS at this same y holds them (held, have_held per
    // lane): the same functions of the same argument, the same bits.  Where every lane that is here holds them, none is
    // formed; otherwise they are formed for all and the holders keep theirs.
    const bool all_held = held != nullptr && __ballot(!have_held) == 0ull;
    if (!all_held) {
        const KT ct = load_kt(ktab());
        const PropT bpt = prop_T<BAR>(ct, y[STT]);
        b.kT = bpt.kT; b.rho = bpt.rho;
    }
    {
        const KP cp = load_kp(ktab());
        const RK k = fetch_reactor(ks);
        if (!all_held) {
            const PropPH bpp = prop_pH<BAR>(cp, k, y[SPH]);
            b.H = bpp.H; b.iw = bpp.iw; b.phi = bpp.phi; b.bpos = bpp.bpos;
        }
        if (held != nullptr && (all_held || have_held)) b = *held;
        nb = fd_base<ROW>(L, k, y, b);
        num_jac_species<ROW, SPH, BAR>(L, cp, k, y, f, b, nb, fac[SPH], cols, bad, badval);
#pragma unroll
        for (int r = 0; r < 3; ++r) J.pp[r] = cols.D[SPH][r];
        J.cp = cols.D[SCL][1];
    }
    {
        const RK k = fetch_reactor(ks);
        num_jac_species<ROW, SCL, BAR>(L, 0, k, y, f, b, nb, fac[SCL], cols, bad, badval);
#pragma unroll
        for (int r = 0; r < 3; ++r) J.cc[r] = cols.D[SCL][r];
    }
    {
        const KT ct = load_kt(ktab());
        const RK k = fetch_reactor(ks);
        num_jac_species<ROW, STT, BAR>(L, ct, k, y, f, b, nb, fac[STT], cols, bad, badval);
#pragma unroll
        for (int r = 0; r < 3; ++r) { J.tt[r] = cols.D[STT][r]; J.pt[r] = cols.D[SPH][r]; J.ct[r] = cols.D[SCL][r]; }
        t_dense = jac_t_dense(J) || (ct.dense_bias != 0.0);
    }
}

} // namespace wt
