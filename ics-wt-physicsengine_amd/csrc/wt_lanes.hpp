// wt_lanes.hpp -- one LANE per reactor zone, the n zones of a reactor in n consecutive lanes: the Lane record and
// how it is filled (lane_geometry), the moves between a zone and its neighbours at power-of-two strides (DPP row and
// wavefront shifts; an exchange row in LDS where a segment straddles a 16-lane DPP row: both()), the sum over a
// segment, and the division-free arithmetic of the step-size controller (rcp, sqrt_k, root4, div_by, powi6:
// radau.py:113,171-174, common.py:130).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>

namespace wt {

// ---------------------------------------------------------------- lane geometry and cross-lane moves
typedef __attribute__((address_space(3))) double LdsDouble;
typedef __attribute__((address_space(3))) char LdsByte;
struct Divisor { double d, inv; };     // a fixed divisor and RN(1 / d): div_by()
struct Lane {
    int n, z;
    bool has_lo, has_hi;
    // the same neighbour tests as all-ones / zero words, one pair per cyclic-reduction stride 2^l: masking
    // with a VGPR operand (v_and) keeps the tests out of the scalar register file, where each would be a
    // 64-bit lane mask for the whole solver loop
    uint32_t m_lo[7], m_hi[7];
    uint32_t m_pt;            // whether the one partner of the top cyclic-reduction level (from_partner) exists
    int a_me;                 // byte offset of this lane's own cell in the exchange row (8 * lane)
    LdsDouble *xrow;          // cell 0 of the exchange row (ROW = false kernels; nullptr otherwise): XROW_PAD cells either side
    int base;                 // lane id of zone 0 of this segment
    unsigned long long segmask;
    Divisor d3n, d9n;         // 3n, 9n: component counts of the RMS norms (common.py:63-65, radau.py:105)
};

template <int CTRL> __device__ __forceinline__ double dpp_mov(double x)
{
    // bound_ctrl: lanes whose source lies outside the row / wavefront read 0; no "old" value to keep
    const int lo = __builtin_amdgcn_mov_dpp(__double2loint(x), CTRL, 0xf, 0xf, true);
    const int hi = __builtin_amdgcn_mov_dpp(__double2hiint(x), CTRL, 0xf, 0xf, true);
    return __hiloint2double(hi, lo);
}

// ROW = true: n divides 16, so a segment never straddles a 16-lane DPP row and
// every power-of-two stride is a row shift.  ROW = false: any n <= 64; stride 1
// is a whole-wave DPP shift; larger strides go through the exchange row (both(), below) in the solver, and
// through ds_bpermute in these two single-direction forms (self-test only).
// Values read from outside the segment are unspecified; callers mask them.
__device__ __forceinline__ double bpermute(int byte_addr, double x)
{
    const int lo = __builtin_amdgcn_ds_bpermute(byte_addr, __double2loint(x));
    const int hi = __builtin_amdgcn_ds_bpermute(byte_addr, __double2hiint(x));
    return __hiloint2double(hi, lo);
}
constexpr int ilog2(int s) { return s <= 1 ? 0 : 1 + ilog2(s >> 1); }

template <bool ROW, int S> __device__ __forceinline__ double from_lo(const Lane &L, double x)
{   // value held by lane (this - S)
    if constexpr (ROW && S < 16) return dpp_mov<0x110 + S>(x);      // row_shr:S
    else if constexpr (S == 1) return dpp_mov<0x138>(x);  // wave_shr:1
    else return bpermute(((L.a_me >> 1) - 4 * S) & 255, x);
}
// A value read from outside the segment only ever meets a zero coefficient, so it is
// enough to make it FINITE: clearing the high dword (sign, exponent, top mantissa bits)
// turns any NaN/Inf another reactor may hold into a denormal.  One v_and per read (with the
// Lane's all-ones / zero mask words), which the compiler folds into the DPP move of that dword.
__device__ __forceinline__ double keep_m(uint32_t mask, double x)
{
    return __hiloint2double(__double2hiint(x) & (int)mask, __double2loint(x));
}

// Strides that neither a row shift nor the whole-wave shift by one can do (ROW = false, S > 1) go through a row of 64
// doubles in LDS: every lane stores its value, then loads its neighbours'.  One ds_write_b64 + two ds_read_b64 per
// double and level where ds_bpermute_b32 needs four moves, at 10-14 cycles each instead of 24 (tools/ubench/lds.hip:
// four wavefronts of a CU sharing its LDS pipe).  The LDS pipe executes a wavefront's operations in order, so the next
// value may be stored as soon as the loads of the last one are issued: no wait between exchanges, only before the use.
// Lane +/- stride is an immediate offset from the lane's own cell (no address registers per level); what a lane reads
// from beyond the row's ends (its neighbours in the allocation: LdsMap) or from another reactor's cells is masked by its
// caller like every out-of-segment value.
constexpr int XROW_PAD = 32, XROW_CELLS = 64 + 2 * XROW_PAD;      // a stand-alone row (self-test kernel) carries padding
// (To the compiler a lane's store to its own cell and its loads of other cells are unrelated accesses of one thread,
// free to be reordered; the wave barriers -- no instruction, an ordering point for memory operations -- say otherwise.)
__device__ __forceinline__ void x_put(const Lane &L, double x)
{
    __builtin_amdgcn_wave_barrier();            // the loads of the previous exchange come first
    *(LdsDouble *)((LdsByte *)L.xrow + L.a_me) = x;
    __builtin_amdgcn_wave_barrier();            // ... and this exchange's loads after the store
}
__device__ __forceinline__ double x_get(const Lane &L, int byte_off) { return *(LdsDouble *)((LdsByte *)L.xrow + byte_off); }
template <int D> __device__ __forceinline__ double x_rel(const Lane &L)
{
    static_assert(D >= -XROW_PAD && D <= XROW_PAD, "stride beyond the padding");
    return *(LdsDouble *)((LdsByte *)L.xrow + L.a_me + 8 * D);
}

// At the top level of the cyclic reduction (stride S = 2^(LV-1) >= n/2) a zone has at most ONE partner: zone z - S if
// z >= S, else zone z + S if that exists.  ROW kernels (n = 2 S): partner = z xor S, a quad permutation (n = 2, 4), a
// row rotation (n = 16) or two moves (n = 8, below).  Otherwise through the exchange row.
template <int CTRL, int BANKS> __device__ __forceinline__ double dpp_merge(double old, double x)
{
    const int lo = __builtin_amdgcn_update_dpp(__double2loint(old), __double2loint(x), CTRL, 0xf, BANKS, false);
    const int hi = __builtin_amdgcn_update_dpp(__double2hiint(old), __double2hiint(x), CTRL, 0xf, BANKS, false);
    return __hiloint2double(hi, lo);
}
// n = 8 (S = 4): z xor 4 is no single DPP control.  As two bank-masked row shifts into one register every lane of a
// 16-lane row is written by exactly one of them (banks 1 and 3 by row_shr:4, banks 0 and 2 by row_shl:4), so the first
// shift's `old` operand never survives -- but it has to be a register, x is still live, and the compiler copies both
// dwords of x first: six instructions per double.  As row_half_mirror (z -> 7 - z) and then quad_perm [3,2,1,0] (3 - p
// within the quad) it is two moves per dword with no `old` at all: four.  Which of the two an instantiation takes is
// partner_exchange_without_copy (wt_step.hpp, with the other switches).  (A zone's partner is a lane of its own reactor,
// in the same solver phase: active whenever the zone is, as for the one-move forms.)
__host__ __device__ constexpr bool partner_exchange_without_copy(int LV, bool ROW);
template <bool ROW, int S> __device__ __forceinline__ double from_partner(const Lane &L, double x)
{
    if constexpr (ROW && S == 1) return dpp_mov<0xB1>(x);            // quad_perm [1,0,3,2]
    else if constexpr (ROW && S == 2) return dpp_mov<0x4E>(x);       // quad_perm [2,3,0,1]
    else if constexpr (ROW && S == 4) {
        if constexpr (partner_exchange_without_copy(3, ROW)) return dpp_mov<0x1B>(dpp_mov<0x141>(x));   // row_half_mirror, quad_perm [3,2,1,0]
        else return dpp_merge<0x104, 0x5>(dpp_merge<0x114, 0xA>(x, x), x);   // row_shr:4 -> zones 4..7, row_shl:4 -> zones 0..3
    }
    else if constexpr (ROW && S == 8) return dpp_mov<0x128>(x);      // row_ror:8
    else { x_put(L, x); return keep_m(L.m_pt, x_get(L, L.a_me + ((L.z >= S) ? -8 * S : 8 * S))); }   // (S: the top stride)
}

template <bool ROW, int S> __device__ __forceinline__ double from_hi(const Lane &L, double x)
{   // value held by lane (this + S)
    if constexpr (ROW && S < 16) return dpp_mov<0x100 + S>(x);      // row_shl:S
    else if constexpr (S == 1) return dpp_mov<0x130>(x);  // wave_shl:1
    else return bpermute(((L.a_me >> 1) + 4 * S) & 255, x);
}

// the values held by lanes (this - S) and (this + S)
template <bool ROW, int S> __device__ __forceinline__ void both(const Lane &L, double x, double &lo, double &hi)
{
    if constexpr (ROW || S == 1) { lo = from_lo<ROW, S>(L, x); hi = from_hi<ROW, S>(L, x); }
    else { x_put(L, x); lo = x_rel<-S>(L); hi = x_rel<S>(L); }
}

// A double that is defined without an instruction, its value irrelevant (Held::init's idiom): for a variable that is
// assigned on some paths only and read on those alone, so that the compiler does not carry its last contents along the
// others (run_item's stage points and values).
__device__ __forceinline__ double undefined_f64()
{
    int lo, hi;
    asm("" : "=v"(lo)); asm("" : "=v"(hi));
    return __hiloint2double(hi, lo);
}

__device__ __forceinline__ bool seg_any(const Lane &L, bool p) { return (__ballot(p) & L.segmask) != 0ull; }
__device__ __forceinline__ bool seg_all(const Lane &L, bool p) { return (__ballot(!p) & L.segmask) == 0ull; }

// Sum over the n lanes of a segment; every lane of the segment receives the
// bitwise-identical value (each butterfly step adds the same two operands in
// both partner lanes; the generic path scans and broadcasts).
// (LV: the kernel's number of cyclic-reduction levels, n <= 2^LV, where the caller knows it: rounds that cannot
// contribute are not compiled)
template <bool ROW, int LV = 6> __device__ __forceinline__ double seg_sum(const Lane &L, double x)
{
    if constexpr (ROW) {
        x += dpp_mov<0xB1>(x);                     // quad_perm [1,0,3,2]
        if (L.n >= 4) x += dpp_mov<0x4E>(x);       // quad_perm [2,3,0,1]
        if (L.n >= 8) x += dpp_mov<0x141>(x);      // row_half_mirror
        if (L.n >= 16) x += dpp_mov<0x140>(x);     // row_mirror
        return x;
    } else {
        // The inclusive scan by strides 1, 2, 4, ... (each lane adds the value 2^k lanes below while that lane is in
        // the segment), two strides per exchange: lane z forms what lane z - 2s would have added in the skipped
        // round itself, from the same operands in the same order -- the same bits as one stride per round, in half
        // the LDS round trips.  Then the last lane's total goes to everyone.
        auto two = [&](auto S_, double y) {
            constexpr int S = decltype(S_)::value;
            x_put(L, y);
            const double v1 = x_rel<-S>(L), v2 = x_rel<-2 * S>(L), v3 = x_rel<-3 * S>(L);
            const double t = (L.z >= 3 * S) ? v2 + v3 : v2;
            y = (L.z >= S) ? y + v1 : y;
            return (L.z >= 2 * S) ? y + t : y;
        };
        x = two(std::integral_constant<int, 1>{}, x);
        if (LV >= 3 && L.n > 4) x = two(std::integral_constant<int, 4>{}, x);
        if (LV >= 5 && L.n > 16) {
            x_put(L, x);
            const double v1 = x_rel<-16>(L);
            double t = 0.0;
            if (LV >= 6 && L.n > 32) {      // (the row's neighbours in the allocation do not reach 48 cells down: clamp)
                const double v2 = x_get(L, max(L.a_me - 8 * 32, 0)), v3 = x_get(L, max(L.a_me - 8 * 48, 0));
                t = (L.z >= 48) ? v2 + v3 : v2;
            }
            x = (L.z >= 16) ? x + v1 : x;
            x = (L.z >= 32) ? x + t : x;
        }
        x_put(L, x);
        return x_get(L, (L.base + L.n - 1) << 3);
    }
}

// 1/x to ~1 ulp: hardware seed + two Newton steps (no denormal / inf handling:
// every divisor on this path is a finite, normal number or the result is discarded)
__device__ __forceinline__ double rcp(double x)
{
    double r = __builtin_amdgcn_rcp(x);
    double e = __builtin_fma(-x, r, 1.0);
    r = __builtin_fma(r, e, r);
    e = __builtin_fma(-x, r, 1.0);
    return __builtin_fma(r, e, r);
}

// x^(1/4) and x^(-1/4) for the step-size controller (radau.py:171-174, common.py:130)
// through two square roots instead of the general pow(); the result only steers h.
// sqrt: the library's iteration (reciprocal square root seed, two Goldschmidt steps, one correction: correctly rounded)
// without its rescaling of arguments below 2^-767, which the norms and step-size ratios formed here never are
// (0, +inf and NaN behave as in the library).  Half the instructions.
__device__ __forceinline__ double sqrt_k(double x)
{
    const double y = __builtin_amdgcn_rsq(x);
    double g = x * y, h = y * 0.5;
    const double r = __builtin_fma(-h, g, 0.5);
    g = __builtin_fma(g, r, g); h = __builtin_fma(h, r, h);
    double d = __builtin_fma(-g, g, x); g = __builtin_fma(d, h, g);
    d = __builtin_fma(-g, g, x); g = __builtin_fma(d, h, g);
    return __builtin_amdgcn_class(x, 0x260) ? x : g;       // +-0, +inf
}
__device__ __forceinline__ double root4(double x) { return sqrt_k(sqrt_k(x)); }

// x / d for a fixed divisor, correctly rounded like the division it replaces (Markstein: q = x * RN(1/d) is within
// an ulp, its residual is exact in one fma, one more fma rounds correctly): three instructions instead of fourteen.
__device__ __forceinline__ double div_by(double x, const Divisor &c)
{
    const double q = x * c.inv;
    const double r = __builtin_fma(-c.d, q, x);
    const double q2 = __builtin_fma(r, c.inv, q);
    return __builtin_amdgcn_class(q, 0x204) ? q : q2;      // +-inf stays inf (its residual is NaN)
}

// rate ** k for k = 1..6 (radau.py:113) by repeated multiplication
__device__ __forceinline__ double powi6(double x, int k)
{
    const double x2 = x * x, x3 = x2 * x;
    double r = x;
    r = (k == 2) ? x2 : r; r = (k == 3) ? x3 : r; r = (k == 4) ? x2 * x2 : r;
    r = (k == 5) ? x2 * x3 : r; r = (k == 6) ? x3 * x3 : r;
    return r;
}

// lane -> (segment, zone) geometry; the same for every work item of a wavefront
__device__ __forceinline__ void lane_geometry(int n, Lane &L)
{
    const int lane = threadIdx.x & 63;
    const int seg = lane / n;
    L.n = n; L.z = lane - seg * n;
    L.base = seg * n;
    L.a_me = lane << 3; L.xrow = nullptr;
    L.has_lo = L.z > 0; L.has_hi = L.z < n - 1;
#pragma unroll
    for (int l = 0; l < 7; ++l) {
        L.m_lo[l] = (L.z - (1 << l) >= 0) ? ~0u : 0u;
        L.m_hi[l] = (L.z + (1 << l) < n) ? ~0u : 0u;
        // opaque to the optimiser, or `x & mask` is canonicalised back into a select on the compare
        asm("" : "+v"(L.m_lo[l]));
        asm("" : "+v"(L.m_hi[l]));
    }
    L.segmask = ((n >= 64) ? ~0ull : ((1ull << n) - 1ull)) << L.base;
    {
        int top = 1;
        while (2 * top < n) top *= 2;                     // 2^(LV-1): the top stride
        const bool up = L.z >= top, has = up || (L.z + top < n);
        L.m_pt = has ? ~0u : 0u;
        asm("" : "+v"(L.m_pt));
    }
    L.d3n = {(double)(3 * n), 1.0 / (double)(3 * n)};
    L.d9n = {(double)(9 * n), 1.0 / (double)(9 * n)};
}

// rhs_kernel / selftest: one wavefront-group per workgroup
__device__ __forceinline__ bool lane_setup(int64_t r0, int64_t r1, int n, int R, Lane &L, int64_t &r)
{
    lane_geometry(n, L);
    const int seg = (threadIdx.x & 63) / n;
    r = r0 + (int64_t)blockIdx.x * R + seg;
    return (seg < R) && (r < r1);
}

} // namespace wt
