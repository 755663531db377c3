// wt_device.hpp -- gfx950 device code of the multi-zone CSTR physics step.
//
// Mapping (CDNA4, 64-wide wavefronts): one LANE per reactor zone, the n zones
// of a reactor in n consecutive lanes, floor(64/n) reactors per wavefront, one
// wavefront per workgroup.  Everything a reactor needs for a whole outer step
// (state, Radau iterates, Jacobian bands, tridiagonal factors) lives in that
// segment's registers; the 1-D inter-zone stencil, the tridiagonal solves
// (parallel cyclic reduction) and the RMS norms are DPP / wavefront shuffles (zone counts that straddle a
// 16-lane DPP row exchange strides >= 2 through a row of LDS instead: both()).
// HBM is touched once per work item (a wavefront's reactors advanced by a few outer steps): state in,
// state + derived out.  Work items come from a device-side queue, so one launch advances the whole
// ensemble by any number of outer steps and no wavefront waits for a launch boundary; the sensor
// suite and the PLC register image / command path of an outer step run on the same wavefront right
// behind it (wt_sensors.hpp, wt_plc.hpp).
//
// What is computed is the reference's IntegratedCSTR.step():
//   RHS            reactor.py:272-448 (+ thermodynamics.py:160-193,
//                  chemistry.py:400-437,483-523, spatial.py:142-320)
//   time stepping  scipy 1.15.3 Radau IIA(5): radau.py:48-176,399-539,
//                  common.py:63-134 (initial step), :257-382 (num_jac)
//   post-step      reactor.py:493-541
// The decision sequence (initial step, Newton iteration counts, accept/reject,
// Jacobian refresh, LU reuse) is scipy's; the linear algebra exploits the
// structure of this RHS instead of a dense LU: with unknowns ordered
// [T | pH | Cl] the Jacobian is block lower-triangular with tridiagonal
// diagonal blocks, so (mu/h I - J) x = b is three tridiagonal solves.
//
// Control structure: the solver is a per-reactor state machine (Phase) driven by
// one wave-wide loop.  Each trip evaluates the RHS once (three Radau stages for
// reactors in their Newton phase, one point for the others), so reactors of a
// wavefront that are at different places of scipy's algorithm (more Newton
// iterations, a rejected step, an extra internal step) still share the
// expensive transcendental work instead of waiting for each other phase by
// phase, and every heavy block exists exactly once in the code object.
//
// Where each subject lives (every header compiles when included alone):
//   wt_tables.hpp   tolerances, status bits, scipy's constants (rc::), the fp64 constant tables, exp / exp10
//   wt_args.hpp     StepArgs: the kernel-argument block, and fresh(), how a section re-reads it
//   wt_lanes.hpp    Lane and lane_geometry, DPP / LDS cross-lane moves, seg_sum, rcp / sqrt_k / div_by
//   wt_rhs.hpp      the reactor constants (RK), the zone properties, the rows of the RHS
//   wt_pcr.hpp      Jacobian bands, factor store, cyclic-reduction factorisation, solve_real / solve_rc
//   wt_numjac.hpp   num_jac and its passes
//   wt_queue.hpp    the device-side work queue
//   wt_step.hpp     Phase, LdsMap, rhs_points, run_item: one work item
//   this file       every __global__ kernel with its argument struct; their order is the order of .text
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "wt_tables.hpp"
#include "wt_args.hpp"
#include "wt_lanes.hpp"
#include "wt_rhs.hpp"
#include "wt_pcr.hpp"
#include "wt_numjac.hpp"
#include "wt_queue.hpp"
#include "wt_step.hpp"

namespace wt {

// One trajectory record from the state in memory, for the kernels that record at launch boundaries (x_in_item):
// reactors [r0, r1), destination pointers already at the record's slot.
struct RecordCopyArgs {
    int64_t r0, r1; int n;
    const double *pH, *Cl, *T, *time, *flow; const uint32_t *status;
    double *rec_pH, *rec_Cl, *rec_T, *rec_time, *rec_flow; uint32_t *rec_status;
};
__global__ __launch_bounds__(256) void record_copy_kernel(const RecordCopyArgs a)
{
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;   // grid: (r1 - r0) * n threads
    if (j < (a.r1 - a.r0) * a.n) {
        const int64_t i = a.r0 * a.n + j;
        a.rec_pH[i] = a.pH[i]; a.rec_Cl[i] = a.Cl[i]; a.rec_T[i] = a.T[i];
    }
    if (j < a.r1 - a.r0) {
        const int64_t r = a.r0 + j;
        a.rec_time[r] = a.time[r]; a.rec_flow[r] = a.flow[r]; a.rec_status[r] = a.status[r];
    }
}

// Start of a queue-schedule launch: every group is ready for step 0, nothing has been pushed yet.
struct QueueResetArgs { int32_t *q_ctrl; unsigned long long *q_slots; int32_t *q_next; int n_groups, q_cap; };
__global__ __launch_bounds__(256) void queue_reset_kernel(const QueueResetArgs a)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < a.q_cap) a.q_slots[i] = 0ull;
    if (i < a.n_groups) a.q_next[i] = 0;
    if (i < Q_WORDS) a.q_ctrl[i] = (i == Q_AVAIL) ? a.n_groups : 0;
}

// The physics kernel.  Queue schedule: a grid of worker wavefronts that take (wavefront-group, next few outer
// steps) items from a device-side FIFO until the whole ensemble has advanced n_steps -- one launch, no launch
// tails: a slow wavefront delays nobody, and with more groups than resident wavefronts every SIMD stays busy.
// Stream schedule (q_ctrl == nullptr): workgroup b advances group r0 / R + b by n_steps and exits.
template <int LV, bool ROW>
__global__ __launch_bounds__(64) void step_kernel(const StepArgs a_unused)
{
    (void)a_unused;   // never read directly: every section fetches what it needs through `pa` (see fresh())
    __shared__ __attribute__((aligned(16))) double lds[LdsMap<LV>::TOTAL];
    // the by-value argument block sits at offset 0 of the kernel-argument segment
    const ArgPtr pa = (ArgPtr)__builtin_amdgcn_kernarg_segment_ptr();
    Lane L;
    // ROW instantiations serve exactly one zone count (n = 2^LV): a compile-time constant for everything below
    lane_geometry(ROW ? (1 << LV) : fresh(pa)->n, L);
    if constexpr (!ROW) L.xrow = (LdsDouble *)(lds + LdsMap<LV>::X_OFF);   // cross-lane moves by strides >= 2
    bool exchanged = true;
    int group;
    {
        ArgPtr a = fresh(pa);
        group = a->q_ctrl ? queue_next(pa, -1, false, exchanged) : (int)(a->r0 / a->R) + (int)blockIdx.x;
    }
    while (group >= 0) {          // (one call site: the item body exists once in the code object)
        int step0 = 0, cnt;
        long long t0 = 0;
        bool queue;
        {
            ArgPtr a = fresh(pa);
            queue = a->q_ctrl != nullptr;
            cnt = a->n_steps;
            if (queue) {
                // taken over from another worker: its release (queue_next) -> this acquire -> plain loads of the group's state
                if (exchanged) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
                if ((threadIdx.x & 63) == 0) step0 = __hip_atomic_load(a->q_next + group, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                step0 = __builtin_amdgcn_readfirstlane(step0);
                const int left = a->n_steps - step0, item = a->item_steps;
                cnt = left < item ? left : item;
                if (a->trace) t0 = __builtin_amdgcn_s_memrealtime();
            }
        }
        run_item<LV, ROW>(pa, L, lds, group, step0, cnt);
        if (!queue) break;
        ArgPtr a = fresh(pa);
        const bool more = step0 + cnt < a->n_steps;
        int hold = 0;
        if ((threadIdx.x & 63) == 0) {
            __hip_atomic_store(a->q_next + group, step0 + cnt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            // items this group has behind it against the ensemble's average
            const long long done = __hip_atomic_fetch_add(a->q_ctrl + Q_DONE, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) + 1;
            const int item = a->item_steps;
            const long long mine = (step0 + cnt + item - 1) / item;
            hold = (mine * a->n_groups < done) ? 1 : 0;     // (one item more or less of slack either way: measured worse)
            if (a->trace) {
                const int slot = __hip_atomic_fetch_add(a->q_ctrl + Q_TRACE, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (slot < a->trace_cap) {
                    int64_t *o = a->trace + (int64_t)slot * 5;
                    o[0] = blockIdx.x; o[1] = group; o[2] = (int64_t)step0 | ((int64_t)cnt << 32); o[3] = t0; o[4] = __builtin_amdgcn_s_memrealtime();
                }
            }
        }
        hold = __builtin_amdgcn_readfirstlane(hold);
        group = queue_next(pa, more ? group : -1, hold != 0, exchanged);
    }
}

// After a queue-schedule launch: every group must have advanced by the launch's step count and the hand-off must
// not have timed out; anything else is recorded in a word that survives the next launch's queue reset and that every
// download path reports (a short-changed group must not pass as WT_OK).
struct QueueCheckArgs { const int32_t *q_ctrl, *q_next; int n_groups, n_steps; int32_t *sticky; };
__global__ __launch_bounds__(256) void queue_check_kernel(const QueueCheckArgs a)
{
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    // the record is two words of host-coherent memory, each only ever set to 1: plain stores, no copy to read them
    if (g < a.n_groups && a.q_next[g] != a.n_steps) a.sticky[1] = 1;
    if (g == 0 && a.q_ctrl[Q_ERROR] != 0) a.sticky[0] = 1;
}

// One contiguous image of a small ensemble's state for a single device-to-host copy:
// [pH | Cl | T | H | rho | k] (N n doubles each), [time | flow] (N doubles each), status (N words), sticky word.
struct SnapshotArgs {
    int64_t cnt, N;
    const double *pH, *Cl, *T, *dH, *dRho, *dK, *time, *flow; const uint32_t *status; const int32_t *sticky;
    double *out;
};
__global__ __launch_bounds__(256) void snapshot_pack_kernel(const SnapshotArgs a)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < a.cnt) {
        a.out[i] = a.pH[i]; a.out[a.cnt + i] = a.Cl[i]; a.out[2 * a.cnt + i] = a.T[i];
        a.out[3 * a.cnt + i] = a.dH[i]; a.out[4 * a.cnt + i] = a.dRho[i]; a.out[5 * a.cnt + i] = a.dK[i];
    }
    if (i < a.N) {
        double *tail = a.out + 6 * a.cnt;
        tail[i] = a.time[i]; tail[a.N + i] = a.flow[i];
        uint32_t *w = reinterpret_cast<uint32_t *>(tail + 2 * a.N);
        w[i] = a.status[i];
        if (i == 0) w[a.N] = (uint32_t)(a.sticky[0] | a.sticky[1]);
    }
}

// derivatives() at caller-supplied states, for parity tests (reactor.py:272-448)
struct RhsArgs {
    int64_t N; int n; int R;
    const double *par, *bc;
    const double *pH, *Cl, *T;
    double *dpH, *dCl, *dT;
    uint32_t *flags;
};

template <bool ROW>
__global__ __launch_bounds__(64) void rhs_kernel(const RhsArgs a)
{
    Lane L; int64_t r;
    if (!lane_setup(0, a.N, a.n, a.R, L, r)) return;
    const int64_t idx = r * a.n + L.z;
    RK k; load_reactor(a.par, a.bc, a.N, r, a.n, k); mask_reactor_for_lane(L, k);
    double y[3] = {a.pH[idx], a.Cl[idx], a.T[idx]}, f[3];
    const bool bad = rhs_full<ROW>(L, kp_of(default_ktab()), kt_of(default_ktab()), k, y, f);
    a.dpH[idx] = f[SPH]; a.dCl[idx] = f[SCL]; a.dT[idx] = f[STT];
    const bool anybad = seg_any(L, bad);
    if (L.z == 0) a.flags[r] = anybad ? ST_T_RANGE : 0u;
}

// ReactorState.update_derived placeholders after the state was overwritten (reactor.py:137-147)
struct PlaceholderArgs { int64_t count; const double *pH; double *dH, *dRho, *dK; };
__global__ __launch_bounds__(256) void derived_placeholder_kernel(const PlaceholderArgs a)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.count) return;
    a.dH[i] = exp10_k(kp_of(default_ktab()), -a.pH[i]); a.dRho[i] = 998.2; a.dK[i] = 0.0001;
}

// Self-test of the cross-lane primitives against ds_bpermute-based __shfl:
// out[lane] = number of mismatching moves for that lane (parity tests assert 0).
struct ShuffleTestArgs { int n; int *out; };
template <bool ROW>
__global__ __launch_bounds__(64) void shuffle_selftest_kernel(const ShuffleTestArgs a)
{
    Lane L; int64_t r;
    __shared__ double xrow[XROW_CELLS];
    const bool present = lane_setup(0, 64 / a.n, a.n, 64 / a.n, L, r);
    if constexpr (!ROW) L.xrow = (LdsDouble *)xrow + XROW_PAD;
    if (!present) { a.out[threadIdx.x] = 0; return; }
    const int lane = threadIdx.x & 63;
    const double x = 1000.0 * (lane + 1) + 0.5;
    int bad = 0;
    auto chk = [&](double got, int src, bool valid) { if (valid && got != 1000.0 * (src + 1) + 0.5) bad++; };
    chk(from_lo<ROW, 1>(L, x), lane - 1, L.z >= 1); chk(from_hi<ROW, 1>(L, x), lane + 1, L.z + 1 < L.n);
    chk(from_lo<ROW, 2>(L, x), lane - 2, L.z >= 2); chk(from_hi<ROW, 2>(L, x), lane + 2, L.z + 2 < L.n);
    chk(from_lo<ROW, 4>(L, x), lane - 4, L.z >= 4); chk(from_hi<ROW, 4>(L, x), lane + 4, L.z + 4 < L.n);
    chk(from_lo<ROW, 8>(L, x), lane - 8, L.z >= 8); chk(from_hi<ROW, 8>(L, x), lane + 8, L.z + 8 < L.n);
    {   // the exchange-row moves of the cyclic reduction, every stride, and the top level's one partner
        double lo, hi;
        both<ROW, 1>(L, x, lo, hi); chk(lo, lane - 1, L.z >= 1); chk(hi, lane + 1, L.z + 1 < L.n);
        both<ROW, 2>(L, x, lo, hi); chk(lo, lane - 2, L.z >= 2); chk(hi, lane + 2, L.z + 2 < L.n);
        both<ROW, 4>(L, x, lo, hi); chk(lo, lane - 4, L.z >= 4); chk(hi, lane + 4, L.z + 4 < L.n);
        both<ROW, 8>(L, x, lo, hi); chk(lo, lane - 8, L.z >= 8); chk(hi, lane + 8, L.z + 8 < L.n);
        if constexpr (!ROW) {
            both<ROW, 16>(L, x, lo, hi); chk(lo, lane - 16, L.z >= 16); chk(hi, lane + 16, L.z + 16 < L.n);
            both<ROW, 32>(L, x, lo, hi); chk(lo, lane - 32, L.z >= 32); chk(hi, lane + 32, L.z + 32 < L.n);
            int top = 1;
            while (2 * top < L.n) top *= 2;
            const bool up = L.z >= top;
            const double got = top == 1 ? from_partner<false, 1>(L, x) : top == 2 ? from_partner<false, 2>(L, x)
                             : top == 4 ? from_partner<false, 4>(L, x) : top == 8 ? from_partner<false, 8>(L, x)
                             : top == 16 ? from_partner<false, 16>(L, x) : from_partner<false, 32>(L, x);
            chk(got, up ? lane - top : lane + top, up || (L.z + top < L.n));
        }
    }
    double ref = 0.0;
    for (int j = 0; j < L.n; ++j) ref += 1000.0 * (L.base + j + 1) + 0.5; // exact in fp64 (small integers + halves)
    if (seg_sum<ROW>(L, x) != ref) bad++;
    a.out[threadIdx.x] = bad;
}

// AqueousChemistry.calculate_pH (chemistry.py:271-330), one system per thread.
struct PhArgs {
    int64_t n;
    const double *Kw, *Ka1, *Ka2, *CT, *alk, *guess;
    double tol; int max_iter;
    double *pH; int32_t *iters; int32_t *rc;
};

__global__ __launch_bounds__(256) void ph_solve_kernel(const PhArgs a)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.n) return;
    const double Kw = a.Kw[i], Ka1 = a.Ka1[i], Ka2 = a.Ka2[i], CT = a.CT[i];
    const double alk_eq = a.alk[i] / 50000.0;                 // chemistry.py:223
    double pH = a.guess[i];
    int rcode = 2, it = 0;
    for (it = 0; it < a.max_iter; ++it) {
        // charge_balance_error chemistry.py:193-228
        const double H = exp10_k(kp_of(default_ktab()), -pH);
        const double OH = Kw / H;
        const double H2 = H * H;
        const double D = H2 + Ka1 * H + Ka1 * Ka2;
        const double a1 = (Ka1 * H) / D, a2 = (Ka1 * Ka2) / D;
        const double fval = H - OH + a1 * CT + 2 * (a2 * CT) - alk_eq;
        // charge_balance_derivative chemistry.py:230-269
        const double dH = -rc::LN10 * H;
        const double dOH = -(Kw / H2) * dH;
        const double dD = 2 * H + Ka1;
        const double D2 = D * D;
        const double da1 = Ka1 * (D - H * dD) / D2;
        const double da2 = -Ka1 * Ka2 * dD / D2;
        const double df = dH - dOH + CT * da1 * dH + 2 * (CT * da2 * dH);
        if (fabs(df) < 1e-15) { rcode = 1; break; }           // chemistry.py:309-312
        const double delta = -fval / df;
        const double pH_new = fmin(fmax(pH + delta, 0.0), 14.0);
        if (fabs(delta) < a.tol) { pH = pH_new; rcode = 0; ++it; break; }
        pH = pH_new;
    }
    a.pH[i] = pH; a.iters[i] = it; a.rc[i] = rcode;
}

} // namespace wt
