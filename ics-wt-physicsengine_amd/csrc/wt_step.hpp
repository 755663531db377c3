// wt_step.hpp -- one work item of the step kernel: a wavefront's reactors advanced by a few outer steps of the
// reference's IntegratedCSTR.step().  Time stepping is scipy 1.15.3 Radau IIA(5) (radau.py:48-176,399-539, initial
// step common.py:63-134) as a per-reactor state machine (Phase) driven by one wave-wide loop, post-step
// reactor.py:493-541; the sensor suite, the PLC scan and the per-reactor programs of an outer step run right behind
// it.  The norm and step-size helpers, the wavefront's LDS map, rhs_points and run_item (DESIGN.md 7.15 maps it).
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

namespace wt {

// ---------------------------------------------------------------- helpers
template <bool ROW, int LV = 6, int PLAIN = 1>
__device__ __forceinline__ double rms3(const Lane &L, const double x[3], const double sc[3])
{
    // common.py:63-65 norm(x / scale) over the 3n components of one reactor
    // Which squares fuse into the sum is spelled out: left to the compiler it differs from one inlined copy to the next,
    // and moves when the code around a copy does.  v[PLAIN]^2 is the plain product; the probe's d2 has always had PLAIN = 0.
#pragma clang fp contract(off)
    double v[3];
#pragma unroll
    for (int q = 0; q < 3; ++q) v[q] = x[q] * rcp(sc[q]);
    const double s = __builtin_fma(v[2], v[2], __builtin_fma(v[1 - PLAIN], v[1 - PLAIN], v[PLAIN] * v[PLAIN]));
    return sqrt_k(div_by(seg_sum<ROW, LV>(L, s), L.d3n));
}

__device__ __forceinline__ double ulp_above(double t)
{
    // |nextafter(t, +inf) - t| for t >= 0 (radau.py:408)
    return __longlong_as_double(__double_as_longlong(t) + 1) - t;
}

// radau.py:139-176
__device__ __forceinline__ double predict_factor(double h_abs, bool have_old, double h_abs_old,
                                                 double error_norm, double error_norm_old)
{
    double mult = 1.0;
    const double ie = rcp(error_norm);           // +inf for error_norm == 0, as numpy's 0 ** -0.25
    if (have_old && error_norm != 0) mult = h_abs * rcp(h_abs_old) * root4(error_norm_old * ie);
    return fmin(1.0, mult) * root4(ie);
}

// The error estimate and the dense output of an accept with their roundings spelled out, as the listing of the literal
// forms has them (loaded_constants_in_estimate_and_accept): which product of a sum stays plain, which are fused, and
// that the first row of Q = Z^T P adds three rounded products.
__device__ __forceinline__ ZRow z_of_w_spelled(const KZ &kz, const double (&W)[3][3], int q)
{
#pragma clang fp contract(off)
    return {__builtin_fma(kz.T02, W[2][q], __builtin_fma(kz.T00, W[0][q], kz.T01 * W[1][q])),
            __builtin_fma(kz.T12, W[2][q], __builtin_fma(kz.T10, W[0][q], kz.T11 * W[1][q])),
            W[0][q] + W[1][q]};
}
__device__ __forceinline__ void estimate_spelled(const KZ &kz, const KE &ke, const ZRow &z, double ih, double fq, double ycq, double &err, double &esc)
{
#pragma clang fp contract(off)
    const double ZE = __builtin_fma(ke.E2, z.z2, __builtin_fma(ke.E1, z.z1, ke.E0 * z.z0));
    err = __builtin_fma(ZE, ih, fq);
    esc = __builtin_fma(fmax(fabs(ycq), fabs(ycq + z.z2)), kz.rtol, kz.atol);
}
__device__ __forceinline__ void dense_row_spelled(const KA &ka, const ZRow &z, double (&Q)[3])
{
#pragma clang fp contract(off)
    Q[0] = (z.z0 * ka.P[0] + z.z1 * ka.P[3]) + z.z2 * ka.P[6];
    Q[1] = __builtin_fma(ka.P[7], z.z2, __builtin_fma(ka.P[4], z.z1, ka.P[1] * z.z0));
    Q[2] = __builtin_fma(ka.P[8], z.z2, __builtin_fma(ka.P[2], z.z0, ka.P[5] * z.z1));
}

// ---------------------------------------------------------------- the solver state machine
// The per-reactor yes/no state of the solver lives in the bits of ONE VGPR (`fl` in step_kernel).  As separate
// `bool`s every one of them is a 64-bit lane mask in an SGPR pair for the whole loop -- two dozen of them exhaust
// the scalar register file and the compiler spills SGPRs through v_writelane / v_readlane.
struct Flag {
    uint32_t &w; const uint32_t m;
    __device__ __forceinline__ operator bool() const { return (w & m) != 0u; }
    __device__ __forceinline__ Flag &operator=(bool v) { w = v ? (w | m) : (w & ~m); return *this; }
    __device__ __forceinline__ Flag &operator=(const Flag &o) { return *this = (bool)o; }
    __device__ __forceinline__ Flag &operator|=(bool v) { w = v ? (w | m) : w; return *this; }
};

// The first three phases are the fresh solver's preamble.  With solver_preamble_ahead_of_loop a lane passes through them
// ahead of the trip loop, once per outer step, and enters the loop in PH_NEWTON with its stage values preset (flag
// `preset`): inside the loop a lane is then in one of the phases from PH_STEP_BEGIN on, and only PH_NEWTON, PH_ERR_REFINE
// and PH_FNEW evaluate anything -- the first in the stage block, the other two at the loop's single-point site.
enum Phase : int {
    PH_OUTER_BEGIN = 0, // start an outer step: f0 = f(y0) is evaluated ahead of the first trip  radau.py:303
    PH_INIT_STEP,       // f0 known: first half of select_initial_step (no evaluation needed)  common.py:111-119
    PH_F1,              // next evaluates f(y0 + h0 f0); its epilogue starts the first attempt  common.py:120-122
    PH_STEP_BEGIN,      // _step_impl prologue of every later step (no evaluation needed)   radau.py:399-424
    PH_ATTEMPT,         // (re)start an attempt with the current h_abs                      radau.py:426-448
    PH_NEWTON,          // one simplified-Newton iteration per trip (three evaluations)     radau.py:84-134
    PH_ERR_REFINE,      // second error estimate after a rejection (one evaluation)         radau.py:485-487
    PH_FNEW,            // step accepted and a fresh Jacobian asked for: evaluate f(y_new)   radau.py:500-539
    PH_DONE             // solve finished, failed or raised: wait for the wavefront's other reactors
};

struct SolverCounters { int nfev, njev, nlu, nsteps, nrej; };

// LDS of one wavefront, ONE array: [reactor constants | history base | factor store, reused between outer steps as StepIO]
template <int LV> struct LdsMap {
    static constexpr int RK_DOUBLES = RK_UNI * rk_maxr(LV) + rk_lane_doubles(LV);
    static constexpr int HIST_DOUBLES = rk_maxr(LV);                      // 2 x rk_maxr ints: history base, reactor index of each segment
    static constexpr int F_DOUBLES = FSlots<LV>::LDS_SLOTS * 64;
    static constexpr int IO_DOUBLES = (int)((sizeof(wts::StepIO) + 7) / 8);
    static constexpr int TAIL_DOUBLES = F_DOUBLES > IO_DOUBLES ? F_DOUBLES : IO_DOUBLES;
    // the exchange row of the ROW = false kernels (both(), from_partner()): 64 cells between the reactor constants and
    // the factor store.  A lane whose neighbour lies outside the wavefront reads up to 2^(LV-2) cells beyond either
    // end -- constants or factors of this same allocation, masked by the caller like every out-of-segment value.
    static constexpr int X_OFF = RK_DOUBLES + HIST_DOUBLES, X_DOUBLES = 64;
    static constexpr int F_OFF = (X_OFF + X_DOUBLES + 1) & ~1;       // 16-byte aligned: the factor store's cells are pairs
    static constexpr int TOTAL = F_OFF + TAIL_DOUBLES;
    static_assert(X_OFF >= (LV >= 2 ? (1 << (LV - 2)) : 0), "reads below the exchange row must stay inside the allocation");
};

// derivatives() at the NS points of one trip, section by section: pH properties of all points, temperature properties
// of all points, then the rows.  Each section fetches its own fp64 constants (scalar loads from the argument block)
// and its own share of the reactor constants (LDS), so neither is live outside it, and inside a section the NS
// evaluations are independent chains for the scheduler to interleave.
template <bool ROW, int NS, bool BAR = false>   // BAR: see row_fence
__device__ __forceinline__ void rhs_points(const Lane &L, const RKStore &ks, ArgPtr pa, const double (*y)[3], double (*F)[3], bool *bad,
                                           ZoneProps *keep = nullptr)   // keep: the zone-local properties of point 0, for num_jac
{
    PropPH pp[NS]; PropT pt[NS];
    {
        ArgPtr a = fresh(pa);
        const KP c = load_kp(&a->kt);
        const RK k = fetch_reactor(ks);
        double x[NS];
#pragma unroll
        for (int s = 0; s < NS; ++s) x[s] = y[s][SPH];
        prop_pH_n<NS, BAR>(c, k, x, pp);
    }
    __builtin_amdgcn_sched_barrier(0);   // the next section's constants are fetched when this one is through (SGPR budget)
    {
        ArgPtr a = fresh(pa);
        const KT c = load_kt(&a->kt);
        double x[NS];
#pragma unroll
        for (int s = 0; s < NS; ++s) x[s] = y[s][STT];
        prop_T_n<NS, BAR>(c, x, pt);
#pragma unroll
        for (int s = 0; s < NS; ++s) bad[s] = pt[s].bad;
    }
    {
        const RK k = fetch_reactor(ks);
#pragma unroll
        for (int s = 0; s < NS; ++s)
            rhs_rows<ROW>(L, k, pp[s].H, pp[s].iw, pp[s].bpos, pt[s].kT * pp[s].phi, pt[s].rho, y[s][SCL], y[s][STT], F[s]);
    }
    if (keep) { keep->H = pp[0].H; keep->iw = pp[0].iw; keep->phi = pp[0].phi; keep->bpos = pp[0].bpos; keep->kT = pt[0].kT; keep->rho = pt[0].rho; }
}

// Whether the probe's epilogue (PH_F1) also starts the first attempt, so that the trip that probed the step size goes on
// to the Jacobian, the factorisation and Newton iteration 1 with f(y0) as the three stage values.  The one switch for an
// instantiation whose register allocation or timing would take the join badly: without it the lane goes through
// PH_STEP_BEGIN / PH_ATTEMPT and a stage evaluation in the next trip, same results.  No instantiation needs it.
__host__ __device__ constexpr bool first_attempt_in_probe_trip(int /*LV*/, bool /*ROW*/) { return true; }
// Whether the fresh solver's preamble -- the first half of select_initial_step, the probe evaluation f(y0 + h0 f0) and
// the probe's epilogue with its first-attempt set-up -- runs once per outer step ahead of the trip loop, right behind
// f(y0) (needs outer_begin_ahead_of_first_trip and first_attempt_in_probe_trip).  The lanes then enter the loop in
// PH_NEWTON with their stage values preset, every trip of the loop is a Newton trip or one of the two rare single-point
// phases, and the loop carries neither the preamble's phase tests nor the per-phase selects of its first evaluation
// point.  Off: the first trip goes through PH_INIT_STEP and PH_F1 inside the loop, same results.  (The n > 32 kernel
// has its 60 B of scratch with it, and 68 B without it or without the single-point fence of wt_rhs.hpp.)
__host__ __device__ constexpr bool solver_preamble_ahead_of_loop(int /*LV*/, bool /*ROW*/) { return true; }

// Where a pending f is evaluated, one switch per piece; with a switch off that piece's path is the
// one the lane took before, same results.
// A: an outer step ends in the trip that accepts its last internal step.  f(y_new) of that step is not evaluated there:
// its first user is the next outer step, which evaluates it as its own f(y0) -- if it still needs it (the item may end,
// the state may be clamped, the boundary reloaded).  Off: the lane spends one more trip in PH_FNEW and carries f over.
__host__ __device__ constexpr bool outer_step_ends_at_accept(int /*LV*/, bool /*ROW*/) { return true; }
// B: f(y0) of an outer step that has none carried over is evaluated ahead of its first trip, so that the trip goes on
// to the probe, the Jacobian, the factorisation and Newton iteration 1.  Off: PH_OUTER_BEGIN takes a trip of its own.
__host__ __device__ constexpr bool outer_begin_ahead_of_first_trip(int /*LV*/, bool /*ROW*/) { return true; }
// C: the pending f(y_new) of a non-final accepted step is the fourth point of the stage block of the next Newton trip.
// Off: it is a single-point evaluation of its own right behind the block.
__host__ __device__ constexpr bool pending_f_in_stage_block(int /*LV*/, bool /*ROW*/) { return true; }
// D: the derived state (H+ concentration, density, decay rate) is formed when the item stores its results, from the
// pre-clamp state of the reactor's last live step; a step that clamps or leaves the temperature range forms it at once.
// Off: it is formed after every outer step.
__host__ __device__ constexpr bool derived_once_per_item(int /*LV*/, bool /*ROW*/) { return true; }
// E (needs B): the zone-local properties that B's evaluation forms at y0 are the base point's of the outer step's first
// Jacobian, in the same trip: num_jac takes them over.  Ten registers held from the evaluation to the Jacobian, which
// the n > 32 kernel does not have.  Off: num_jac forms them itself.
__host__ __device__ constexpr bool base_properties_handed_to_num_jac(int LV, bool /*ROW*/) { return LV <= 5; }
// F: the accept of an outer step's last internal step leaves the step-size controller and the dense output alone: they
// would serve a next internal step, and the next outer step is a fresh solver.  Off: every accept updates them.
__host__ __device__ constexpr bool lean_last_accept(int /*LV*/, bool /*ROW*/) { return true; }

// Whether the fences of the item's single-point evaluations (f(y0), the probe, the rare phases' points, num_jac, the
// post-step properties) are scheduling barriers without operands (row_fence in wt_rhs.hpp), which spares the hazard
// `s_nop` after every step of their chains.  At n = 8 it measures 0.8 % slower on top of the preamble piece, so the
// kernels for n <= 16 keep the asm form.  The n > 32 kernel has its 60 B of scratch with the barrier in the two n > 16
// kernels, and 64 to 68 B with it in that kernel alone or in none.
__host__ __device__ constexpr bool single_point_fence_is_barrier(int LV, bool /*ROW*/) { return LV >= 5; }

// Whether the error estimate and the accept take their Radau constants from the argument block (one scalar load per
// section, as the other sections do) with their roundings spelled out, and not as fp64 literals.
__host__ __device__ constexpr bool loaded_constants_in_estimate_and_accept(int LV, bool /*ROW*/) { return LV <= 5; }

// Data movement that computes nothing, one switch per piece; off is the code as it stood, same results.
// Whether the n = 8 partner exchange of the top cyclic-reduction level is the two-move form that needs no copy of its
// operand (from_partner<true, 4>, wt_lanes.hpp).  Only <3, true> has that exchange.
__host__ __device__ constexpr bool partner_exchange_without_copy(int /*LV*/, bool /*ROW*/) { return true; }
// Whether a trip's stage points and stage values (ye, Fe) are defined afresh where the trip declares them.  They are
// assigned on three paths; for a lane that takes none of them the compiler otherwise keeps the trip before's contents,
// which no lane ever reads, and carries them round the loop's back edge through accumulation registers (in <3, true>
// 36 + 41 v_accvgpr moves a trip and 30 registers; the n > 32 kernel has its 60 B of scratch for them).
__host__ __device__ constexpr bool stage_values_fresh_each_trip(int /*LV*/, bool /*ROW*/) { return true; }

// One work item: the reactors of wavefront-group `group` advanced by `cnt` outer steps, starting with step `step0`
// of this launch.  Reactors of a wavefront start every outer step together (they wait for the slowest of them), so
// their Jacobians, factorisations and Newton trips coincide, and the end of an outer step is a wave-uniform point
// where the sensor suite and the PLC scan run.
template <int LV, bool ROW>
__device__ __forceinline__ void run_item(ArgPtr pa, const Lane &L, double *lds, int group, int step0, int cnt)
{
    using M = LdsMap<LV>;
    ArgPtr a = fresh(pa);                             // ---- section: load the group
    const int n_zones = L.n, R = a->R;
    const int lane = threadIdx.x & 63, seg = lane / n_zones;
    const int64_t q_first = (int64_t)group * R;       // slots of this group; slot q holds reactor perm[q]
    const int64_t q_end = a->q_ctrl ? a->N : a->r1;
    const bool present = (seg < R) && (q_first + seg < q_end);
    const int64_t r = present ? (int64_t)a->perm[q_first + seg] : 0;
    const int64_t idx = r * n_zones + L.z;
    const double dt = a->dt;
    const int step_limit = a->step_limit, sens_on = a->sens.on, plc_on = a->sens.plc_on;
    const bool want_diag = a->wave_diag != nullptr;
    const RKStore ks = {lds + seg, lds + RK_UNI * rk_maxr(LV) + lane, rk_maxr(LV), L.m_lo[0], L.m_hi[0], rk_lane_in_lds(LV)};
    int *hist0 = reinterpret_cast<int *>(lds + M::RK_DOUBLES);
    int *rix = hist0 + rk_maxr(LV);                   // reactor index of each segment, for the sensor / PLC lanes
    double *lds_factors = lds + M::F_OFF;
    wts::StepIO &io = *reinterpret_cast<wts::StepIO *>(lds_factors);

    // ---- per-reactor state carried from one outer step to the next (segment-uniform scalars replicated in every lane)
    double y0[3] = {7.0, 1.0, 20.0};                  // state at the start of the outer step
    double f[3] = {0, 0, 0};                          // f(y0) when f_valid
    double t_out = 0;                                 // ReactorState.time
    double dH = 0, dR = 0, dK = 0, badval = 0;
    double flow_used = 0;                             // ReactorState.flow_rate: the flows of the last step taken
    uint32_t st = 0;
    bool frozen = !present, f_valid = false, wrote_k = false, raised = false;
    bool derive_due = false;                          // y0 is the pre-clamp state of a live step whose derived state is not formed yet
    constexpr bool END_AT_ACCEPT = outer_step_ends_at_accept(LV, ROW), BEGIN_AHEAD = outer_begin_ahead_of_first_trip(LV, ROW),
                   PEND_IN_BLOCK = pending_f_in_stage_block(LV, ROW), DERIVE_ONCE = derived_once_per_item(LV, ROW),
                   HAND_BASE = BEGIN_AHEAD && base_properties_handed_to_num_jac(LV, ROW), LEAN_LAST_ACCEPT = lean_last_accept(LV, ROW),
                   LOADED_EA = loaded_constants_in_estimate_and_accept(LV, ROW), FIRST_IN_PROBE = first_attempt_in_probe_trip(LV, ROW), BAR1 = single_point_fence_is_barrier(LV, ROW),
                   PRE_AHEAD = BEGIN_AHEAD && FIRST_IN_PROBE && solver_preamble_ahead_of_loop(LV, ROW),
                   FRESH_STAGES = stage_values_fresh_each_trip(LV, ROW);
    int steps_done = 0, reads_done = 0, cost_acc = 0;
    SolverCounters last_cnt = {0, 0, 0, 0, 0};
    int diag_trips = 0, diag_newton = 0;              // per item: 32 bits are plenty
#ifdef WT_STAMPS  // block-execution counters cost a ballot and a branch each per trip: diagnostic builds only
    int diag_fact = 0, diag_jac = 0, diag_f3 = 0;
#define WT_COUNT(c) ++(c)
#else
    constexpr int diag_fact = 0, diag_jac = 0, diag_f3 = 0;
#define WT_COUNT(c) do { } while (0)
#endif
#ifdef WT_STAMPS  // diagnostic build only: shader-clock shares of the loop's sections (never in the product .so)
    long long sec[8] = {0, 0, 0, 0, 0, 0, 0, 0}; long long tprev = __builtin_amdgcn_s_memtime();
#define WT_STAMP(i) do { const long long tn_ = __builtin_amdgcn_s_memtime(); sec[i] += tn_ - tprev; tprev = tn_; } while (0)
#else
#define WT_STAMP(i) do { } while (0)
#endif
    const long long clk0 = want_diag ? __builtin_amdgcn_s_memtime() : 0, wall0 = want_diag ? __builtin_amdgcn_s_memrealtime() : 0;
    if (present) {
        st = a->status[r];
        // a reactor whose last step raised stays frozen until the host rewrites its state
        if (st & (ST_T_RANGE | ST_T_RANGE_POST)) frozen = true;
        y0[SPH] = a->pH[idx]; y0[SCL] = a->Cl[idx]; y0[STT] = a->T[idx];
        t_out = a->time[r];
        // under a boundary schedule the item's first outer step integrates under its own row
        const double *bc = a->sched ? a->sched + (int64_t)(a->first_step + step0) * NB * a->N : a->bc;
        RK k0; load_reactor(a->par, bc, a->N, r, n_zones, k0); mask_reactor_for_lane(L, k0);
        park_reactor(ks, k0);
        if (sens_on && L.z == 0) hist0[seg] = a->sens.hist_value ? a->sens.hist_pos[r] : 0;
        if (L.z == 0) rix[seg] = (int)r;
    }

    for (int k = 0; k < cnt; ++k) {
        bool stepped = false;
        if (!frozen) {
          // scipy refuses a non-finite initial state: ValueError out of step(), self.state untouched (base.py:19-20)
          if (WT_RARE(seg_any(L, !(isfinite(y0[0]) && isfinite(y0[1]) && isfinite(y0[2]))))) { st |= ST_NONFINITE; frozen = true; }
          else {
            // ================= one IntegratedCSTR.step(): a fresh scipy solver object (reactor.py:476)
            double yc[3], W[3][3];                    // solver's current y; Newton iterate in transformed variables
            double aux[3] = {0, 0, 0};                // y0 + h0 f0 (initial step) / error vector (refinement)
            constexpr bool HELD = LV <= 5;           // (see Held; the n = 17...32 kernel holds all but the Jacobian: +0.7 %)
            typedef Held<HELD> AReg64;
            // dense output of the last accepted step: written when a step is accepted, read when the next attempt is set up
            AReg64 Qa[3][3], y_old_a[3], sol_t_old_a, sol_h_a;
#pragma unroll
            for (int q = 0; q < 3; ++q) { y_old_a[q].init(); Qa[q][0].init(); Qa[q][1].init(); Qa[q][2].init(); }
            sol_t_old_a.init(); sol_h_a.init();
            Jac J;                                    // num_jac's output; between its uses the Jacobian lives in `ja`
            JacA<(LV <= 4)> ja; ja.init();
            FStore<LV> F;
            F.cell = (LdsDouble2 *)lds_factors + lane;
            uint32_t fl = 1u << 4;                    // current_jac = true
            Flag have_fac{fl, 1u << 0}, have_old{fl, 1u << 1}, have_old_l{fl, 1u << 2}, have_sol{fl, 1u << 3}, current_jac{fl, 1u << 4},
                 have_lu{fl, 1u << 5}, rejected{fl, 1u << 6}, keep_h{fl, 1u << 7}, have_norm_old{fl, 1u << 8}, have_rate{fl, 1u << 9},
                 bad{fl, 1u << 10}, failed{fl, 1u << 11}, fv{fl, 1u << 12}, need_jac{fl, 1u << 13},
                 limit_hit{fl, 1u << 16}, pend_f{fl, 1u << 17}, jac_after_fnew{fl, 1u << 18},
                 j_dense{fl, 1u << 19},               // this lane's Jacobian couples a row to a neighbour's temperature
                 base_held{fl, 1u << 20}, base_bpos{fl, 1u << 21},   // zb_a holds the properties at yc; their beta > 0
                 preset{fl, 1u << 22};                // the stage values of this lane's next Newton iteration are f (PRE_AHEAD)
            fv = f_valid;
            AReg64 fac_a[3]; fac_a[0].init(); fac_a[1].init(); fac_a[2].init();   // num_jac's factors: touched once per Jacobian
            // H, iw, phi, kT, rho at y0 from the evaluation ahead of the first trip, for the Jacobian of that trip (HAND_BASE)
            AReg64 zb_a[5];
            if constexpr (HAND_BASE) { zb_a[0].init(); zb_a[1].init(); zb_a[2].init(); zb_a[3].init(); zb_a[4].init(); }
            double t = t_out, t_bound = t_out + dt, max_step = fmin(dt, 10.0);
            double h = 0, t_new = 0, h_abs = 0, h_abs_l = 0, min_step = 0;
            // the step-size controller's memory: written when a step is accepted / begun, read when the next one is judged
            AReg64 h_abs_old_a, err_old_a, h_abs_old_l_a, err_old_l_a;
            h_abs_old_a.init(); err_old_a.init(); h_abs_old_l_a.init(); err_old_l_a.init();
            int kk = 0, n_iter = 0; double dW_norm_old = 0, rate = 0;
            double error_norm = 0, safety = 0;
            double d0 = 0, d1 = 0, h0 = 0;            // select_initial_step
            SolverCounters cnt_s = {0, 0, 0, 0, 0};
            int attempts = 0;   // guard against unbounded solves (sliding along a discontinuity): see limit_hit
            int badstage = 0;   // which evaluation of the trip raised: 0 deferred f(y_new) / num_jac, 1..3 stage / single point
            // pend_f: f(yc) of the last accepted step has not been evaluated yet
            // jac_after_fnew: that step also asked for a fresh Jacobian (radau.py:500,512)
            int phase = PH_OUTER_BEGIN;
#pragma unroll
            for (int q = 0; q < 3; ++q) { yc[q] = y0[q]; W[0][q] = W[1][q] = W[2][q] = 0.0; }

            // select_initial_step (common.py:68-134), order 3, up to the probe point y0 + h0 f0
            auto initial_step_first_half = [&]() {
                double sc[3];
#pragma unroll
                for (int q = 0; q < 3; ++q) sc[q] = ATOL + fabs(yc[q]) * RTOL;
                d0 = rms3<ROW, LV>(L, yc, sc); d1 = rms3<ROW, LV>(L, f, sc);
                h0 = (d0 < 1e-5 || d1 < 1e-5) ? 1e-6 : 0.01 * d0 * rcp(d1);
                h0 = fmin(h0, fabs(t_bound - t));
#pragma unroll
                for (int q = 0; q < 3; ++q) aux[q] = yc[q] + h0 * f[q];
            };
            // the probe's epilogue: fp = f(y0 + h0 f0) gives the second half of select_initial_step (common.py:120-134)
            auto probe_epilogue = [&](const double *fp) {
                double sc[3], df[3];
#pragma unroll
                for (int q = 0; q < 3; ++q) { sc[q] = ATOL + fabs(yc[q]) * RTOL; df[q] = fp[q] - f[q]; }
                const double d2 = rms3<ROW, LV, 0>(L, df, sc) * rcp(h0);
                double h1;
                if (d1 <= 1e-15 && d2 <= 1e-15) h1 = fmax(1e-6, h0 * 1e-3);
                else h1 = root4(0.01 * rcp(fmax(d1, d2)));
                h_abs = fmin(fmin(100 * h0, h1), fmin(fabs(t_bound - t), max_step));
                need_jac = true;                                          // radau.py:359-365
                if constexpr (!FIRST_IN_PROBE) phase = PH_STEP_BEGIN;
                else {
                    // ---- the first attempt of this fresh solver, here and not in a trip of its own: what PH_STEP_BEGIN and
                    // PH_ATTEMPT do when nothing has been attempted yet.  have_old_l, rejected, keep_h, have_norm_old and
                    // have_rate are still false, kk, rate and W still the zeros the outer step declared them with.  Neither
                    // guard of PH_ATTEMPT can fire: attempts == 0, and h_abs <= max_step from the line above, so h_abs_l
                    // is h_abs or min_step.
                    min_step = 10 * fabs(ulp_above(t));                  // radau.py:408
                    h_abs_l = (h_abs < min_step) ? min_step : h_abs;
                    attempts++;
                    h = h_abs_l;
                    t_new = t + h;
                    if (t_new - t_bound > 0) t_new = t_bound;
                    h = t_new - t;
                    h_abs_l = fabs(h);
                    // Z0 = 0 without a dense output, and the RHS has no time argument: the three stage points are yc, their
                    // values the f this lane holds, bit for bit (one rounding behaviour per expression); counted as scipy
                    // does.  The caller hands f to the Newton iteration as its three stage values.
                    cnt_s.nfev += 3;
                    phase = PH_NEWTON;
                }
            };
            // error_norm > 1: radau.py:489-496
            auto reject_step = [&]() {
                const double fct = predict_factor(h_abs_l, have_old_l, h_abs_old_l_a.get(), error_norm, err_old_l_a.get());
                h_abs_l *= fmax(MIN_FACTOR, safety * fct);
                have_lu = false; rejected = true; cnt_s.nrej++;
                phase = PH_ATTEMPT;
            };
            // step accepted: radau.py:500-539.  scipy evaluates f(y_new) right here; the value is first
            // needed by the next error estimate, so unless a Jacobian refresh needs it at once, it is
            // evaluated together with the next Newton trip (pend_f) -- or, where the accept ends the outer
            // step, by the next outer step as its f(y0) (END_AT_ACCEPT).
            auto accept_step = [&]() {
                const bool recompute_jac = (n_iter > 2) && have_rate && (rate > 1e-3);
                const bool more = (t_new - t_bound) < 0;
                // The accept that ends the outer step prepares no further internal step: the next step size and the dense output
                // belong to a solver object that the reference discards with the outer step (reactor.py:476).
                if (!LEAN_LAST_ACCEPT || more) {
                    double fct = predict_factor(h_abs_l, have_old_l, h_abs_old_l_a.get(), error_norm, err_old_l_a.get());
                    fct = fmin(MAX_FACTOR, safety * fct);
                    if (!recompute_jac && fct < 1.2) fct = 1.0; else have_lu = false;
                    h_abs_old_a.set(h_abs);       // sic radau.py:520: the solver-level value
                    err_old_a.set(error_norm);
                    have_old = true;
                    h_abs = h_abs_l * fct;
                    if constexpr (LOADED_EA) {
                        const RTabPtr rt = &fresh(pa)->rt;
                        const KZ kz = load_kz(rt); const KA ka = load_ka(rt);
#pragma unroll
                        for (int q = 0; q < 3; ++q) {
                            double Qr[3];
                            dense_row_spelled(ka, z_of_w_spelled(kz, W, q), Qr);
                            y_old_a[q].set(yc[q]);
                            Qa[q][0].set(Qr[0]); Qa[q][1].set(Qr[1]); Qa[q][2].set(Qr[2]);
                        }
                    } else {
                    const KZ kz = lit_kz(); const KA ka = lit_ka();
#pragma unroll
                    for (int q = 0; q < 3; ++q) {
                        const ZRow z = z_of_w(kz, W, q);
                        y_old_a[q].set(yc[q]);
                        Qa[q][0].set(z.z0 * ka.P[0] + z.z1 * ka.P[3] + z.z2 * ka.P[6]);  // Q = Z^T P  radau.py:541-543
                        Qa[q][1].set(z.z0 * ka.P[1] + z.z1 * ka.P[4] + z.z2 * ka.P[7]);
                        Qa[q][2].set(z.z0 * ka.P[2] + z.z1 * ka.P[5] + z.z2 * ka.P[8]);
                    }
                    }
                    sol_t_old_a.set(t); sol_h_a.set(t_new - t); have_sol = true;
                }
                {
                    const KZ kz = lit_kz();
#pragma unroll
                    for (int q = 0; q < 3; ++q) yc[q] = yc[q] + z_of_w(kz, W, q).z2;   // y_new = y + Z[2]
                }
                t = t_new;
                cnt_s.nsteps++; cnt_s.nfev++;     // f(y_new) counted where scipy calls it
                pend_f = true; fv = false;
                current_jac = recompute_jac;
                if (recompute_jac || (!END_AT_ACCEPT && !more)) { jac_after_fnew = recompute_jac; phase = PH_FNEW; }
                else if (!more) {
                    // the outer step ends here, f(y_new) pending (fv stays false: the next outer step begins with its own
                    // evaluation).  The reference raises out of f(y_new) when a zone of y_new is outside the temperature
                    // range, state untouched: prop_T's own test, NaN passing as it does there.
                    const bool out = (yc[STT] < 0.0) || (yc[STT] > 100.0);
                    if (WT_RARE(seg_any(L, out))) {
                        if (out) { badstage = 0; badval = yc[STT]; }
                        bad |= out; raised = true;
                    }
                    phase = PH_DONE;
                }
                else phase = PH_STEP_BEGIN;
            };

            WT_STAMP(1);   // outer-step set-up (slot 1 also takes the step / attempt prologues inside the loop)
            if (fv) {
                // f(y0) is already in f (last evaluation of the previous outer step, same y, same
                // boundary): count it as scipy does and go straight to the initial-step probe
                cnt_s.nfev++;
                phase = PH_INIT_STEP;
            }
            if constexpr (BEGIN_AHEAD) {
                // A lane is in PH_OUTER_BEGIN in the first trip of its outer step and in no other, so the evaluation at the top
                // of that trip stands here, ahead of the loop: f0 = f(y0), and the first trip goes through PH_INIT_STEP to the
                // probe and on.  A temperature outside the range raises as in a trip of its own (first evaluation, stage 1).
                if (__ballot(phase == PH_OUTER_BEGIN) != 0ull) {
                    double fy[1][3]; bool bb[1];
                    ZoneProps zb;
                    rhs_points<ROW, 1, BAR1>(L, ks, pa, &yc, fy, bb, HAND_BASE ? &zb : nullptr);
                    const bool mine = bb[0] && phase == PH_OUTER_BEGIN;
                    if (phase == PH_OUTER_BEGIN) {
                        if constexpr (HAND_BASE) {
                            zb_a[0].set(zb.H); zb_a[1].set(zb.iw); zb_a[2].set(zb.phi); zb_a[3].set(zb.kT); zb_a[4].set(zb.rho);
                            base_bpos = zb.bpos; base_held = true;
                        }
                        cnt_s.nfev++;
#pragma unroll
                        for (int q = 0; q < 3; ++q) f[q] = fy[0][q];
                        phase = PH_INIT_STEP;
                    }
                    if (WT_RARE(__ballot(mine) != 0ull)) {
                        if (mine) { badstage = 1; badval = yc[STT]; }
                        bad |= mine;
                        if (seg_any(L, bad)) { raised = true; phase = PH_DONE; }
                    }
                }
            }
            if constexpr (PRE_AHEAD) {
                // Every lane that starts a solve holds f(y0) now, evaluated just above or carried over: the rest of the fresh
                // solver's preamble, once per outer step.  The lanes leave it in PH_NEWTON with `preset` (or in PH_DONE: a
                // probe point outside the temperature range ends the lane before any attempt), so inside the loop no lane is
                // ever in PH_OUTER_BEGIN, PH_INIT_STEP or PH_F1.  The probe keeps no properties: those handed to num_jac are
                // the ones at y0.
                if (__ballot(phase == PH_INIT_STEP) != 0ull) {
                    if (phase == PH_INIT_STEP) {      // the one copy of this arithmetic, whether f0 was evaluated or carried over
                        initial_step_first_half();
                        phase = PH_F1;
                    }
                    double fy[1][3]; bool bb[1];
                    rhs_points<ROW, 1, BAR1>(L, ks, pa, &aux, fy, bb);
                    const bool mine = bb[0] && phase == PH_F1;
                    if (phase == PH_F1) cnt_s.nfev++;
                    if (WT_RARE(__ballot(mine) != 0ull)) {
                        if (mine && !bad) { badstage = 1; badval = aux[STT]; }
                        bad |= mine;
                        if (seg_any(L, bad)) { raised = true; phase = PH_DONE; }
                    }
                    if (phase == PH_F1) { probe_epilogue(fy[0]); preset = true; }
                }
            }
            WT_STAMP(0);   // the solver's preamble alone: f(y0), the initial step's first half, the probe and its epilogue
            while (true) {
                // reactors that finished their outer step wait here until every reactor of the wavefront has
                if (__ballot(phase != PH_DONE) == 0ull) break;
                // ================= trips that need no RHS evaluation (run first so the lane can join this trip's evaluation)
                if constexpr (!PRE_AHEAD) {
                    if (phase == PH_INIT_STEP) {  // the one copy of this arithmetic, whether f0 was evaluated or carried over
                        initial_step_first_half();
                        phase = PH_F1;
                    }
                }
                if (phase == PH_STEP_BEGIN) {
                    min_step = 10 * fabs(ulp_above(t));                      // radau.py:408
                    if (h_abs > max_step) { h_abs_l = max_step; have_old_l = false; }
                    else if (h_abs < min_step) { h_abs_l = min_step; have_old_l = false; }
                    else { h_abs_l = h_abs; have_old_l = have_old; h_abs_old_l_a.set(h_abs_old_a.get()); err_old_l_a.set(err_old_a.get()); }
                    rejected = false; keep_h = false;
                    phase = PH_ATTEMPT;
                }
                if (phase == PH_ATTEMPT) {
                    if (!keep_h) {
                        if (WT_RARE(step_limit > 0 && attempts >= step_limit)) { failed = true; limit_hit = true; phase = PH_DONE; }
                        else if (WT_RARE(h_abs_l < min_step)) { failed = true; phase = PH_DONE; }  // radau.py:427-428
                        else {
                            attempts++;
                            h = h_abs_l;
                            t_new = t + h;
                            if (t_new - t_bound > 0) t_new = t_bound;
                            h = t_new - t;
                            h_abs_l = fabs(h);
                        }
                    }
                    if (phase == PH_ATTEMPT) {
                        keep_h = false;
                        // initial guess Z0 (radau.py:445-448,557-572) and W = TI Z0 (radau.py:88)
                        double Z0[3][3];
                        if (!have_sol) {
#pragma unroll
                            for (int s = 0; s < 3; ++s)
#pragma unroll
                                for (int q = 0; q < 3; ++q) Z0[s][q] = 0.0;
                        } else {
                            const double sol_t_old = sol_t_old_a.get(), isol = rcp(sol_h_a.get());
                            double Q[3][3], y_old[3];
#pragma unroll
                            for (int q = 0; q < 3; ++q) { y_old[q] = y_old_a[q].get(); Q[q][0] = Qa[q][0].get(); Q[q][1] = Qa[q][1].get(); Q[q][2] = Qa[q][2].get(); }
                            const KG kg = load_kg(&fresh(pa)->rt);
                            const double cs[3] = {kg.C0, kg.C1, 1.0};
#pragma unroll
                            for (int s = 0; s < 3; ++s) {
                                const double x = ((t + h * cs[s]) - sol_t_old) * isol;
                                const double p1 = x * x, p2 = p1 * x;
#pragma unroll
                                for (int q = 0; q < 3; ++q)
                                    // (which products fuse is spelled out: the polynomial's rounding steers Newton's start)
                                    Z0[s][q] = (__builtin_fma(Q[q][2], p2, __builtin_fma(Q[q][0], x, Q[q][1] * p1)) + y_old[q]) - yc[q];
                            }
                        }
                        const KN kn0 = load_kn(&fresh(pa)->rt);
#pragma unroll
                        for (int q = 0; q < 3; ++q) {
                            W[0][q] = kn0.TI[0] * Z0[0][q] + kn0.TI[1] * Z0[1][q] + kn0.TI[2] * Z0[2][q];
                            W[1][q] = kn0.TI[3] * Z0[0][q] + kn0.TI[4] * Z0[1][q] + kn0.TI[5] * Z0[2][q];
                            W[2][q] = kn0.TI[6] * Z0[0][q] + kn0.TI[7] * Z0[1][q] + kn0.TI[8] * Z0[2][q];
                        }
                        kk = 0; have_norm_old = false; have_rate = false; rate = 0.0;
                        phase = PH_NEWTON;
                    }
                }
                WT_STAMP(1);   // step / attempt prologues
                // ================= this trip's evaluation points
                const bool newton = (phase == PH_NEWTON);
                diag_trips++;
                // the lanes whose point is slot 0 of this trip's evaluation; with PRE_AHEAD the stage block is the Newton lanes'
                // alone, and the two rare phases that evaluate one point of their own have the single-point site to themselves
                const bool single = PRE_AHEAD && (phase == PH_ERR_REFINE || phase == PH_FNEW);
                const bool eval0 = PRE_AHEAD ? newton
                                             : ((!BEGIN_AHEAD && phase == PH_OUTER_BEGIN) || phase == PH_F1 || phase == PH_ERR_REFINE || phase == PH_FNEW || newton);
                // f(y) of a just-accepted step rides along with the next attempt's first Newton trip
                const bool eval3 = newton && pend_f;
                constexpr int NPT = PEND_IN_BLOCK ? 4 : 3;   // the stage block's points: the three stages, then the pending point
                double ye[NPT][3], Fe[NPT][3];
                if constexpr (FRESH_STAGES) {
#pragma unroll
                    for (int s = 0; s < NPT; ++s)
#pragma unroll
                        for (int q = 0; q < 3; ++q) { ye[s][q] = undefined_f64(); Fe[s][q] = undefined_f64(); }
                }
                if constexpr (!PRE_AHEAD) {
#pragma unroll
                    for (int q = 0; q < 3; ++q) {
                        double p0 = yc[q];                                    // PH_OUTER_BEGIN, PH_FNEW
                        if (phase == PH_F1) p0 = aux[q];
                        if (phase == PH_ERR_REFINE) p0 = yc[q] + aux[q];
                        ye[0][q] = p0;
                    }
                }
                // Z = T W (radau.py:124): Z[2] = W0 + W1 -- the stage points
                auto stage_points = [&]() {
                    const KZ kzp = load_kz(&fresh(pa)->rt);
#pragma unroll
                    for (int q = 0; q < 3; ++q) {
                        const ZRow z = z_of_w(kzp, W, q);
                        if (PRE_AHEAD || newton) ye[0][q] = yc[q] + z.z0;
                        ye[1][q] = yc[q] + z.z1; ye[2][q] = yc[q] + z.z2;
                    }
                };
                // formed only on trips that evaluate them (+1 % at n = 8) -- except in the n = 17...32 kernel, where the
                // extra block measures 0.6 % slower (and, before its solver state was restructured, cost a private segment)
                if constexpr (LV >= 5) stage_points();
                bool b0 = false, b1 = false, b2 = false, b3 = false;
                // (with PRE_AHEAD a lane comes out of the preamble with its stage values preset: all lanes of the wavefront do so
                // in the same trip, the first of the outer step, and that trip has no stage block)
                if (__ballot(newton && !(PRE_AHEAD && preset)) != 0ull) {
                    if constexpr (LV < 5) stage_points();
                    // some reactor of the wavefront is in its Newton phase: all three stage points (three independent
                    // chains for the scheduler to interleave); the other lanes' slot-1/2 results are simply not used
                    bool bb[NPT];
                    bool four = false;
                    if constexpr (PEND_IN_BLOCK) four = __ballot(eval3) != 0ull;
                    if (four) {
                        // some Newton lane has a pending f(y_new): a fourth chain in the same sections, with their constants
                        if constexpr (PEND_IN_BLOCK) {
                            WT_COUNT(diag_f3);
#pragma unroll
                            for (int q = 0; q < 3; ++q) ye[NPT - 1][q] = yc[q];
                            rhs_points<ROW, NPT>(L, ks, pa, ye, Fe, bb);
                            b3 = bb[NPT - 1] && eval3;
                            if (eval3) {
                                pend_f = false;   // (counted in nfev when the step was accepted)
#pragma unroll
                                for (int q = 0; q < 3; ++q) f[q] = Fe[NPT - 1][q];
                            }
                        }
                    } else {
                        rhs_points<ROW, 3>(L, ks, pa, ye, Fe, bb);
                    }
                    b0 = bb[0] && eval0; b1 = bb[1] && newton; b2 = bb[2] && newton;
                    if (eval0 && phase != PH_FNEW) cnt_s.nfev++;
                    if (newton) cnt_s.nfev += 2;
                } else if (PRE_AHEAD && __ballot(newton && preset) != 0ull) {
                    // Z0 = 0 and the RHS has no time argument: the three stage values are f(y0), which the lane holds
#pragma unroll
                    for (int s = 0; s < 3; ++s)
#pragma unroll
                        for (int q = 0; q < 3; ++q) Fe[s][q] = f[q];
                } else if (!PRE_AHEAD && __ballot(eval0) != 0ull) {
                    bool bb[1];
                    rhs_points<ROW, 1, BAR1>(L, ks, pa, ye, Fe, bb);
                    b0 = bb[0] && eval0;
                    if (eval0 && phase != PH_FNEW) cnt_s.nfev++;
                }
                if (PRE_AHEAD && WT_RARE(__ballot(single) != 0ull)) {
                    // the second error estimate's point and f(y_new) ahead of a Jacobian refresh: the loop's single-point site
                    double yp[1][3], fy[1][3]; bool bb[1];
#pragma unroll
                    for (int q = 0; q < 3; ++q) yp[0][q] = (phase == PH_ERR_REFINE) ? yc[q] + aux[q] : yc[q];
                    rhs_points<ROW, 1, BAR1>(L, ks, pa, yp, fy, bb);
                    if (single) {
#pragma unroll
                        for (int q = 0; q < 3; ++q) { ye[0][q] = yp[0][q]; Fe[0][q] = fy[0][q]; }
                        b0 = bb[0];
                        if (phase == PH_ERR_REFINE) cnt_s.nfev++;
                    }
                }
                if (!PEND_IN_BLOCK && __ballot(eval3) != 0ull) {
                    WT_COUNT(diag_f3);
                    double fy[1][3]; bool bb[1];
                    rhs_points<ROW, 1, BAR1>(L, ks, pa, &yc, fy, bb);
                    b3 = bb[0] && eval3;
                    if (eval3) {
                        pend_f = false;       // (counted in nfev when the step was accepted)
#pragma unroll
                        for (int q = 0; q < 3; ++q) f[q] = fy[0][q];
                    }
                }
                if (WT_RARE(__ballot(b0 || b1 || b2 || b3) != 0ull)) {   // rare: a zone temperature outside [0, 100] C
                    // the reference raises in the first evaluation, at the first zone, that sees it: scipy calls
                    // f(y_new) of the accepted step before the stages of the next Newton iteration
                    const bool mine = b0 || b1 || b2 || b3;
                    if (mine && !bad) {
                        badstage = b3 ? 0 : (b0 ? 1 : (b1 ? 2 : 3));
                        badval = b3 ? yc[STT] : (b0 ? ye[0][STT] : (b1 ? ye[1][STT] : ye[2][STT]));
                    }
                    bad |= mine;
                    if (seg_any(L, bad)) { raised = true; phase = PH_DONE; }
                }

                // ================= the epilogues of the phases that are not Newton's: they may ask for a Jacobian, and the probe's
                // starts the first attempt, so they come before num_jac, the factorisation and the Newton epilogue of this same trip
                if (!BEGIN_AHEAD && WT_RARE(phase == PH_OUTER_BEGIN)) {   // (with BEGIN_AHEAD no lane is in this phase inside the loop)
#pragma unroll
                    for (int q = 0; q < 3; ++q) f[q] = Fe[0][q];
                    phase = PH_INIT_STEP;
                } else if (!PRE_AHEAD && phase == PH_F1) {     // (with PRE_AHEAD the probe and its epilogue stand ahead of the loop)
                    probe_epilogue(Fe[0]);
                    if constexpr (FIRST_IN_PROBE) {
#pragma unroll
                        for (int s = 0; s < 3; ++s)
#pragma unroll
                            for (int q = 0; q < 3; ++q) Fe[s][q] = f[q];
                    }
                } else if (phase == PH_FNEW) {
                    // f(y_new) of an accepted step that needs it before anything else can happen:
                    // Jacobian refresh (radau.py:512-514) or the end of the outer step
#pragma unroll
                    for (int q = 0; q < 3; ++q) f[q] = Fe[0][q];
                    pend_f = false;
                    fv = true;
                    if (jac_after_fnew) { need_jac = true; jac_after_fnew = false; }
                    phase = ((t - t_bound) < 0) ? PH_STEP_BEGIN : PH_DONE;
                }

                WT_STAMP(3);   // RHS evaluations, epilogues of the phases that are not Newton's
                // ================= finite-difference Jacobian at (yc, f) when a phase asked for it: the probe and PH_FNEW just now,
                // a Newton iteration that diverged on an old Jacobian in the trip before (its retry's stage points are evaluated
                // above, the reference's after its jac call: a bad column here takes precedence over a bad stage point)
#ifdef WT_STAMPS
                if (__ballot(need_jac) != 0ull) WT_COUNT(diag_jac);
#endif
                if (need_jac) {
                    bool jbad = false, hf = have_fac, jd = false; double jval = 0;
                    asm volatile("" ::: "memory");               // a fresh fetch: do not keep the constants live across the epilogue
                    double fac[3] = {fac_a[0].get(), fac_a[1].get(), fac_a[2].get()};
                    if constexpr (HAND_BASE) {
                        // the first Jacobian of an outer step that began with its own evaluation is taken at that point, yc = y0
                        // untouched since: its base properties are the held ones.  Any later Jacobian forms its own.
                        const ZoneProps zb = {zb_a[0].get(), zb_a[1].get(), zb_a[2].get(), zb_a[3].get(), zb_a[4].get(), (bool)base_bpos};
                        num_jac<ROW, BAR1>(L, ks, [&]() { return &fresh(pa)->kt; }, yc, f, fac, hf, J, jbad, jval, jd, &zb, (bool)base_held);
                        base_held = false;
                    } else {
                        num_jac<ROW, BAR1>(L, ks, [&]() { return &fresh(pa)->kt; }, yc, f, fac, hf, J, jbad, jval, jd);
                    }
                    cnt_s.njev++;
                    fac_a[0].set(fac[0]); fac_a[1].set(fac[1]); fac_a[2].set(fac[2]);
                    have_fac = hf;
                    j_dense = jd;
                    ja.put(J);
                    need_jac = false;
                    if (WT_RARE(seg_any(L, jbad))) {
                        if (jbad) { badstage = 0; badval = jval; }
                        bad |= jbad; raised = true; phase = PH_DONE;
                    }
                }
                WT_STAMP(5);   // num_jac
#ifdef WT_STAMPS
                if (__ballot(phase == PH_NEWTON && !have_lu) != 0ull) WT_COUNT(diag_fact);
#endif
                if (phase == PH_NEWTON && !have_lu) {
                    { Jac Jb; ja.bands(Jb); factorize<ROW, LV>(L, Jb, h, F); } have_lu = true; cnt_s.nlu += 2;      // radau.py:454-456
                }

                WT_STAMP(2);   // factorisation
                // ================= the Newton iteration and the second error estimate
                if (__ballot(phase == PH_NEWTON) != 0ull) diag_newton++;
                if (phase == PH_NEWTON) {
                    // ---- one iteration of solve_collocation_system radau.py:84-134
                    Jac Jc; ja.coupling(Jc);
                    if constexpr (PRE_AHEAD) preset = false;
                    bool finite = true;
#pragma unroll
                    for (int s = 0; s < 3; ++s)
#pragma unroll
                        for (int q = 0; q < 3; ++q) finite = finite && isfinite(Fe[s][q]);
                    bool conv = false, diverged = false;
                    if (WT_RARE(!seg_all(L, finite))) {
                        diverged = true;
                    } else {
                        const double ih = rcp(h);
                        const RTabPtr rt = &fresh(pa)->rt;
                        const KN kn = load_kn(rt); const KZ kz = load_kz(rt);
                        const double M_real = kn.mu_r * ih, Mcr = kn.mu_cr * ih, Mci = kn.mu_ci * ih;
                        double fr[3], fcr[3], fci[3], scale[3];
#pragma unroll
                        for (int q = 0; q < 3; ++q) {
                            scale[q] = kz.atol + fabs(yc[q]) * kz.rtol;
                            fr[q] = (Fe[0][q] * kn.TI[0] + Fe[1][q] * kn.TI[1] + Fe[2][q] * kn.TI[2]) - M_real * W[0][q];
                            const double re = Fe[0][q] * kn.TI[3] + Fe[1][q] * kn.TI[4] + Fe[2][q] * kn.TI[5];
                            const double im = Fe[0][q] * kn.TI[6] + Fe[1][q] * kn.TI[7] + Fe[2][q] * kn.TI[8];
                            fcr[q] = re - (Mcr * W[1][q] - Mci * W[2][q]);
                            fci[q] = im - (Mcr * W[2][q] + Mci * W[1][q]);
                        }
                        solve_rc<ROW, LV>(L, Jc, F, fr, fcr, fci, __ballot(j_dense) == 0ull);
                        double ssum = 0.0;
#pragma unroll
                        for (int q = 0; q < 3; ++q) {
                            const double is = rcp(scale[q]);
                            const double u = fr[q] * is, v = fcr[q] * is, w = fci[q] * is;
                            ssum += u * u + v * v + w * w;
                        }
                        const double dW_norm = sqrt_k(div_by(seg_sum<ROW, LV>(L, ssum), L.d9n));
                        if (have_norm_old) { rate = dW_norm * rcp(dW_norm_old); have_rate = true; }
                        const double i1r = rcp(1 - rate);
                        if (have_rate && (rate >= 1 || powi6(rate, NEWTON_MAXITER - kk) * i1r * dW_norm > kn.newton_tol)) {
                            diverged = true;
                        } else {
#pragma unroll
                            for (int q = 0; q < 3; ++q) { W[0][q] += fr[q]; W[1][q] += fcr[q]; W[2][q] += fci[q]; }
                            if (dW_norm == 0 || (have_rate && rate * i1r * dW_norm < kn.newton_tol)) conv = true;
                            dW_norm_old = dW_norm; have_norm_old = true;
                        }
                    }
                    n_iter = kk + 1;
                    kk++;
                    if (!conv && !diverged && kk == NEWTON_MAXITER) diverged = true;   // loop ran out: radau.py:136
                    if (WT_RARE(diverged)) {                                          // radau.py:462-476
                        if (current_jac) { h_abs_l *= 0.5; have_lu = false; cnt_s.nrej++; phase = PH_ATTEMPT; }
                        else { need_jac = true; current_jac = true; have_lu = false; keep_h = true; phase = PH_ATTEMPT; }
                    } else if (conv) {
                        // ---- error estimate radau.py:477-487
                        double err[3], esc[3];
                        const double ih_e = rcp(h);
                        if constexpr (LOADED_EA) {
                            const RTabPtr rte = &fresh(pa)->rt;
                            const KZ kze = load_kz(rte); const KE ke = load_ke(rte);
#pragma unroll
                            for (int q = 0; q < 3; ++q) estimate_spelled(kze, ke, z_of_w_spelled(kze, W, q), ih_e, f[q], yc[q], err[q], esc[q]);
                        } else {
                        const KZ kze = lit_kz(); const KE ke = lit_ke();
#pragma unroll
                        for (int q = 0; q < 3; ++q) {
                            const ZRow z = z_of_w(kze, W, q);
                            const double ZE = (z.z0 * ke.E0 + z.z1 * ke.E1 + z.z2 * ke.E2) * ih_e;
                            err[q] = f[q] + ZE;
                            esc[q] = kze.atol + fmax(fabs(yc[q]), fabs(yc[q] + z.z2)) * kze.rtol;
                        }
                        }
                        solve_real<ROW, LV>(L, Jc, F, err, __ballot(j_dense) == 0ull);
                        error_norm = rms3<ROW, LV>(L, err, esc);
                        safety = 0.9 * (2 * NEWTON_MAXITER + 1) / (2 * NEWTON_MAXITER + n_iter);
                        if (WT_RARE(rejected && error_norm > 1)) {
#pragma unroll
                            for (int q = 0; q < 3; ++q) aux[q] = err[q];
                            phase = PH_ERR_REFINE;
                        } else if (WT_RARE(error_norm > 1)) {                         // radau.py:489-496
                            reject_step();
                        } else {
                            accept_step();
                        }
                    }
                } else if (WT_RARE(phase == PH_ERR_REFINE)) {
                    Jac Jc; ja.coupling(Jc);
                    double err[3], esc[3];
                    const double ih_e = rcp(h);
                    if constexpr (LOADED_EA) {
                        const RTabPtr rte = &fresh(pa)->rt;
                        const KZ kze = load_kz(rte); const KE ke = load_ke(rte);
#pragma unroll
                        for (int q = 0; q < 3; ++q) estimate_spelled(kze, ke, z_of_w_spelled(kze, W, q), ih_e, Fe[0][q], yc[q], err[q], esc[q]);
                    } else {
                    const KZ kze = lit_kz(); const KE ke = lit_ke();
#pragma unroll
                    for (int q = 0; q < 3; ++q) {
                        const ZRow z = z_of_w(kze, W, q);
                        const double ZE = (z.z0 * ke.E0 + z.z1 * ke.E1 + z.z2 * ke.E2) * ih_e;
                        err[q] = Fe[0][q] + ZE;
                        esc[q] = kze.atol + fmax(fabs(yc[q]), fabs(yc[q] + z.z2)) * kze.rtol;
                    }
                    }
                    solve_real<ROW, LV>(L, Jc, F, err, __ballot(j_dense) == 0ull);
                    error_norm = rms3<ROW, LV>(L, err, esc);
                    if (error_norm > 1) reject_step(); else accept_step();
                }
                WT_STAMP(4);   // Newton solve, error estimates, accept / reject
            }
            last_cnt = cnt_s;
            cost_acc += cnt_s.nfev;

            // ================= after the solve: reactor.py:486-507
            if (WT_RARE(raised)) {
                // the reference raised (thermodynamics.py:146-157): self.state untouched; name the temperature its
                // message names -- first evaluation of the trip, lowest zone
                st |= ST_T_RANGE; frozen = true;
                double v = badval; int best = 1 << 30;
#pragma unroll 1
                for (int sidx = 0; sidx < 5; ++sidx) {
                    const unsigned long long m = __ballot(bad && badstage == sidx) & L.segmask;
                    if (m != 0ull && best == (1 << 30)) { best = sidx; v = __shfl(badval, (int)__builtin_ctzll(m), 64); }
                }
                badval = v;
                raised = false;
            } else {
                if (failed) st |= ST_SOLVER_FAILED;    // reactor.py:486-487; state <- last accepted y
                if (limit_hit) st |= ST_STEP_LIMIT;
                const double T_before = y0[STT];       // (read on one rare path below)
#pragma unroll
                for (int q = 0; q < 3; ++q) y0[q] = yc[q];
                stepped = true; steps_done++;
                t_out = t_out + dt;                    // reactor.py:496
                flow_used = ks.uni[15 * ks.stride];    // reactor.py:497-501
                // The derived state is stored when the item ends and read by nothing before, so an ordinary step only notes
                // that it is due: the item's end forms it from y0, the pre-clamp state of the last live step.  A step that
                // leaves the temperature range or clamps takes the path below, which forms it at once.
                bool ordinary = false;
                if constexpr (DERIVE_ONCE) {
                    const bool odd = (y0[STT] < 0.0) || (y0[STT] > 100.0)        // prop_T's own test (T_RANGE_POST, CLAMP_T)
                                  || (y0[SPH] < 0) || (y0[SPH] > 14) || (y0[SCL] < 0);
                    ordinary = !WT_RARE(seg_any(L, odd));
                }
                if (ordinary) {
                    derive_due = true;
                    f_valid = fv && !failed;
                } else {
                    // _update_derived_state reactor.py:511-524 (before the clamp)
                    double dHv; PropT pt;
                    if (DERIVE_ONCE && derive_due) {
                        // the step before this one was ordinary: should this one leave the range, its decay rate is the one that stays
                        dK = prop_T<BAR1>(load_kt(&fresh(pa)->kt), T_before).kT; wrote_k = true;
                        derive_due = false;
                    }
                    {
                        ArgPtr a2 = fresh(pa);
                        const KP cp = load_kp(&a2->kt); const KT ct = load_kt(&a2->kt);
                        dHv = exp10_k(cp, -y0[SPH]); pt = prop_T<BAR1>(ct, y0[STT]);
                    }
                    dH = dHv;
                    dR = pt.rho;
                    bool clamped = false;
                    if (WT_RARE(seg_any(L, pt.bad))) {
                        st |= ST_T_RANGE_POST; frozen = true;
                        const unsigned long long m = __ballot(pt.bad) & L.segmask;
                        badval = __shfl(y0[STT], (int)__builtin_ctzll(m), 64);
                    } else {
                        dK = pt.kT; wrote_k = true;
                        // _enforce_physical_bounds reactor.py:526-541
                        if (WT_RARE(seg_any(L, y0[SPH] < 0 || y0[SPH] > 14))) { st |= ST_CLAMP_PH; y0[SPH] = fmin(fmax(y0[SPH], 0.0), 14.0); clamped = true; }
                        if (WT_RARE(seg_any(L, y0[SCL] < 0))) { st |= ST_CLAMP_CL; y0[SCL] = fmax(y0[SCL], 0.0); clamped = true; }
                        if (WT_RARE(seg_any(L, y0[STT] < 0 || y0[STT] > 100))) { st |= ST_CLAMP_T; y0[STT] = fmin(fmax(y0[STT], 0.0), 100.0); clamped = true; }
                        // f(y) of the last accepted point is f0 of the next outer step when nothing touched y
                        f_valid = fv && !clamped && !failed;
                    }
                }
            }
          }
        }

        WT_STAMP(6);       // post-step (derived, clamps)
        // ================= the score program (wave-uniform flag): excursion metrics of the true state after the step.
        // It reads y0 and t_out and writes its own arrays only: no reload of the reactor constants, f(y0) stays valid.
        if constexpr (prog_in_item(LV)) {
          if (WT_RARE(fresh(pa)->scr.on)) {
            ArgPtr s = fresh(pa);            // ---- section: score program
            static_assert(M::TAIL_DOUBLES >= wtsc::STAGE_DOUBLES, "the score program stages the zones' state in the factor store");
            const bool live = present && stepped && !(st & ST_T_RANGE_POST);   // the sensor section's test
            wtsc::evaluate(s->scr, live, L.z, n_zones, lane, L.base, r, t_out, y0, lds_factors,
                           s->scr.step0 + s->first_step + step0 + k);
          }
        }
        // ================= the disturbance program and the train program (wave-uniform flags): the rows of the next
        // outer step.  Before the plant-I/O section, whose scan reload then reads these rows from the boundary block
        // while the command path writes rows 0 / 4 / 6 -- neither overwrites the other's rows.  A disturbance slot never
        // targets a row the train feeds (the set calls refuse it), so the two write different cells; one barrier and one
        // reload serve both.
        if constexpr (prog_in_item(LV)) {
          const int dst_on = fresh(pa)->dst.on, trn_on = fresh(pa)->trn.on;
          if (WT_RARE((dst_on | trn_on) != 0)) {
            ArgPtr d = fresh(pa);            // ---- section: disturbance program, train program
            const bool live = present && stepped && !(st & ST_T_RANGE_POST);   // the sensor section's test
            bool reload = false;
            // a junction program reads the row 0 that was in force during this step, before this section stores anything
            double q0 = 0.0;
            if (trn_on && d->trn.jct.on && present && !L.has_hi) q0 = d->bc[r];
            if (dst_on) {
                if (live && L.z == 0) wtd::evaluate(d->dst, r, t_out, d->bc, d->N, ExpK());
                reload = live;
            }
            // a stage's outlet lane stores its state into the next stage's rows 1..3; fed: this lane's reactor got rows
            static_assert(M::TAIL_DOUBLES >= wtr::PARK_Q * wtr::PARK_SEGS, "a junction program parks the outlets in the factor store");
            if (trn_on) reload = wtr::feed(d->trn, present, live, !L.has_hi, seg, n_zones, r, t_out, y0, q0, d->bc, d->N, lds_factors, JctK()) || reload;
            __syncthreads();                 // the rows are in memory for every lane of the reactor
            if (reload) {
                RK k1; load_reactor(d->par, d->bc, d->N, r, n_zones, k1); mask_reactor_for_lane(L, k1);
                park_reactor(ks, k1);
                f_valid = false;
            }
          }
        }
        // ================= what follows reactor.step() in the reference's loop body (__main__.py:403-423)
        if (sens_on) {
            ArgPtr b = fresh(pa);            // ---- section: sensors and plant I/O
            __syncthreads();                 // the factor store is dead now; the same LDS carries the hand-off
            if (seg < R) {
                const bool live = stepped && !(st & ST_T_RANGE_POST);     // the reference's loop stops where step() raises
                if (L.z == 0) {
                    io.stepped[seg] = live ? 1 : 0;
                    if (live) reads_done++;
                    io.t_after[seg] = t_out;
                    io.tap[0][seg] = (float)y0[SPH]; io.tap[2][seg] = (float)y0[SCL]; io.tap[4][seg] = (float)y0[STT];
                    io.tap[6][seg] = (float)flow_used;
                }
                if (!L.has_hi) { io.tap[1][seg] = (float)y0[SPH]; io.tap[3][seg] = (float)y0[SCL]; io.tap[5][seg] = (float)y0[STT]; }
            }
            __syncthreads();
            // read_all_sensors; then the service program (wave-uniform flag), which the n > 32 kernel leaves out
            if constexpr (prog_in_item(LV)) wts::suite_step(b->sens, b->ins, io, rix, R, hist0, k, wtsv::Program());
            else wts::suite_step(b->sens, b->ins, io, rix, R, hist0, k);
            if (plc_on) {
                const int gs = b->first_step + step0 + k;
                const bool scan = ((gs + 1) % b->sens.scan_every == 0) || (gs + 1 == b->call_steps);
                __syncthreads();
                // the wire program (wave-uniform flags), before everything else in the scan: wired slots of a scan lane's
                // column get the readings of another stage's instruments.  One barrier inside, between gather and
                // scatter; none after it -- what follows reads the lane's own column only (wt_wir.hpp).
                if constexpr (prog_in_item(LV)) {
                  if (scan && WT_RARE(fresh(pa)->wir.on)) {
                    ArgPtr wp = fresh(pa);
                    wtw::route(wp->wir, wp->trn.length, lane < R && io.stepped[lane], lane, rix, io);
                  }
                }
                if (lane < R && io.stepped[lane]) {                       // one lane per reactor
                    const int64_t rr = rix[lane];
                    const double lt = b->sens.pack.loop_time[rr];
                    if (scan) {
                        // an injection program (wave-uniform flag) tampers with this lane's copy of the readings and
                        // with the decoded commands; t is the loop time this scan stores.  Not in the n > 32 kernel.
                        // a link program (wave-uniform flag) comes first on both paths: what the fieldbus delivers of this
                        // lane's readings and of the decoded commands is what an injection tampers with (wt_lnk.hpp)
                        const bool lnk = prog_in_item(LV) && WT_RARE(fresh(pa)->lnk.on);
                        const bool inj = prog_in_item(LV) && WT_RARE(fresh(pa)->inj.on);
                        if (lnk) wtl::link_sensors(fresh(pa)->lnk, fresh(pa)->sens.reactor_base, rr, &io.val[0][lane], &io.fault[0][lane], wts::RMAX, lt + dt);
                        if (inj) wti::tamper_sensors(fresh(pa)->inj, rr, &io.val[0][lane], &io.fault[0][lane], wts::RMAX, lt + dt);
                        wtp::pack_inputs(b->sens.pack, rr, &io.val[0][lane], &io.fault[0][lane], wts::RMAX, lt);   // update_modbus_inputs
                        double c[3];
                        // an actuator program (wave-uniform flag) needs the inlet row as it was before this scan
                        const bool act = prog_in_item(LV) && WT_RARE(fresh(pa)->act.on);
                        const double row0 = act ? b->sens.cmd.bc[rr] : 0.0;
                        double inlet_v;
                        if (lnk) inlet_v = wtp::apply_commands(b->sens.cmd, rr, c, wtl::link_then_tamper(fresh(pa)->lnk, fresh(pa)->inj, inj, fresh(pa)->sens.reactor_base, rr, lt + dt));
                        else if (inj) inlet_v = wtp::apply_commands(b->sens.cmd, rr, c, wti::command_tamper(fresh(pa)->inj, rr, lt + dt));
                        else inlet_v = wtp::apply_commands(b->sens.cmd, rr, c);    // read_modbus_commands + apply_boundary_conditions
                        // an alarm program's trips in force (from the previous scan) replace the validated commands
                        if (prog_in_item(LV) && WT_RARE(fresh(pa)->alm.on)) wta::override_commands(fresh(pa)->alm, b->sens.cmd, rr, c);
                        // the final elements, downstream of the whole command path: their positions are what the plant gets
                        if (act) wtv::actuate(fresh(pa)->act, b->sens.cmd, rr, c, inlet_v, row0, lt + dt);
                        io.cmd[0][lane] = c[0]; io.cmd[1][lane] = c[1]; io.cmd[2][lane] = c[2];
                    }
                    b->sens.pack.loop_time[rr] = lt + dt;                 // sim_time += dt (__main__.py:446)
                }
                // the tune program (wave-uniform flag), immediately before the PLC program and with its inputs: a relay
                // experiment owns its loop's holding words; owned: the loops the PLC program skips in this scan
                int owned = 0;
                if constexpr (prog_in_item(LV)) {
                  if (scan && WT_RARE(fresh(pa)->tun.on) && lane < R && io.stepped[lane]) {
                    ArgPtr up = fresh(pa);
                    const int64_t rr = rix[lane];
                    owned = wtu::tune_execute(up->tun, up->ctl, rr, &io.val[0][lane], &io.fault[0][lane], wts::RMAX, up->sens.pack.loop_time[rr]);
                  }
                }
                // the response program (wave-uniform flag), directly after the tune program and before the controllers: a
                // slot that is engaged holds its loop's words as a relay experiment does, except where the tuner has the
                // loop in this scan (wt_rsp.hpp).  The controllers and the PLC program see one mask.
                if constexpr (prog_in_item(LV)) {
                  if (scan && WT_RARE(fresh(pa)->rsp.on) && lane < R && io.stepped[lane]) {
                    ArgPtr rp = fresh(pa);
                    const int64_t rr = rix[lane];
                    owned |= wtrp::respond_execute(rp->rsp, rp->ctl, rp->alm, rp->det, rp->mpc, rr, &io.val[0][lane], &io.fault[0][lane],
                                                   wts::RMAX, rp->sens.pack.loop_time[rr], owned);
                  }
                }
                // the model predictive controllers (wave-uniform flag), between the tune program and the PLC program and
                // with their inputs.  The whole wavefront enters: a scan lane decides, all 64 lanes carry the reactor's
                // prediction (wt_mpc.hpp).  A controller owns its loop's holding words as a relay experiment does.
                if constexpr (prog_in_item(LV)) {
                  if (scan && WT_RARE(fresh(pa)->mpc.on)) {
                    ArgPtr mp = fresh(pa);
                    owned |= wtm::mpc_execute(mp->mpc, mp->ctl, lane < R && io.stepped[lane], lane, rix, &io.val[0][0], &io.fault[0][0],
                                              wts::RMAX, mp->sens.pack.loop_time, owned);
                  }
                }
                // the PLC program, after the scan's command path: its commands act from the next scan on, like a host
                // master's between two calls; t_now is the loop time just stored
                if (scan && WT_RARE(fresh(pa)->ctl.on) && lane < R && io.stepped[lane]) {
                    ArgPtr cp = fresh(pa);
                    const int64_t rr = rix[lane];
                    wtc::pi_execute(cp->ctl, rr, &io.val[0][lane], &io.fault[0][lane], wts::RMAX, cp->sens.pack.loop_time[rr], owned);
                }
                // the alarm program, after the PLC program: IMAGE slots read this lane's (possibly tampered) copy,
                // FIELD slots what the sensor lanes stored before the barrier above; its trips act from the next scan on
                if (prog_in_item(LV) && scan && WT_RARE(fresh(pa)->alm.on) && lane < R && io.stepped[lane]) {
                    ArgPtr ap = fresh(pa);
                    const int64_t rr = rix[lane];
                    wta::evaluate(ap->alm, rr, ap->sens.N, &io.val[0][lane], &io.fault[0][lane], wts::RMAX, ap->sens.out_value,
                                  ap->sens.out_fault, ap->sens.pack.loop_time[rr]);
                }
                // the detector program, after the alarm program: the same inputs as the alarm program's, its own arrays only
                if constexpr (prog_in_item(LV)) {
                  if (scan && WT_RARE(fresh(pa)->det.on) && lane < R && io.stepped[lane]) {
                    ArgPtr dp = fresh(pa);
                    const int64_t rr = rix[lane];
                    wtk::evaluate(dp->det, rr, dp->sens.N, &io.val[0][lane], &io.fault[0][lane], wts::RMAX, dp->sens.out_value,
                                  dp->sens.out_fault, dp->sens.pack.loop_time[rr]);
                  }
                }
                // the trend recorder, last in the scan: what this lane's programs left in their records, its own arrays only
                if constexpr (prog_in_item(LV)) {
                  if (scan && WT_RARE(fresh(pa)->trd.on) && lane < R && io.stepped[lane]) {
                    ArgPtr tp = fresh(pa);
                    const int64_t rr = rix[lane];
                    wtt::record(*tp, rr, &io.val[0][lane], &io.fault[0][lane], &io.cmd[0][lane], wts::RMAX, tp->sens.pack.loop_time[rr]);
                  }
                }
                if (scan) {
                    __syncthreads();
                    if (present && io.stepped[seg]) {                    // the next step integrates under the new setpoints
                        RK k0; load_reactor(b->par, b->bc, b->N, r, n_zones, k0, &io.cmd[0][seg], wts::RMAX); mask_reactor_for_lane(L, k0);
                        park_reactor(ks, k0);
                        f_valid = false;
                    }
                }
            }
            __syncthreads();                 // hand-off read; the next step's factors may overwrite it
        }
        // The n > 32 kernel has no register to spare for this section (any fp64 store here costs it scratch): the host
        // runs its forced / recorded calls one outer step per launch instead (x_in_item).
        if constexpr (x_in_item(LV)) {
          if (WT_RARE(fresh(pa)->x_on)) {
            ArgPtr x = fresh(pa);            // ---- section: trajectory record, next row of the boundary schedule
            const int gs = x->first_step + step0 + k;
            if (x->rec_pH) {
                // what wt_ensemble_get_snapshot would return now (a reactor that did not step keeps what memory holds);
                // 32-bit arithmetic: the host folds the steps before this call into rec_phase / rec_slot0
                const unsigned m = (unsigned)x->rec_phase + (unsigned)gs + 1u, every = (unsigned)x->rec_every;
                const unsigned slot = (unsigned)x->rec_slot0 + m / every - 1u;
                if (m % every == 0u && slot < (unsigned)x->rec_cap && present) {
                    const int64_t row = (int64_t)slot * x->N;
                    const int64_t o = row * n_zones + idx;
                    x->rec_pH[o] = y0[SPH]; x->rec_Cl[o] = y0[SCL]; x->rec_T[o] = y0[STT];
                    if (L.z == 0) {
                        x->rec_time[row + r] = t_out;
                        x->rec_flow[row + r] = steps_done > 0 ? flow_used : x->flow[r];
                        x->rec_status[row + r] = st;
                    }
                }
            }
            if (x->sched && k + 1 < cnt) {
                // the PLC scan's reload (above) with the next row: the next step integrates under its own boundary
                if (present) {
                    RK k1; load_reactor(x->par, x->sched + (int64_t)(gs + 1) * NB * x->N, x->N, r, n_zones, k1);
                    mask_reactor_for_lane(L, k1);
                    park_reactor(ks, k1);
                }
                f_valid = false;
            }
          }
        }
        WT_STAMP(7);       // sensor suite, plant I/O, forcing, recording
    }

    // ================= the item's results
    if constexpr (DERIVE_ONCE) {
        // _update_derived_state reactor.py:511-524 of the last live step, whose pre-clamp state y0 still is (a reactor that
        // froze afterwards left y0 alone, a step that clamped formed its own)
        if (derive_due) {
            ArgPtr a2 = fresh(pa);
            const KP cp = load_kp(&a2->kt); const KT ct = load_kt(&a2->kt);
            const PropT pt = prop_T<BAR1>(ct, y0[STT]);
            dH = exp10_k(cp, -y0[SPH]); dR = pt.rho; dK = pt.kT; wrote_k = true;
        }
    }
    ArgPtr c = fresh(pa);
    if (present) {
        if (steps_done > 0) {
            c->pH[idx] = y0[SPH]; c->Cl[idx] = y0[SCL]; c->T[idx] = y0[STT];
            c->dH[idx] = dH; c->dRho[idx] = dR;
            if (wrote_k) c->dK[idx] = dK;
        }
        if (L.z == 0) {
            if (steps_done > 0) {
                c->time[r] = t_out;
                c->flow[r] = flow_used;
                if (c->stats) {
                    int32_t *o = c->stats + r * 5;
                    o[0] = last_cnt.nfev; o[1] = last_cnt.njev; o[2] = last_cnt.nlu; o[3] = last_cnt.nsteps; o[4] = last_cnt.nrej;
                }
                if (sens_on && c->sens.hist_value) c->sens.hist_pos[r] = hist0[seg] + reads_done;
            }
            c->status[r] = st;
            if (st & (ST_T_RANGE | ST_T_RANGE_POST)) c->bad_T[r] = badval;
            if (c->cost && cost_acc > 0) c->cost[r] += cost_acc;
        }
    }
    if (want_diag && lane == 0) {
        unsigned long long *o = reinterpret_cast<unsigned long long *>(c->wave_diag + (int64_t)group * WT_DIAG_SLOTS);
        atomicAdd(o + 0, (unsigned long long)diag_trips); atomicAdd(o + 1, (unsigned long long)diag_newton);
        atomicAdd(o + 2, (unsigned long long)(__builtin_amdgcn_s_memtime() - clk0));
        atomicAdd(o + 3, (unsigned long long)(__builtin_amdgcn_s_memrealtime() - wall0));
        atomicAdd(o + 4, (unsigned long long)diag_fact); atomicAdd(o + 5, (unsigned long long)diag_jac);
        atomicAdd(o + 6, (unsigned long long)diag_f3); atomicAdd(o + 7, 1ull);
#ifdef WT_STAMPS
        for (int i = 0; i < 8; ++i) atomicAdd(o + 8 + i, (unsigned long long)sec[i]);
#endif
    }
}

} // namespace wt
