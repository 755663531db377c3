// wt_trn.hpp -- gfx950 device code of the train program (wt_ensemble_train_*): reactors coupled into treatment trains.
// An ensemble of N reactors is read as N / length trains of `length` stages; reactor r is stage r % length of train
// r / length.  After every outer step its upstream took, a linked stage gets the upstream's outlet zone (zone n - 1:
// pH, Cl, T) in rows 1, 2, 3 of its boundary block -- the boundary of its next outer step (zero-order hold).  Flows
// are not carried: row 0 belongs to the command path or the master, every tank keeps its own inlet flow.
//
//   feed      runs in the end-of-outer-step section of run_item that the disturbance program shares, before the
//             sensor and plant-I/O section.  The host deals whole trains into consecutive slots of one
//             wavefront-group (h->R is a multiple of length, wt_place.hpp deals units of length), so the upstream of
//             the reactor in segment s sits in segment s - 1 of the same wavefront and has just ended the same outer
//             step: the upstream's outlet lane stores its own state into the downstream's rows (vector stores, no
//             LDS), and the downstream's lanes learn from one ballot whether they were fed.
//   host_op   one thread per reactor: FEED writes every link from the state in memory (train_set, set_boundary and
//             set_state with a program set), RESTORE writes the base back into the linked rows (clear, a set over a
//             program).
//
// Device layout (indexed by reactor: placement changes nothing):
//   lk   [N] int32        0: not linked; otherwise LINKED | rows mask (1 pH, 2 Cl, 4 T)
//   st   [N][NTRS] fp64   n_fed (feeds written by the step kernel), t_last (the upstream's time at the last of them)
//   base [3][N] fp64      rows 1..3 as wt_ensemble_set_boundary last gave them
//
// The pipe program (wt_ensemble_pipe_*) sits on top of a train program: link d (into reactor d) may carry a delay line
// of D = delay[d] outer steps.  A sample is (pH, Cl, T of the upstream's outlet zone, the upstream's time).  The line
// is a ring of D + 1 slots in device memory: a feed stores the current sample at slot head, loads slot
// (head + 1) % (D + 1) -- the sample of D feeds ago -- delivers that one and makes its slot the head.  Between feeds
// slot head therefore holds the sample last delivered (what FEED of host_op writes again), and the D slots after it,
// in ring order, the samples in flight, oldest first.  Inside the step kernel the upstream's outlet lane is the only
// lane that touches link d's line; the item hand-off orders its accesses across items as it orders those to st.  A
// link with D = 0 has no line and takes the code path of a handle without a pipe program.
//   delay [N] int32               D per link, 0 where there is no line
//   head  [N] int32               the ring's head slot
//   ring  [slots][PIPE_Q][N] fp64 slots = (largest D) + 1; reactor d uses slots 0 .. delay[d]
//   st    [N][NPS] fp64           n_sent (feeds through the line inside step calls), t_sent (the time stamp of the
//                                 sample last delivered by one; NaN: none yet, or one of the initial fill)
//
// The junction program (wt_ensemble_junction_*) sits on top of a train program too: a linked reactor with at least one
// used source slot (stage g, share f) is a junction, fed by the flow-weighted blend of its sources' outlet zones and
// not by stage - 1 (include/wtphys.h has the arithmetic; blend() below is the one copy of it on the device).  A source
// is any other stage of the same train, so it sits in this wavefront at segment seg - stage + g (the wire program's
// rule).  Inside the step kernel every outlet lane parks (pH, Cl, T, time, row 0, live) of its reactor in the factor
// store, which is dead at the end of an outer step; after one barrier the junction's own outlet lane reads its sources'
// cells, blends, passes the sample through the junction's line (it is the only lane that touches that line) and stores
// the rows, and one ballot tells the junction's lanes whether they were fed.  Row 0 (the row in force during the step
// just taken: plant I/O writes it after this section) is read first and parked before the barrier, so every read of a
// row 0 precedes every store of a carried flow.
//   src   [N] uint32              slot k in bits 6 k .. 6 k + 5: USED (bit 5) | stage g (bits 0..4); CARRY in bit 24
//   share [JCT_SLOTS][N] fp64     f per slot
//   st    [N][NJS] fp64           n_blend, n_held, q_last
//   base0 [N] fp64                row 0 as wt_ensemble_set_boundary last gave it (what clear restores for a carrier)
//   tmp   [JCT_TMP][N] fp64       host_op scratch: BLEND leaves (pH, Cl, T, time, Qs) here, FEED and PIPE_FILL read it
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace wtr {

constexpr int NTR = 2, NTRS = 2, FED_ROWS = 3, LINKED = 8;
enum { P_LINK = 0, P_ROWS };
enum { S_N_FED = 0, S_T_LAST };

constexpr int NPS = 2, PIPE_Q = 4, PIPE_MAX_DELAY = 4095;
enum { PS_N_SENT = 0, PS_T_SENT };

struct PipeArgs {
    int on;                  // 0: no pipe program (feed reads this flag only)
    int slots;               // ring slots: the largest delay + 1
    const int32_t *delay;    // [N]
    int32_t *head;           // [N]
    double *ring;            // [slots][PIPE_Q][N]
    double *st;              // [N][NPS]
};

constexpr int JCT_SLOTS = 4, NJ = 2, NJS = 3, JCT_BITS = 6, JCT_TMP = 5, PARK_Q = 6, PARK_SEGS = 32;
constexpr uint32_t JCT_USED = 1u << 5, JCT_CARRY = 1u << 24, JCT_ANY = JCT_USED * 0x041041u;   // USED of the four slots
enum { J_STAGE = 0, J_SHARE };
enum { JS_N_BLEND = 0, JS_N_HELD, JS_Q_LAST };

struct JctArgs {
    int on;                  // 0: no junction program (feed reads this flag only)
    const uint32_t *src;     // [N]
    const double *share;     // [JCT_SLOTS][N]
    double *st;              // [N][NJS]
    double *base0;           // [N]
    double *tmp;             // [JCT_TMP][N]
};

struct TrnArgs {
    int on;                  // 0: no program (the step kernel's section reads this flag only)
    int length;              // stages per train
    const int32_t *lk;       // [N]
    double *st;              // [N][NTRS]
    double *base;            // [FED_ROWS][N]
    PipeArgs pipe;           // the pipe program on top (pipe.on == 0: none)
    JctArgs jct;             // the junction program on top (jct.on == 0: none)
};

__host__ __device__ constexpr uint32_t jct_slot_word(int k, int stage) { return (JCT_USED | (uint32_t)stage) << (JCT_BITS * k); }

// (P: PipeArgs in whichever address space the caller's arguments live)
template <class P> __device__ __forceinline__ double *ring_slot(const P &p, int slot, int64_t N, int64_t d)
{
    return p.ring + (int64_t)slot * PIPE_Q * N + d;
}

// One feed through the line of link d (delay D >= 1): s[0..3] = (pH, Cl, T, time) goes in, the sample of D feeds ago
// comes out in s.  Only the upstream's outlet lane (or host_op's thread d) calls it.
template <class P> __device__ __forceinline__ void pipe_feed(const P &p, int D, int64_t N, int64_t d, double s[PIPE_Q])
{
    const int h = p.head[d];
    const int nh = h >= D ? 0 : h + 1;                    // (head + 1) % (D + 1), head in 0..D
    double *in = ring_slot(p, h, N, d);
#pragma unroll
    for (int q = 0; q < PIPE_Q; ++q) in[q * N] = s[q];
    const double *out = ring_slot(p, nh, N, d);           // D >= 1: another slot than `in`
#pragma unroll
    for (int q = 0; q < PIPE_Q; ++q) s[q] = out[q * N];
    p.head[d] = nh;
    double *st = p.st + d * NPS;
    st[PS_N_SENT] = st[PS_N_SENT] + 1.0; st[PS_T_SENT] = s[3];
}

// the rows of reactor d that word w names, from (pH, Cl, T)
__device__ __forceinline__ void store_rows(int w, double *bc, int64_t N, int64_t d, double pH, double Cl, double T)
{
    if (w & 1) bc[1 * N + d] = pH;
    if (w & 2) bc[2 * N + d] = Cl;
    if (w & 4) bc[3 * N + d] = T;
}

// The blend of the junction word w of reactor r, slots in order: s = (pH, Cl, T, time stamp) of the sample, Qs the summed
// flow; returns the number of used slots.  source(g, v) gives stage g's (pH, Cl, T, time, row 0) and returns whether
// it is live; all / any: every / some source was.  One source: its values unchanged.  Two or more: flow-weighted means
// of H+ = 10^-pH, chlorine and temperature, every product and sum rounded (nothing contracted), IEEE division, then
// the clamps of the disturbance program's rows 1..3.  The slot loop stays rolled (see wt_wir.hpp).
template <class Source, class E>
__device__ __forceinline__ int blend(uint32_t w, const double *share, int64_t N, int64_t r, Source source, E fn,
                                     double s[PIPE_Q], double &Qs, bool &all, bool &any)
{
#pragma clang fp contract(off)
    double aH = 0.0, aCl = 0.0, aT = 0.0;
    int m = 0;
    Qs = 0.0; all = true; any = false;
#pragma unroll 1
    for (int k = 0; k < JCT_SLOTS; ++k) {
        const uint32_t c = w >> (JCT_BITS * k);
        if (c & JCT_USED) {
            double v[5];
            const bool up = source((int)(c & 31u), v);
            all = all && up; any = any || up;
            const double Q = share[k * N + r] * v[4];
            if (m == 0) { s[0] = v[0]; s[1] = v[1]; s[2] = v[2]; s[3] = v[3]; }
            const double QH = Q * fn.exp10(-v[0]), QCl = Q * v[1], QT = Q * v[2];
            Qs = Qs + Q; aH = aH + QH; aCl = aCl + QCl; aT = aT + QT;
            ++m;
        }
    }
    if (m >= 2) {
        const double H = aH / Qs, Cl = aCl / Qs, T = aT / Qs;
        s[0] = fmin(fmax(fn.pH_of(H), 0.0), 14.0);
        s[1] = fmax(Cl, 0.0);
        s[2] = fmin(fmax(T, 0.0), 100.0);
    }
    return m;
}

// The junction path of feed (below): park holds PARK_Q rows of PARK_SEGS cells, dead LDS of this wavefront; q0: row 0
// of reactor r as it was in force during the step just taken.  Returns whether this lane's reactor was fed.
template <class A, class E>
__device__ __forceinline__ bool feed_junctions(const A &a, bool present, bool live, bool outlet, int seg, int n_zones, int64_t r,
                                               double t, const double y[3], double q0, double *bc, int64_t N, double *park,
                                               E fn)
{
    const int stage = (int)((uint32_t)r % (uint32_t)a.length);
    __syncthreads();                                      // whoever read this LDS before is through
    if (outlet && seg < PARK_SEGS) {
        double *c = park + seg;
        c[0 * PARK_SEGS] = y[0]; c[1 * PARK_SEGS] = y[1]; c[2 * PARK_SEGS] = y[2]; c[3 * PARK_SEGS] = t; c[4 * PARK_SEGS] = q0;
        c[5 * PARK_SEGS] = live ? 1.0 : 0.0;
    }
    __syncthreads();                                      // every source is parked, every row 0 read
    const int w = present ? a.lk[r] : 0;
    const uint32_t jw = w ? a.jct.src[r] : 0u;
    bool fed = false;
    if (outlet && seg < PARK_SEGS && w) {
        double q[PIPE_Q], Qs = 0.0;
        bool all = true, any = false, carry = false;
        if (jw & JCT_ANY) {
            const double *first = park + (seg - stage);   // the cell of the train's stage 0
            const int m = blend(jw, a.jct.share, N, r, [&](int g, double v[5]) {
                const double *c = first + g;
                v[0] = c[0 * PARK_SEGS]; v[1] = c[1 * PARK_SEGS]; v[2] = c[2 * PARK_SEGS]; v[3] = c[3 * PARK_SEGS]; v[4] = c[4 * PARK_SEGS];
                return c[5 * PARK_SEGS] != 0.0; }, fn, q, Qs, all, any);
            (void)m;
            fed = all && Qs > 0.0;
            carry = (jw & JCT_CARRY) != 0u;
            double *js = a.jct.st + r * NJS;
            if (fed) { js[JS_N_BLEND] = js[JS_N_BLEND] + 1.0; js[JS_Q_LAST] = Qs; }
            else if (any) js[JS_N_HELD] = js[JS_N_HELD] + 1.0;
        } else {                                          // a plain link: the upstream's cell, as it is
            const double *c = park + (seg - 1);
            q[0] = c[0 * PARK_SEGS]; q[1] = c[1 * PARK_SEGS]; q[2] = c[2 * PARK_SEGS]; q[3] = c[3 * PARK_SEGS];
            fed = c[5 * PARK_SEGS] != 0.0;
        }
        if (fed) {
            const double ts = q[3];
            const int D = a.pipe.on ? a.pipe.delay[r] : 0;
            if (D > 0) pipe_feed(a.pipe, D, N, r, q);
            store_rows(w, bc, N, r, q[0], q[1], q[2]);
            if (carry) bc[r] = Qs;
            double *s = a.st + r * NTRS;
            s[S_N_FED] = s[S_N_FED] + 1.0; s[S_T_LAST] = ts;
        }
    }
    const unsigned long long m = __ballot(fed);
    const int out = (seg * n_zones + n_zones - 1) & 63;   // this segment's outlet lane
    return ((m >> out) & 1ull) != 0ull;
}

// One outer step's feeds of a wavefront; every lane calls it.  live: this lane's reactor r stepped and its state
// stands (the sensor section's test); outlet: this lane holds zone n - 1; y: the lane's state after the step; t: the
// reactor's time after it.  Returns whether this lane's reactor was fed (its lanes then reload the reactor constants).
// With a junction program (a.jct.on, wave-uniform) the whole wavefront takes feed_junctions, plain links included:
// the same stores and the same bits, made by the fed reactor's own outlet lane.  present: the lane has a reactor;
// q0, park, fn: see feed_junctions.
template <class A, class E>
__device__ __forceinline__ bool feed(const A &a, bool present, bool live, bool outlet, int seg, int n_zones, int64_t r, double t,
                                     const double y[3], double q0, double *bc, int64_t N, double *park, E fn)
{
    if (a.jct.on) return feed_junctions(a, present, live, outlet, seg, n_zones, r, t, y, q0, bc, N, park, fn);
    const int stage = (int)((uint32_t)r % (uint32_t)a.length);   // (reactor indices fit 31 bits: perm is int32)
    if (live && outlet && stage != a.length - 1) {
        const int64_t d = r + 1;                          // segment seg + 1 of this wavefront
        const int w = a.lk[d];
        if (w) {
            const int D = a.pipe.on ? a.pipe.delay[d] : 0;
            if (D > 0) {                                  // through the line: the sample of D feeds ago is delivered
                double q[PIPE_Q] = {y[0], y[1], y[2], t};
                pipe_feed(a.pipe, D, N, d, q);
                store_rows(w, bc, N, d, q[0], q[1], q[2]);
            } else {
                store_rows(w, bc, N, d, y[0], y[1], y[2]);
            }
            double *s = a.st + d * NTRS;
            s[S_N_FED] = s[S_N_FED] + 1.0; s[S_T_LAST] = t;
        }
    }
    const unsigned long long m = __ballot(live);
    const int up = seg > 0 ? (seg - 1) * n_zones : 0;     // first lane of the upstream's segment
    return stage != 0 && ((m >> up) & 1ull) != 0ull && a.lk[r] != 0;
}

// FEED with a pipe program: a link with a line gets the sample last delivered (slot head) again.  PIPE_FILL: every
// slot of every line holds the upstream's outlet from the state in memory with the time stamp NaN, head 0, and the
// pipe state starts over (every reactor's, linked or not); a FEED after it delivers that same sample.
// With a junction program the host runs JCT_BLEND before FEED and PIPE_FILL: every junction's blend from the state and
// the row 0 in memory goes to jct.tmp, so that no store of a carried flow precedes a read of that row.  FEED then
// writes a junction's rows (and a carrier's row 0) from tmp where Qs > 0 and leaves them where it is not; PIPE_FILL
// fills a junction's line with the blend, or with slot 0's outlet where Qs is 0.  RESTORE also writes a carrier's row 0.
enum { OP_FEED = 0, OP_RESTORE, OP_PIPE_FILL, OP_JCT_BLEND };
struct HostOpArgs { TrnArgs t; double *bc; const double *pH, *Cl, *T, *time; int64_t N; int n; int op; };
template <class E> __global__ __launch_bounds__(256) void host_op_kernel(const HostOpArgs a)
{
    const int64_t d = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (d >= a.N) return;
    const int w = a.t.lk[d];
    const uint32_t jw = (a.t.jct.on && w) ? a.t.jct.src[d] : 0u;
    const bool junction = (jw & JCT_ANY) != 0u;
    if (a.op == OP_JCT_BLEND) {
        if (!junction) return;
        const int64_t first = d - (int64_t)((uint32_t)d % (uint32_t)a.t.length);
        double q[PIPE_Q], Qs; bool all, any;
        blend(jw, a.t.jct.share, a.N, d, [&](int g, double v[5]) {
            const int64_t o = (first + g) * a.n + (a.n - 1);
            v[0] = a.pH[o]; v[1] = a.Cl[o]; v[2] = a.T[o]; v[3] = a.time[first + g]; v[4] = a.bc[first + g];
            return true; }, E(), q, Qs, all, any);
        double *c = a.t.jct.tmp + d;
        if (!(Qs > 0.0)) {                                // nothing flows: what PIPE_FILL takes is slot 0's outlet
            int g = 0;
            for (int k = JCT_SLOTS - 1; k >= 0; --k) if ((jw >> (JCT_BITS * k)) & JCT_USED) g = (int)((jw >> (JCT_BITS * k)) & 31u);
            const int64_t o = (first + g) * a.n + (a.n - 1);
            q[0] = a.pH[o]; q[1] = a.Cl[o]; q[2] = a.T[o];
        }
        c[0] = q[0]; c[a.N] = q[1]; c[2 * a.N] = q[2]; c[3 * a.N] = q[3]; c[4 * a.N] = Qs;
        return;
    }
    if (a.op == OP_PIPE_FILL) {
        const PipeArgs &p = a.t.pipe;
        p.st[d * NPS + PS_N_SENT] = 0.0; p.st[d * NPS + PS_T_SENT] = __builtin_nan("");
        p.head[d] = 0;
        const int D = w ? p.delay[d] : 0;
        if (D > 0) {
            const int64_t o = (d - 1) * a.n + (a.n - 1);
            const double *j = a.t.jct.tmp + d;
            const double s[PIPE_Q] = {junction ? j[0] : a.pH[o], junction ? j[a.N] : a.Cl[o], junction ? j[2 * a.N] : a.T[o],
                                      __builtin_nan("")};
            for (int slot = 0; slot <= D && slot < p.slots; ++slot) {
                double *c = ring_slot(p, slot, a.N, d);
#pragma unroll
                for (int q = 0; q < PIPE_Q; ++q) c[q * a.N] = s[q];
            }
        }
        return;
    }
    if (!w) return;                                       // (a first stage is never linked)
    if (a.op == OP_FEED) {
        const double *j = a.t.jct.tmp + d;
        if (junction && !(j[4 * a.N] > 0.0)) return;      // nothing flows: the rows stay
        if (junction && (jw & JCT_CARRY)) a.bc[d] = j[4 * a.N];
        const int D = a.t.pipe.on ? a.t.pipe.delay[d] : 0;
        if (D > 0) {
            const double *c = ring_slot(a.t.pipe, a.t.pipe.head[d], a.N, d);
            store_rows(w, a.bc, a.N, d, c[0], c[a.N], c[2 * a.N]);
            return;
        }
        if (junction) { store_rows(w, a.bc, a.N, d, j[0], j[a.N], j[2 * a.N]); return; }
        const int64_t o = (d - 1) * a.n + (a.n - 1);      // the upstream's outlet zone
        store_rows(w, a.bc, a.N, d, a.pH[o], a.Cl[o], a.T[o]);
    } else {
        store_rows(w, a.bc, a.N, d, a.t.base[d], a.t.base[a.N + d], a.t.base[2 * a.N + d]);
        if (jw & JCT_CARRY) a.bc[d] = a.t.jct.base0[d];
    }
}

} // namespace wtr
