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

struct TrnArgs {
    int on;                  // 0: no program (the step kernel's section reads this flag only)
    int length;              // stages per train
    const int32_t *lk;       // [N]
    double *st;              // [N][NTRS]
    double *base;            // [FED_ROWS][N]
    PipeArgs pipe;           // the pipe program on top (pipe.on == 0: none)
};

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

// One outer step's feeds of a wavefront; every lane calls it.  live: this lane's reactor r stepped and its state
// stands (the sensor section's test); outlet: this lane holds zone n - 1; y: the lane's state after the step; t: the
// reactor's time after it.  Returns whether this lane's reactor was fed (its lanes then reload the reactor constants).
template <class A>
__device__ __forceinline__ bool feed(const A &a, bool live, bool outlet, int seg, int n_zones, int64_t r, double t,
                                     const double y[3], double *bc, int64_t N)
{
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
enum { OP_FEED = 0, OP_RESTORE, OP_PIPE_FILL };
struct HostOpArgs { TrnArgs t; double *bc; const double *pH, *Cl, *T; int64_t N; int n; int op; };
__global__ __launch_bounds__(256) void host_op_kernel(const HostOpArgs a)
{
    const int64_t d = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (d >= a.N) return;
    const int w = a.t.lk[d];
    if (a.op == OP_PIPE_FILL) {
        const PipeArgs &p = a.t.pipe;
        p.st[d * NPS + PS_N_SENT] = 0.0; p.st[d * NPS + PS_T_SENT] = __builtin_nan("");
        p.head[d] = 0;
        const int D = w ? p.delay[d] : 0;
        if (D > 0) {
            const int64_t o = (d - 1) * a.n + (a.n - 1);
            const double s[PIPE_Q] = {a.pH[o], a.Cl[o], a.T[o], __builtin_nan("")};
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
        const int D = a.t.pipe.on ? a.t.pipe.delay[d] : 0;
        if (D > 0) {
            const double *c = ring_slot(a.t.pipe, a.t.pipe.head[d], a.N, d);
            store_rows(w, a.bc, a.N, d, c[0], c[a.N], c[2 * a.N]);
            return;
        }
        const int64_t o = (d - 1) * a.n + (a.n - 1);      // the upstream's outlet zone
        store_rows(w, a.bc, a.N, d, a.pH[o], a.Cl[o], a.T[o]);
    } else {
        store_rows(w, a.bc, a.N, d, a.t.base[d], a.t.base[a.N + d], a.t.base[2 * a.N + d]);
    }
}

} // namespace wtr
