// wt_mpc.hpp -- gfx950 device code of the per-reactor model predictive controllers (wt_ensemble_mpc_*): dynamic matrix
// control (DMC) on a per-reactor step-response model, one controller per dosing loop.  The reference's roadmap lists an
// "MPC controller module"; it has none.  Where a PI loop can only be detuned until it survives the dead time of sample
// lines, pipes and wires, a DMC controller carries the dead time in its model: it keeps a prediction of the next 64
// controller periods of the reading, corrects it by the difference between reading and prediction (the bias feedback),
// and moves the output by the dot product of a precomputed gain row with the predicted error.
//
//   mpc_execute   runs at a PLC scan, immediately AFTER tune_execute (wt_tun.hpp) and BEFORE pi_execute (wt_ctl.hpp),
//                 with their inputs: the scan's (possibly tampered) readings and the loop time the scan stores.  Every
//                 lane of the wavefront calls it, in wave-uniform control flow.  It writes the holding words as the PI
//                 does -- loop 0 chlorine (words 2-3), loop 1 acid (words 0-1) -- so its commands act from the next scan
//                 on.  It returns, in the scan lanes, the mask of the loops it owned in this scan; pi_execute skips those.
//
// The controller runs on the wavefront, not on a lane.  A scan lane (one per reactor that stepped) does the scalar part
// of its reactor from the array-of-structures record -- enable, t_start, ownership, the period counter, the validity of
// the reading -- and leaves a code: nothing to do, shift the prediction, execute, or start and execute.  A wave-uniform loop then walks the
// lanes that left a code, and for each of them all 64 lanes take element `lane` of that reactor's prediction, step
// response and gain rows (512 contiguous bytes each): the shift is a load at lane + 1, the dot product a butterfly of six
// exchange-and-add steps, the clamps are computed in every lane, and the new prediction is one coalesced store.  The
// scan lane then stores the scalars and the holding words.  No per-lane array, no LDS, no private segment.
//
// Device layout:
//   par  [N][LOOPS][NM]  fp64  enable, sensor, setpoint, every, horizon, u0, out_min, out_max, du_max, t_start
//   st   [N][LOOPS][NMS] fp64  phase (0 waiting, 1 running), output, count, bias, move, t_exec, ise, iae, dose, n_exec,
//                              n_held, n_sat, n_rate, n_skipped
//   step, gain, pred [N][LOOPS][H] fp64
// The C ABI is SoA ([LOOPS][NM][N], [LOOPS][NMS][N], [LOOPS][H][N]) like the control blocks; the host transposes.  The
// arrays live in the plant I/O array group: they come and go with plant I/O, and the switch is one of its scalars.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "wt_plc.hpp"
#include "wt_ctl.hpp"

namespace wtm {

constexpr int LOOPS = wtc::LOOPS, NM = 10, NMS = 14, H = 64;
enum { M_ENABLE = 0, M_SENSOR, M_SETPOINT, M_EVERY, M_HORIZON, M_U0, M_OUT_MIN, M_OUT_MAX, M_DU_MAX, M_T_START };
enum { MS_PHASE = 0, MS_OUTPUT, MS_COUNT, MS_BIAS, MS_MOVE, MS_T_EXEC, MS_ISE, MS_IAE, MS_DOSE, MS_N_EXEC, MS_N_HELD,
       MS_N_SAT, MS_N_RATE, MS_N_SKIPPED };
enum { PH_WAITING = 0, PH_RUNNING = 1 };
enum { DO_NOTHING = 0, DO_SHIFT = 1, DO_EXECUTE = 2, DO_START = 3 };    // what a scan lane asks the wavefront for
constexpr int PAR_DOUBLES = LOOPS * NM;             // 160 bytes per reactor
constexpr int ST_DOUBLES = LOOPS * NMS;             // 224 bytes per reactor
constexpr int ROW_DOUBLES = LOOPS * H;              // 1 KiB per reactor: a loop's row is 512 contiguous bytes
static_assert(H == 64, "a row is one wavefront wide: lane i holds element i");
static_assert(NM % 2 == 0, "the parameter records are read in 16-byte pairs");
static_assert(M_SENSOR == M_ENABLE + 1 && M_EVERY == M_SETPOINT + 1 && M_T_START == M_DU_MAX + 1 && M_ENABLE % 2 == 0,
              "the parameter pairs the scan lane reads");

struct MpcArgs {
    int on;                  // 0: no controller (the scan section reads this flag only)
    const double *par;       // [N][PAR_DOUBLES]
    double *st;              // [N][ST_DOUBLES]
    const double *step;      // [N][ROW_DOUBLES]
    const double *gain;      // [N][ROW_DOUBLES]
    double *pred;            // [N][ROW_DOUBLES]
};

// The balanced-tree sum of the 64 lanes' x, in every lane: for half = 32 ... 1 element i takes x[i] + x[i + half].  The
// butterfly pairs the same elements (lane i with lane i ^ half) and an add is commutative, so every lane ends with the
// bits of the tree's root.
__device__ __forceinline__ double tree_sum(double x)
{
#pragma clang fp contract(off)
#pragma unroll 1                                            // rolled: the block is cold, and every kernel is larger than the instruction cache
    for (int half = H / 2; half >= 1; half >>= 1) x = x + __shfl_xor(x, half, 64);
    return x;
}

// a: MpcArgs, c: the PI program's CtlArgs (the holding image), both read in place from the kernel arguments.  mine: this
// lane is the scan lane of a reactor that took the step (lane < R && io.stepped[lane]); rix: reactor of each scan lane
// (LDS); value / fault: this scan's readings, sensor i of scan lane j at [i * stride + j] (LDS); loop_time: the loop
// times the scan has stored; tuned: in a scan lane, the loops the tune program owned in this scan.  Every operation
// below is spelled out in the order of tests/mpc_ref.py and nothing is contracted into an fma, so the host restatement
// gives the same bits.
//
// Within a scan a record field is written by one party only: count, n_held and n_skipped by the scan lane's scalar part,
// everything else after the wavefront's part, by the same lane -- and the wavefront's part reads none of the three.
template <class A, class C>
__device__ __forceinline__ int mpc_execute(const A &a, const C &c, bool mine, int lane, const int *rix, const float *value, const int *fault,
                                           int stride, const double *loop_time, int tuned)
{
#pragma clang fp contract(off)
    int owned = 0;
#pragma unroll 1
    for (int l = 0; l < LOOPS; ++l) {
        // ---- the scalar part, in the scan lanes
        int code = DO_NOTHING;
        float v = 0.0f;
        if (mine) {
            const int64_t r = rix[lane];
            const double2 *p2 = reinterpret_cast<const double2 *>(a.par + r * PAR_DOUBLES + l * NM);
            double *q = a.st + r * ST_DOUBLES + l * NMS;
            const double2 es = p2[M_ENABLE / 2];                    // enable, sensor
            if (es.x != 0.0 && loop_time[r] >= p2[M_DU_MAX / 2].y) {
                if ((tuned >> l) & 1) {
                    q[MS_N_SKIPPED] = q[MS_N_SKIPPED] + 1.0;        // the relay experiment has the loop in this scan
                } else {
                    owned |= 1 << l;
                    const double phase = q[MS_PHASE], count = q[MS_COUNT];
                    bool running = phase == (double)PH_RUNNING;
                    if (count == 0.0) {                             // due
                        const int si = (int)es.y;
                        v = value[si * stride + lane];
                        if (!isfinite(v) || fault[si * stride + lane] != 0) {
                            q[MS_N_HELD] = q[MS_N_HELD] + 1.0;      // hold: no move, no word; a running loop's horizon moves on
                            if (running) code = DO_SHIFT;
                        } else {
                            code = running ? DO_EXECUTE : DO_START;
                            running = true;
                        }
                    }
                    if (running) {                                  // (count + 1) mod every
                        const double next = count + 1.0;
                        q[MS_COUNT] = next >= p2[M_SETPOINT / 2].y ? 0.0 : next;
                    }
                }
            }
        }
        // ---- the wavefront's part: one reactor at a time, element `lane` of its rows
        unsigned long long todo = __ballot(code != DO_NOTHING);
        while (todo) {
            const int j = (int)__builtin_ctzll(todo);
            todo &= todo - 1;
            const int cj = __builtin_amdgcn_readlane(code, j);      // j is wave-uniform: the code and the reading come as scalars
            const int64_t r = rix[j];
            const int64_t row = (r * LOOPS + l) * H;
            double *pred = a.pred + row;
            const int up = lane < H - 1 ? lane + 1 : H - 1;
            if (cj == DO_SHIFT) {
                const double s = pred[up];
                pred[lane] = s;
                continue;
            }
            const double vd = (double)__int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), j));
            const double *p = a.par + r * PAR_DOUBLES + l * NM;
            double *q = a.st + r * ST_DOUBLES + l * NMS;
            const double lo = p[M_OUT_MIN], hi = p[M_OUT_MAX];
            double s = vd, first = vd, output;
            if (cj == DO_START) {                                   // the prediction starts flat at the reading
                output = fmin(fmax(p[M_U0], lo), hi);
            } else {
                s = pred[up]; first = pred[0];
                output = q[MS_OUTPUT];
            }
            const double d = vd - first;
            const double sp = p[M_SETPOINT];
            const int horizon = (int)p[M_HORIZON];
            double term = 0.0;
            if (lane < horizon) term = a.gain[row + lane] * ((sp - s) - d);
            const double du = tree_sum(term);
            const double dm = p[M_DU_MAX];
            const double dc = fmin(fmax(du, -dm), dm);
            const double u = output + dc;
            const double y = fmin(fmax(u, lo), hi);
            const double move = y - output;                         // the move as applied: the anti-windup
            pred[lane] = s + a.step[row + lane] * move;
            if (lane == j) {                                        // the scan lane: scalars, holding words, metrics
                const double t = loop_time[r];
                const double e = sp - vd;
                const double h = cj == DO_START ? 0.0 : t - q[MS_T_EXEC];
                q[MS_PHASE] = (double)PH_RUNNING; q[MS_OUTPUT] = y;
                q[MS_BIAS] = d; q[MS_MOVE] = move; q[MS_T_EXEC] = t;
                if (dc != du) q[MS_N_RATE] = q[MS_N_RATE] + 1.0;
                if (y != u) q[MS_N_SAT] = q[MS_N_SAT] + 1.0;
                const uint32_t b = wtp::f32_bits_from_double(y);
                uint16_t *w = c.hr + r * wtp::HR_WORDS + wtc::loop_word(l);
                w[0] = (uint16_t)(b >> 16); w[1] = (uint16_t)(b & 0xffffu);
                q[MS_ISE] = q[MS_ISE] + (e * e) * h;
                q[MS_IAE] = q[MS_IAE] + fabs(e) * h;
                q[MS_DOSE] = q[MS_DOSE] + y * h;
                q[MS_N_EXEC] = q[MS_N_EXEC] + 1.0;
            }
        }
    }
    return owned;
}

} // namespace wtm
