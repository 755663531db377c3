// wt_wir.hpp -- gfx950 device code of the wire program (wt_ensemble_wire_*): the signal cables of a treatment train.
// On top of a set train program, input slot i (the seven sensors, suite order) of a reactor's controller-side copy of
// the readings may come from sensor s of stage g of the same train instead of the reactor's own instrument i.
//
//   route     runs at the head of a PLC scan in run_item, after the barrier that follows suite_step and before
//             everything else in the scan, so the injection program, pack_inputs, the PI loops, the IMAGE slots of
//             alarms and detectors and the trend recorder's image tags all see the wired value.  A train's stages sit
//             in consecutive reactor slots of one wavefront, starting at a multiple of `length`, in stage order, and
//             end every outer step together: when the scan starts every stage's readings are in the wavefront's LDS
//             (StepIO::val / fault, one column per slot).  The scan lane of slot `lane` holds stage
//             rix[lane] % length, so the source column is lane - stage + g.
//             Gather: the lane loads the source cells of its wired slots (the values wait in the lane's own column
//             of StepIO::tap, dead since suite_step; the fault codes in a register).  Barrier.  Scatter: it writes
//             them into its own column.  The barrier makes every lane's gather complete before any lane
//             overwrites its own column -- to the compiler a lane's store to its own cell and other lanes' loads of
//             it are unrelated accesses of one thread; only the barrier orders them.  So a source is always the
//             instrument's own output of this outer step (what suite_step left): wires do not chain, and a spoof in
//             the source stage's image does not travel.  No barrier follows the scatter: everything after it in the
//             scan reads the lane's own column only (&io.val[0][lane], &io.fault[0][lane]), and the scan's closing
//             reload of the reactor constants has its own barrier.
//             A source that did not take the outer step (io.stepped == 0: frozen, or T_RANGE_POST) has a stale
//             column: the slot reads NaN with fault FL_OPEN_CIRCUIT, a dead current loop.
//             FIELD slots, wt_ensemble_sensors_get and the sensor history read sens.out_value / out_fault and the
//             history arrays, which the sensor lanes wrote before: they stay the reactor's own instrument.
//
// Device layout (indexed by reactor: placement changes nothing):
//   src [N] uint64        slot i in bits 9 i .. 9 i + 8: WIRED (bit 8) | stage g (bits 3..7) | sensor s (bits 0..2);
//                         0: every slot on the reactor's own instrument
//   st  [N][NSENS][NWS]   fp64 n_routed (scans that delivered the source's reading), n_lost (scans that found the
//                         source stopped)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "wt_sensors.hpp"

namespace wtw {

constexpr int NW = 2, NWS = 2, SLOT_BITS = 9, WIRED = 1 << 8;
enum { W_STAGE = 0, W_SENSOR };
enum { WS_N_ROUTED = 0, WS_N_LOST };
constexpr int ST_DOUBLES = wts::NSENS * NWS;
static_assert(SLOT_BITS * wts::NSENS <= 64 && wts::RMAX <= 32 && wts::NSENS <= 8, "a reactor's seven slots fit one 64-bit word");

struct WirArgs {
    int on;                  // 0: no program (the scan's section reads this flag only)
    const uint64_t *src;     // [N]
    double *st;              // [N][NSENS][NWS]
};

__host__ __device__ constexpr uint64_t slot_word(int i, int stage, int sensor)
{
    return (uint64_t)(WIRED | (stage << 3) | sensor) << (SLOT_BITS * i);
}

// One scan's routing of a wavefront; every lane calls it, in wave-uniform control flow (it holds a barrier).  mine: this
// lane is the scan lane of a reactor that took the step (lane < R && io.stepped[lane]); length: stages per train.
// Between gather and scatter a value waits in the lane's own column of StepIO::tap: the sensor lanes are through with
// the taps of this outer step (the barrier behind suite_step), the next outer step writes them again, and no other
// lane touches this column meanwhile.  So nothing but the packed fault codes is held in registers across the barrier.
// The two slot loops stay rolled: unrolled, the allocator placed the solver loop's scalar spills differently and the
// kernel without any program measured 0.5 to 0.9 % slower.
template <class A>
__device__ __forceinline__ void route(const A &a, int length, bool mine, int lane, const int *rix, wts::StepIO &io)
{
    static_assert(wts::NTAP >= wts::NSENS, "a tap cell per input slot");
    uint32_t held = 0;                                    // slot i: fault code in bits 4 i .. 4 i + 2, lost in bit 4 i + 3
    uint64_t w = 0;
    if (mine) w = a.src[rix[lane]];
    if (w != 0) {                                         // gather
        const int first = lane - (int)((uint32_t)rix[lane] % (uint32_t)length);   // the slot of the train's stage 0
#pragma unroll 1
        for (int i = 0; i < wts::NSENS; ++i) {
            const uint32_t c = (uint32_t)(w >> (SLOT_BITS * i));
            if (c & WIRED) {
                const int src = (first + (int)((c >> 3) & 31u)) & (wts::RMAX - 1), s = (int)(c & 7u);
                const bool up = io.stepped[src] != 0;
                io.tap[i][lane] = up ? io.val[s][src] : __builtin_nanf("");
                held |= (up ? (uint32_t)(io.fault[s][src] & 7) : (uint32_t)(8 | wts::FL_OPEN_CIRCUIT)) << (4 * i);
            }
        }
    }
    __syncthreads();                                      // every gather before any scatter
    if (mine) w = a.src[rix[lane]];                       // (read again rather than held across the barrier)
    if (w != 0) {                                         // scatter, into this lane's own column
        double *st = a.st + (int64_t)rix[lane] * ST_DOUBLES;
#pragma unroll 1
        for (int i = 0; i < wts::NSENS; ++i) {
            if ((uint32_t)(w >> (SLOT_BITS * i)) & WIRED) {
                const uint32_t f = held >> (4 * i);
                io.val[i][lane] = io.tap[i][lane];
                io.fault[i][lane] = (int)(f & 7u);
                double *c = st + i * NWS + ((f >> 3) & 1u);
                *c = *c + 1.0;
            }
        }
    }
}

} // namespace wtw
