// wt_lnk.hpp -- gfx950 device code of the per-reactor link programs (wt_ensemble_link_*): what the fieldbus between the
// plant and its controller does to a signal in time.  A slot sits on one channel of the plant's I/O, keeps a ring of the
// channel's last DEPTH samples, and decides at every PLC scan what the receiving end gets: the sample of some scans ago
// (a delay attack, or a slow network), the last value that came through (lost polls, a denial of service, with a
// timeout after which a reading goes dead and a command falls back to its fail-safe), or a taped stretch of the
// channel's own past played in a loop (a replay attack, which carries the tape's noise and passes a flat-line check).
// The reference has no link model at all: its loop hands the readings to the registers in the same breath.
//
//   link_sensors     runs in the scan lane of a reactor that stepped, after the wire program and directly BEFORE
//                    wti::tamper_sensors: it rewrites the lane's copy of the readings in StepIO (LDS), so the image, the
//                    controllers, IMAGE slots and the trend tags see the linked value; the instrument's own reading
//                    (sensor_readings(), FIELD slots) stays as it is.
//   LinkThenTamper   the functor apply_commands runs on the three floats it decodes from the holding words: the link's
//                    command slots, then (where an injection program is on) wti::CommandTamper.  The holding image is
//                    not touched.
//
// One scan of one slot on the sample (x, f) of its channel (f = 0 for a command), t the loop time the scan stores, in
// slot order (two slots on one channel chain); every count is an fp64 whole number:
//   1. record: ring[n_rec % DEPTH] = (x, f), n_rec += 1 -- except a REPLAY slot inside its window: the tape must survive.
//   2. outside the window (mode OFF, or not start <= t < end): (x, f) passes; held = (x, f), t_fresh = t, tape_end = NaN.
//   3. inside: j = n_applied, n_applied += 1, then
//        DELAY   d = a, or a + floor(u * (b + 1)) where b != 0; delivers ring[max(n_rec - 1 - d, 0) % DEPTH]; fresh.
//        LOSS    one draw u; u >= a: (x, f) fresh.  u < a: n_lost += 1; if t_fresh is NaN (nothing was ever delivered) the
//                sample passes, fresh; else held is delivered, or, if t - t_fresh > timeout, the fail state with
//                n_timeout += 1: a reading NaN with fault code `fail`, a command the value float32(fail).
//        REPLAY  if tape_end is NaN (the window's first scan): if n_rec == 0 record this sample, then tape_end = n_rec.
//                L = min(a, tape_end), at least 1; delivers ring[(tape_end - L + j % L) % DEPTH]; fresh.
//      a fresh delivery (y, g): held = (y, g), t_fresh = t, n_fresh += 1.
//   u = word 0 of philox4x32_10(reactor_base + r, slot, n_draw, 2, seed) * 2^-32, n_draw += 1 per draw.
// Every ring index goes through whole() and & (DEPTH - 1): no state row, restored or edited, addresses outside the ring.
//
// Device layout (array of structures, indexed by reactor like wti: placement changes nothing), 2880 bytes per reactor:
//   par   [N][SLOTS][NL]  fp64   mode, target, start, end, a, b, timeout, fail            (64-byte slots)   256 B
//   st    [N][SLOTS][NLS] fp64   n_rec, n_applied, n_fresh, n_lost, n_timeout, n_draw, t_fresh, held_value,
//                                held_fault, tape_end                                                       320 B
//   ring  [N][SLOTS][DEPTH] fp64   the samples' values: the channel's float32 widened, which is exact      2048 B
//   fring [N][SLOTS][DEPTH] uint8  their fault codes (0..6)                                                 256 B
// The C ABI is SoA ([SLOTS][NL][N], [SLOTS][NLS][N], [SLOTS][DEPTH][N]); the host transposes.  The arrays live in the
// plant I/O array group: they come and go with plant I/O, and the switch and the seed are scalars of it.  Only the scan
// lane of a reactor touches that reactor's records and rings, and a work item's hand-off orders the items' accesses, as
// it does for the pipe rings.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "wt_sensors.hpp"
#include "wt_inj.hpp"

namespace wtl {

constexpr int SLOTS = 4, DEPTH = 64, NL = 8, NLS = 10;
enum { L_MODE = 0, L_TARGET, L_START, L_END, L_A, L_B, L_TIMEOUT, L_FAIL };
enum { LS_N_REC = 0, LS_N_APPLIED, LS_N_FRESH, LS_N_LOST, LS_N_TIMEOUT, LS_N_DRAW, LS_T_FRESH, LS_HELD_VALUE, LS_HELD_FAULT,
       LS_TAPE_END };
enum { M_OFF = 0, M_DELAY, M_LOSS, M_REPLAY, N_MODES };
constexpr int CMD_ACID = wti::CMD_ACID, CMD_CHLORINE = wti::CMD_CHLORINE, N_TARGETS = wti::N_TARGETS;   // the injection program's codes
constexpr int PAR_DOUBLES = SLOTS * NL;      // 256 bytes per reactor
constexpr int ST_DOUBLES = SLOTS * NLS;      // 320 bytes per reactor
constexpr int RING_ENTRIES = SLOTS * DEPTH;  // 2048 + 256 bytes per reactor
constexpr uint32_t DRAW_STREAM = 2u;         // Philox counter word 3: 0 the sensors, 1 the disturbances
static_assert((DEPTH & (DEPTH - 1)) == 0, "ring indices are reduced with & (DEPTH - 1)");

struct LnkArgs {
    int on;                  // 0: no program (the scan section reads this flag only)
    uint32_t seed_lo, seed_hi;
    const double *par;       // [N][PAR_DOUBLES]
    double *st;              // [N][ST_DOUBLES]
    double *ring;            // [N][RING_ENTRIES]
    uint8_t *fring;          // [N][RING_ENTRIES]
};

// a count as an index: whole numbers below 2^32 as they are, anything else (NaN, negative, huge) 0
__device__ __forceinline__ uint32_t whole(double c) { return (c >= 0.0 && c < 4294967296.0) ? (uint32_t)c : 0u; }

// One scan of slot s of reactor r (parameters p, read where they are needed) on the incoming sample (x, f): returns
// the delivered value and leaves the delivered fault code in f.  Spelled out in the order of tests/link_ref.py.
template <class A>
__device__ __forceinline__ float link_slot(const A &a, int64_t r, int s, const double *p, uint32_t reactor, float x, int &f, double t,
                                           bool command)
{
#pragma clang fp contract(off)
    double *q = a.st + r * ST_DOUBLES + s * NLS;
    double *ring = a.ring + (r * SLOTS + s) * DEPTH;
    uint8_t *fring = a.fring + (r * SLOTS + s) * DEPTH;
    const double mode = p[L_MODE];
    const bool inside = mode != (double)M_OFF && p[L_START] <= t && t < p[L_END];
    const double xd = (double)x;
    double n_rec = q[LS_N_REC];
    // 1. record
    if (!(inside && mode == (double)M_REPLAY)) {
        const uint32_t i = whole(n_rec) & (DEPTH - 1);
        ring[i] = xd; fring[i] = (uint8_t)f;
        n_rec = n_rec + 1.0;
        q[LS_N_REC] = n_rec;
    }
    // 2. outside the window
    if (!inside) {
        q[LS_HELD_VALUE] = xd; q[LS_HELD_FAULT] = (double)f; q[LS_T_FRESH] = t;
        // the tape is forgotten where there is one: an unconditional store joins the three above as a 32-byte pair of
        // stores whose constant half the compiler keeps in four registers for the whole kernel (counted as VGPR spills)
        if (q[LS_TAPE_END] == q[LS_TAPE_END]) q[LS_TAPE_END] = __builtin_nan("");
        return x;
    }
    // 3. inside
    const double j = q[LS_N_APPLIED];
    q[LS_N_APPLIED] = j + 1.0;
    double y = xd;
    int g = f;
    bool fresh = true;
    double u = 0.0;
    if (mode == (double)M_LOSS || (mode == (double)M_DELAY && p[L_B] != 0.0)) {
        const double nd = q[LS_N_DRAW];
        uint32_t w[4];
        wts::philox4x32_10(reactor, (uint32_t)s, whole(nd), DRAW_STREAM, a.seed_lo, a.seed_hi, w);
        u = (double)w[0] * (1.0 / 4294967296.0);
        q[LS_N_DRAW] = nd + 1.0;
    }
    if (mode == (double)M_DELAY) {
        const double b = p[L_B];
        double d = p[L_A];
        if (b != 0.0) d = d + floor(u * (b + 1.0));
        const uint32_t i = whole(fmax(n_rec - 1.0 - d, 0.0)) & (DEPTH - 1);
        y = ring[i]; g = (int)fring[i];
    } else if (mode == (double)M_LOSS) {
        if (u < p[L_A]) {
            q[LS_N_LOST] = q[LS_N_LOST] + 1.0;
            const double tf = q[LS_T_FRESH];
            if (tf == tf) {
                fresh = false;
                if (t - tf > p[L_TIMEOUT]) {
                    q[LS_N_TIMEOUT] = q[LS_N_TIMEOUT] + 1.0;
                    if (command) { y = (double)(float)p[L_FAIL]; g = 0; }
                    else { y = __builtin_nan(""); g = (int)p[L_FAIL]; }
                } else {
                    y = q[LS_HELD_VALUE]; g = (int)whole(q[LS_HELD_FAULT]);
                }
            }
        }
    } else {
        double te = q[LS_TAPE_END];
        if (te != te) {
            if (n_rec == 0.0) {
                ring[0] = xd; fring[0] = (uint8_t)f;
                n_rec = 1.0;
                q[LS_N_REC] = n_rec;
            }
            te = n_rec;
            q[LS_TAPE_END] = te;
        }
        uint32_t len = whole(fmin(p[L_A], te));
        if (len < 1u) len = 1u;
        const uint32_t i = (whole(te) - len + whole(j) % len) & (DEPTH - 1);
        y = ring[i]; g = (int)fring[i];
    }
    if (fresh) {
        q[LS_HELD_VALUE] = y; q[LS_HELD_FAULT] = (double)g; q[LS_T_FRESH] = t;
        q[LS_N_FRESH] = q[LS_N_FRESH] + 1.0;
    }
    f = g;
    return (float)y;                          // a float32 widened and narrowed again: exact
}

// value / fault: this scan's seven readings of reactor r (element i at [i * stride], LDS); t: the loop time the scan
// stores; reactor_base: the sensor suite's.  The slots stay rolled: one slot's record is live at a time.
template <class A>
__device__ __forceinline__ void link_sensors(const A &a, int64_t reactor_base, int64_t r, float *value, int *fault, int stride, double t)
{
#pragma unroll 1
    for (int s = 0; s < SLOTS; ++s) {
        const double *p = a.par + r * PAR_DOUBLES + s * NL;
        const double target = p[L_TARGET];
        if (!(target < (double)CMD_ACID)) continue;
        const int i = (int)(whole(target) % (uint32_t)CMD_ACID) * stride;
        int f = fault[i];
        value[i] = link_slot(a, r, s, p, (uint32_t)(reactor_base + r), value[i], f, t, false);
        fault[i] = f;
    }
}

// apply_commands' tamper hook (wt_plc.hpp) for reactor r at loop time t: the link's command slots, then the injection
// program's where one is on
template <class A, class I> struct LinkThenTamper {
    const A &a;
    const I &inj;
    bool tamper;
    int64_t reactor_base, r;
    double t;
    __device__ __forceinline__ void operator()(float &acid, float &chlorine, float &inlet) const
    {
#pragma unroll 1
        for (int s = 0; s < SLOTS; ++s) {
            const double *p = a.par + r * PAR_DOUBLES + s * NL;
            const double target = p[L_TARGET];
            if (!(target >= (double)CMD_ACID)) continue;
            const int tg = (int)whole(target);
            const float x = tg == CMD_ACID ? acid : (tg == CMD_CHLORINE ? chlorine : inlet);
            int unused = 0;
            const float y = link_slot(a, r, s, p, (uint32_t)(reactor_base + r), x, unused, t, true);
            if (tg == CMD_ACID) acid = y;
            else if (tg == CMD_CHLORINE) chlorine = y;
            else inlet = y;
        }
        if (tamper) wti::command_tamper(inj, r, t)(acid, chlorine, inlet);
    }
};
template <class A, class I>
__device__ __forceinline__ LinkThenTamper<A, I> link_then_tamper(const A &a, const I &inj, bool tamper, int64_t reactor_base, int64_t r, double t)
{
    return {a, inj, tamper, reactor_base, r, t};
}

} // namespace wtl
