// wt_inj.hpp -- gfx950 device code of the per-reactor injection programs (wt_ensemble_inject_*): scripted sensor
// spoofing and command tampering on the cyber layer between the plant and its controller, at every PLC scan.  The
// reference lists a scripted fault-injection framework on its roadmap; its sensors only fail at random.
//
//   tamper_sensors   runs in the scan lane of a reactor that stepped, after read_all_sensors and before
//                    update_modbus_inputs (wt_plc.hpp pack_inputs): it rewrites the lane's copy of the readings in
//                    StepIO (LDS), so the input image and the PI programs (wt_ctl.hpp) see the tampered value.  The
//                    instrument's state, last reading and history are already stored (wts::emit) and stay as they are.
//   CommandTamper    the functor apply_commands runs on the three floats it decodes from the holding words, before
//                    validate_flow_rate: a man-in-the-middle that leaves the holding image as the master wrote it.
//
// Device layout (array of structures, indexed by reactor like wtc: placement changes nothing):
//   par [N][SLOTS][NI] fp64    mode, target, t_start, t_end, a, b     (48-byte slots: three 16-byte loads)
//   st  [N][SLOTS][NIS] fp64   n_applied, t_first, t_last, held
// The C ABI is SoA ([SLOTS][NI][N], [SLOTS][NIS][N]); the host transposes.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace wti {

constexpr int SLOTS = 4, NI = 6, NIS = 4;
enum { I_MODE = 0, I_TARGET, I_T_START, I_T_END, I_A, I_B };
enum { IS_N_APPLIED = 0, IS_T_FIRST, IS_T_LAST, IS_HELD };
enum { M_OFF = 0, M_BIAS, M_GAIN, M_CONSTANT, M_RAMP, M_FREEZE, M_DROPOUT, M_FAULT, N_MODES };
constexpr int CMD_ACID = 7, CMD_CHLORINE = 8, CMD_INLET = 9, N_TARGETS = 10;   // targets 0..6: the sensors
constexpr int PAR_DOUBLES = SLOTS * NI;     // 192 bytes per reactor
constexpr int ST_DOUBLES = SLOTS * NIS;     // 128 bytes per reactor

struct InjArgs {
    int on;                  // 0: no program (the scan section reads this flag only)
    const double *par;       // [N][PAR_DOUBLES]
    double *st;              // [N][ST_DOUBLES]
};

// a: InjArgs (read in place from the kernel arguments, hence the template).  Slot s of reactor r when it is active at t
// and its target is of the wanted kind: its six parameters in p.
template <class A> __device__ __forceinline__ bool slot_active(const A &a, int64_t r, int s, double t, bool command, double p[NI])
{
    const double2 *p2 = reinterpret_cast<const double2 *>(a.par + r * PAR_DOUBLES + s * NI);   // 16-byte aligned
    const double2 h0 = p2[0], h1 = p2[1];
    if (h0.x == (double)M_OFF || (h0.y >= (double)CMD_ACID) != command || !(h1.x <= t && t < h1.y)) return false;
    const double2 h2 = p2[2];
    p[I_MODE] = h0.x; p[I_TARGET] = h0.y; p[I_T_START] = h1.x; p[I_T_END] = h1.y; p[I_A] = h2.x; p[I_B] = h2.y;
    return true;
}

// One application of an active slot (parameters p, state q of reactor r) to the incoming float32 x at loop time t.
// Spelled out in the order of tests/inject_ref.py, nothing contracted into an fma, rounded once to float32.
__device__ __forceinline__ float apply_slot(const double p[NI], double *q, float x, double t, int &fault)
{
#pragma clang fp contract(off)
    const int mode = (int)p[I_MODE];
    const double xd = (double)x;
    const double n = q[IS_N_APPLIED];
    if (n == 0.0) {
        q[IS_T_FIRST] = t;
        if (mode == M_FREEZE) q[IS_HELD] = xd;
    }
    q[IS_N_APPLIED] = n + 1.0;
    q[IS_T_LAST] = t;
    double y = xd;
    switch (mode) {
        case M_BIAS:     y = xd + p[I_A]; break;
        case M_GAIN:     y = xd * p[I_A]; break;
        case M_CONSTANT: y = p[I_A]; break;
        case M_RAMP:     y = xd + (p[I_A] + p[I_B] * (t - p[I_T_START])); break;
        case M_FREEZE:   y = q[IS_HELD]; break;
        case M_DROPOUT:  y = __builtin_nan(""); break;
        case M_FAULT:    fault = (int)p[I_A]; break;
        default: break;
    }
    return (float)y;                          // round to nearest even
}

// value / fault: this scan's seven readings of reactor r (element i at [i * stride], LDS); t: the loop time the
// scan stores.  The slots stay rolled: one slot's record is live at a time.
template <class A> __device__ __forceinline__ void tamper_sensors(const A &a, int64_t r, float *value, int *fault, int stride, double t)
{
#pragma unroll 1
    for (int s = 0; s < SLOTS; ++s) {
        double p[NI];
        if (!slot_active(a, r, s, t, false, p)) continue;
        const int i = (int)p[I_TARGET] * stride;
        int f = fault[i];
        value[i] = apply_slot(p, a.st + r * ST_DOUBLES + s * NIS, value[i], t, f);
        fault[i] = f;
    }
}

// apply_commands' tamper hook (wt_plc.hpp) for reactor r at loop time t
template <class A> struct CommandTamper {
    const A &a;
    int64_t r;
    double t;
    __device__ __forceinline__ void operator()(float &acid, float &chlorine, float &inlet) const
    {
#pragma unroll 1
        for (int s = 0; s < SLOTS; ++s) {
            double p[NI];
            if (!slot_active(a, r, s, t, true, p)) continue;
            const int tg = (int)p[I_TARGET];
            const float x = tg == CMD_ACID ? acid : (tg == CMD_CHLORINE ? chlorine : inlet);
            int unused = 0;
            const float y = apply_slot(p, a.st + r * ST_DOUBLES + s * NIS, x, t, unused);
            if (tg == CMD_ACID) acid = y;
            else if (tg == CMD_CHLORINE) chlorine = y;
            else inlet = y;
        }
    }
};
template <class A> __device__ __forceinline__ CommandTamper<A> command_tamper(const A &a, int64_t r, double t) { return {a, r, t}; }

} // namespace wti
