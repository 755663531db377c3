// wt_svc.hpp -- gfx950 device code of the sensor service program (wt_ensemble_service_*, wt_ensemble_sensors_service):
// the maintenance half of the reference's sensor interface, which a host loop would call between two iterations:
//
//   BaseSensor.calibrate                          sensors/base_sensor.py:701-755
//   pHSensor.calibrate_two_point, clean_electrode sensors/ph_sensor.py:338-434
//   ChlorineSensor.replace_membrane, _reagent     sensors/chlorine_sensor.py:486-537
//
// All five are deterministic and draw nothing; every effect lands in a row wts::SState already has (DESIGN.md 7.22
// lists the reference fields that reach no reading and get no row).
//
//   apply        one action on one SState at suite time t with the fp32 reference value x
//   Program      the functor wts::suite_step calls for every active sensor lane after the read and before
//                store_state, behind the wave-uniform flag svc_on: the lane that owns sensor i of reactor r walks the
//                reactor's SLOTS slots in slot order, applies every due slot that targets sensor i and updates the
//                slot's state.  A slot names one sensor, so one lane alone writes a slot's state.  Lanes of one
//                wavefront take different actions in the same step: everything is a lane mask.
//   service_kernel  the immediate service of wt_ensemble_sensors_service, one thread per reactor, with the suite time
//                and the taps a fused read of a reactor that has just stepped used.
//
// A service changes the next read, never the current one.  Device layout (array of structures, indexed by reactor):
//   par [N][SLOTS][NSV] fp64    enable, sensor, action, trigger, t_first, period, count, status, delay, ref_mode, ref, ref2
//   st  [N][SLOTS][NSVS] fp64   n_done, t_last, t_due, t_seen
// The C ABI is SoA ([SLOTS][NSV][N], [SLOTS][NSVS][N]); the host transposes.  All trigger arithmetic is fp64 without
// fused multiply-adds (tests/service_ref.py restates it).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "wt_sensors.hpp"

namespace wtsv {

constexpr int SLOTS = 4, NSV = 12, NSVS = 4, NSH = 8;
enum { V_ENABLE = 0, V_SENSOR, V_ACTION, V_TRIGGER, V_T_FIRST, V_PERIOD, V_COUNT, V_STATUS, V_DELAY, V_REF_MODE, V_REF, V_REF2 };
enum { VS_N_DONE = 0, VS_T_LAST, VS_T_DUE, VS_T_SEEN };
enum { A_CALIBRATE = 0, A_TWO_POINT, A_RINSE, A_ACID_CLEAN, A_PEPSIN_CLEAN, A_REPLACE_MEMBRANE, A_REPLACE_REAGENT, N_ACTIONS };
enum { TR_AT_TIME = 0, TR_ON_STATUS, N_TRIGGERS };
enum { REF_CONSTANT = 0, REF_SAMPLE, REF_TRIM, N_REF_MODES };
enum { H_CAL_OFFSET = 0, H_CAL_TIME, H_POWER_ON, H_SLOW0, H_SLOW1, H_SLOW2, H_STATUS, H_FAULT };
constexpr int PAR_DOUBLES = SLOTS * NSV;      // 384 bytes per reactor
constexpr int ST_DOUBLES = SLOTS * NSVS;      // 128 bytes per reactor
constexpr double MIN_PERIOD = 1.0e-3;         // a shorter period (other than 0: once) is refused: t_due must pass t

// One maintenance call of the reference on sensor state s at suite time t; x is the reference value of the
// calibration the action ends in (unused by the cleaning actions).
__device__ __forceinline__ void apply(wts::SState &s, int action, double t, float x)
{
    // Every field gets a selected value, none a conditional store: stores under the action's branches end up as one
    // store through a selected address, which puts the whole SState into scratch memory.
    const bool clean = action >= A_RINSE && action <= A_PEPSIN_CLEAN;            // clean_electrode  ph_sensor.py:395-434
    const bool membrane = action == A_REPLACE_MEMBRANE, reagent = action == A_REPLACE_REAGENT;   // chlorine_sensor.py:503-509, :531-537
    const double keep = (action == A_RINSE) ? 0.5 : ((action == A_ACID_CLEAN) ? 0.1 : ((action == A_PEPSIN_CLEAN) ? 0.2 : 1.0));
    s.slow0 = membrane ? 0.0 : (reagent ? 1.0 : s.slow0 * keep);
    s.slow1 = (clean || membrane || reagent) ? 0.0 : s.slow1;
    s.slow2 = (action == A_TWO_POINT || reagent) ? 0.0 : s.slow2;                // calibrate_two_point  ph_sensor.py:389-393
    s.power_on = t;                                                              // cleaning and calibration both restart the warm-up
    s.cal_offset = clean ? s.cal_offset : x - s.current;                         // calibrate  base_sensor.py:727-741
    s.cal_time = clean ? s.cal_time : t;
    s.status = clean ? s.status : (int)wts::ST_NORMAL;
    s.fault = clean ? s.fault : (int)wts::FL_NONE;
}

// The reference value of an action: the two buffers' midpoint, the replacements' fixed 0.0, else by mode from the
// constant, the sensor's own tap (fp32) and the offset in force; rounded once to float32.
__device__ __forceinline__ float reference_value(int action, int mode, double ref, double ref2, float tap, float cal_offset)
{
#pragma clang fp contract(off)
    double x = ref;
    if (action == A_TWO_POINT) x = (ref + ref2) / 2.0;
    else if (action >= A_REPLACE_MEMBRANE) x = 0.0;
    else if (mode == REF_SAMPLE) x = (double)tap + ref;
    else if (mode == REF_TRIM) x = ((double)tap + (double)cal_offset) + ref;
    return (float)x;
}

// what store_state leaves out because a read never changes it
template <class A> __device__ __forceinline__ void store_serviced(const A &a, int i, int64_t r, const wts::SState &s)
{
    const int64_t N = a.N;
    a.fs[((int64_t)i * wts::NF + wts::F_CAL_OFFSET) * N + r] = s.cal_offset;
    double *D = a.ds + ((int64_t)i * wts::ND) * N + r;
    D[wts::D_CAL_TIME * N] = s.cal_time; D[wts::D_POWER_ON * N] = s.power_on;
}

struct Program {
    // a: SuiteArgs, read in place from the kernel arguments; sp, s: sensor i of reactor r after its read at suite time
    // t, which returned rstatus; tap: the reactor's column of StepIO::tap (stride RMAX)
    template <class A> __device__ __forceinline__ void operator()(const A &a, const wts::SensorSpec &sp, wts::SState &s, int i,
                                                                  const float *tap, int64_t r, double t, int rstatus) const
    {
#pragma clang fp contract(off)
        if (!__builtin_expect(a.svc_on != 0, 0)) return;
        bool serviced = false;
#pragma unroll 1
        for (int k = 0; k < SLOTS; ++k) {
            const double2 *p2 = reinterpret_cast<const double2 *>(a.svc_par + r * PAR_DOUBLES + k * NSV);   // 16-byte aligned
            const double2 h0 = p2[0];
            if (h0.x != 1.0 || (int)h0.y != i) continue;
            double *q = a.svc_st + r * ST_DOUBLES + k * NSVS;
            const double2 h1 = p2[1], h2 = p2[2], h3 = p2[3];       // action, trigger; t_first, period; count, status
            const double n_done = q[VS_N_DONE];
            if (h3.x > 0.0 && n_done >= h3.x) continue;             // the slot has had its services
            bool due;
            if ((int)h1.y == TR_AT_TIME) due = t >= q[VS_T_DUE];
            else {
                double seen = q[VS_T_SEEN];
                if (seen != seen && rstatus == (int)h3.y) { seen = t; q[VS_T_SEEN] = t; }    // the work order is written
                due = t - seen >= p2[4].x;                          // delay (NaN: unarmed, never due)
            }
            if (!due) continue;
            const double2 h4 = p2[4], h5 = p2[5];                   // delay, ref_mode; ref, ref2
            const int action = (int)h1.x;
            apply(s, action, t, reference_value(action, (int)h4.y, h5.x, h5.y, tap[sp.tap_self * wts::RMAX], s.cal_offset));
            serviced = true;
            q[VS_N_DONE] = n_done + 1.0;
            q[VS_T_LAST] = t;
            if ((int)h1.y == TR_AT_TIME) {
                double nd = __builtin_inf();                        // period 0: once
                if (h2.y > 0.0) {
                    const double d0 = q[VS_T_DUE];
                    nd = d0 + (floor((t - d0) / h2.y) + 1.0) * h2.y;
                    if (!(nd > t)) nd = nd + h2.y;
                }
                q[VS_T_DUE] = nd;
            } else q[VS_T_SEEN] = __builtin_nan("");
        }
        if (serviced) store_serviced(a, i, r, s);
    }
};

// wt_ensemble_sensors_service: one action on sensor `sensor` of every reactor the mask selects, now
struct ServiceArgs {
    wts::SuiteArgs s;
    const double *pH, *Cl, *T, *time, *flow;   // [N][n] state, [N]
    int n;
    int sensor, action, ref_mode;
    const double *ref, *ref2;                  // [N] or nullptr: 0
    const uint8_t *mask;                       // [N] or nullptr: all
};

__global__ __launch_bounds__(256) void service_kernel(const ServiceArgs a)
{
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= a.s.N) return;
    if (a.mask && !a.mask[r]) return;
    const wts::SensorSpec sp = wts::spec_of(a.sensor, a.s.full_scale[r]);
    // the taps of wt_step.hpp's sensor section: zone 0 and the last zone of the stored state, the flow of the last step
    const int ts = sp.tap_self;
    const int64_t z = r * a.n + ((ts & 1) && ts < 6 ? a.n - 1 : 0);
    const float tap = ts == 6 ? (float)a.flow[r] : (ts < 2 ? (float)a.pH[z] : (ts < 4 ? (float)a.Cl[z] : (float)a.T[z]));
    const double t = a.time[r] - a.s.t_enable[r];
    wts::SState s = wts::load_state(a.s, a.sensor, r);
    apply(s, a.action, t, reference_value(a.action, a.ref_mode, a.ref ? a.ref[r] : 0.0, a.ref2 ? a.ref2[r] : 0.0, tap, s.cal_offset));
    wts::store_state(a.s, a.sensor, r, s);
    store_serviced(a.s, a.sensor, r, s);
}

} // namespace wtsv
