// wt_ins.hpp -- the per-reactor installation record of the fused sensor suite (wt_ensemble_install_*): the sample
// lines and the InstallationQuality that create_realistic_sensor_suite (sensors/__init__.py:41-120) builds once for
// every reactor, as data.
//
//   SampleLine.__post_init__                 sensors/base_sensor.py:165-175   (the line's delay; the library derives it)
//   InstallationQuality                      sensors/base_sensor.py:125-145
//   BaseSensor._apply_installation_effects   sensors/base_sensor.py:464-507
//
// One record per reactor, array of structures, 16-byte aligned.  The first LANE_DOUBLES doubles are what a sensor lane
// reads, in four 16-byte loads: the two delays, the bubble probability per read (frequency / 60, the reference's
// quotient in fp64), the decision flags -- taken by the host on the doubles as given, so a value on a threshold falls
// where the reference puts it --, the three values the signal path uses in fp32, and one spare.  The parameters as
// the set call took them follow (what wt_ensemble_install_get returns).  The reads themselves are in wt_sensors.hpp.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace wtin {

constexpr int NINS = 9;
enum { P_LINE_VOLUME_INLET = 0, P_LINE_FLOW_INLET, P_LINE_VOLUME_OUTLET, P_LINE_FLOW_OUTLET, P_FLOW_VELOCITY,
       P_AIR_BUBBLE_FREQUENCY, P_GROUNDING_QUALITY, P_PIPE_VIBRATION_G, P_AMBIENT_TEMPERATURE };
enum { R_DELAY_INLET = 0, R_DELAY_OUTLET, R_BUBBLE_P, R_FLAGS, R_GROUND_SCALE, R_VIBRATION, R_AMBIENT, R_SPARE, LANE_DOUBLES,
       R_PARAMS = LANE_DOUBLES };
constexpr int REC_DOUBLES = 18;               // 144 bytes per reactor: 8 for the lanes, the 9 parameters, 1 of padding
static_assert(R_PARAMS + NINS <= REC_DOUBLES && REC_DOUBLES % 2 == 0 && LANE_DOUBLES % 2 == 0, "the record is read in 16-byte pairs");
enum { F_STAGNANT = 1, F_BUBBLES = 2, F_GROUND = 4, F_VIBRATION = 8 };

// the suite's own build (sensors/__init__.py:53-67): what a handle without an installation computes with
constexpr double DEFAULT_DELAY = 30.0;        // (250 / 1000) / (500 / 1000 / 60)
constexpr float DEFAULT_AMBIENT = 30.0f;

// The kernel's arguments: the records are the sensor suite's arrays, allocated with it.  They stand at the end of the
// argument block, so that no other section's arguments move.
struct InsArgs {
    const double *par;    // [N][REC_DOUBLES]
    int on;               // 0: the suite's own build for every reactor
};

// What a sensor lane holds of its reactor's record.  The defaults are the suite's build: no flag, so no branch of the
// installation effects is taken and nothing is drawn.
struct Lane {
    double delay_inlet = DEFAULT_DELAY, delay_outlet = DEFAULT_DELAY;
    double bubble_p = 0.0;
    int flags = 0;
    float ground_scale = 0.0f, vibration = 0.0f, ambient = DEFAULT_AMBIENT;
};

__device__ __forceinline__ Lane load_lane(const double *inst_par, int64_t r)
{
    const double2 *p = reinterpret_cast<const double2 *>(inst_par + r * REC_DOUBLES);   // 16-byte aligned
    const double2 a = p[0], b = p[1], c = p[2], d = p[3];
    Lane l;
    l.delay_inlet = a.x; l.delay_outlet = a.y; l.bubble_p = b.x; l.flags = (int)b.y;
    l.ground_scale = (float)c.x; l.vibration = (float)c.y; l.ambient = (float)d.x;
    return l;
}

} // namespace wtin
