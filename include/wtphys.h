/*
 * wtphys.h -- C ABI of libwtphys.so: the MI355X (gfx950) implementation of the
 * multi-zone CSTR physics step of wt_simulator.core, batched over an ensemble
 * of independent reactors.
 *
 * The reference has no FFI: its boundary for this path is the Python class
 * API  IntegratedCSTR(config).step(dt, boundary) -> ReactorState
 * (/root/reference/src/wt_simulator/core/reactor.py:203, :450-509).  Each entry
 * point below names the reference interface it stands in for.  All functions
 * return 0 on success or a WT_E_* code; wt_last_error() gives the text.  No
 * exception or torch type crosses this boundary; pointers are plain host (or,
 * where stated, device) pointers.
 *
 * Data layout (all fp64):
 *   state   pH, Cl, T : [N][n]   reactor-major, zone fastest  (= numpy (N, n))
 *   par     [WT_NP][N]           per-reactor constants, SoA   (see WT_P_*)
 *   bc      [WT_NB][N]           BoundaryConditions columns, SoA (see WT_B_*)
 * One handle = one device, one HIP stream, one caller thread (not re-entrant).
 */
#ifndef WTPHYS_H
#define WTPHYS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define WT_ABI_VERSION 1
#define WT_MAX_ZONES 64 /* one reactor's zones live in one 64-lane wavefront */
#define WT_MAX_STREAMS 8
#define WT_DEFAULT_CHUNK 50   /* outer steps per launch unless wt_ensemble_set_schedule says otherwise */

/* rows of the per-reactor constant block (values as the reference's __init__
 * computes them: reactor.py:229-270, chemistry.py:116-132, transport.py:202-290) */
enum {
    WT_P_VOLUME = 0, WT_P_HEIGHT = 1, WT_P_DIAMETER = 2,
    WT_P_KW = 3, WT_P_KA1 = 4, WT_P_KA2 = 5, WT_P_KA_HOCL = 6, WT_P_CT_MOL = 7,
    WT_P_KEX = 8, WT_P_USUP = 9, WT_P_STRAT = 10, WT_P_RI_CRIT = 11, WT_P_SUPP = 12,
    WT_NP = 16
};

/* rows of the boundary block = BoundaryConditions fields, reactor.py:169-186 */
enum {
    WT_B_Q_IN = 0, WT_B_PH_IN = 1, WT_B_CL_IN = 2, WT_B_T_IN = 3,
    WT_B_Q_ACID = 4, WT_B_C_ACID = 5, WT_B_Q_CL = 6, WT_B_C_CL = 7,
    WT_B_T_AMB = 8, WT_B_U = 9,
    WT_NB = 10
};

/* per-reactor status bits (OR-accumulated until cleared) */
enum {
    WT_ST_T_RANGE = 1,        /* a zone temperature left [0,100] C inside the solve: the reference
                                 raises ValueError (thermodynamics.py:146-157); state is NOT advanced
                                 and the reactor stays frozen until the host rewrites its state */
    WT_ST_SOLVER_FAILED = 2,  /* Radau "step size too small" -> reactor.py:486-487 warning; state is
                                 still overwritten with the last accepted y, as the reference does */
    WT_ST_CLAMP_PH = 4,       /* reactor.py:529-531 */
    WT_ST_CLAMP_CL = 8,       /* reactor.py:534-536 */
    WT_ST_CLAMP_T = 16,       /* reactor.py:539-541 */
    WT_ST_T_RANGE_POST = 32,  /* ValueError out of _update_derived_state (reactor.py:522-524):
                                 state/time/H/density were updated, decay rate and clamps were not */
    WT_ST_NONFINITE = 64,     /* the state is not finite at the start of a step: scipy's solve_ivp raises ValueError
                                 ("All components of the initial state `y0` must be finite."), self.state untouched;
                                 the reactor does not advance until the host rewrites its state */
    WT_ST_STEP_LIMIT = 128    /* not a reference behaviour: the attempt limit of wt_ensemble_set_step_limit was hit;
                                 always together with WT_ST_SOLVER_FAILED, state = last accepted y */
};

enum {
    WT_OK = 0, WT_E_ARG = 1, WT_E_HIP = 2, WT_E_NOGPU = 3, WT_E_STATE = 4
};

typedef struct wt_ensemble wt_ensemble;

/* per-reactor solver counters of the LAST outer step (scipy's nfev/njev/nlu,
 * accepted and rejected internal steps); used by the parity tests to check the
 * decision sequence against the oracle. */
typedef struct { int32_t nfev, njev, nlu, nsteps, nrej; } wt_solver_stats;

int wt_abi_version(void);
const char *wt_last_error(void);
int wt_device_count(int *count);

/* IntegratedCSTR.__init__ (reactor.py:203-227) for N reactors with n zones each
 * on HIP device `device`.  `par` is host memory, [WT_NP][N]. */
int wt_ensemble_create(int64_t n_reactors, int n_zones, int device, const double *par,
                       wt_ensemble **out);
int wt_ensemble_destroy(wt_ensemble *h);

/* overwrite reactor.state.{pH,chlorine,temperature,time} (reactor.py:217-222,
 * and the documented "callers may edit state between steps" path :467-469).
 * Host arrays [N][n]; `time` [N] may be NULL (keeps current).  Clears status. */
int wt_ensemble_set_state(wt_ensemble *h, const double *pH, const double *Cl, const double *T,
                          const double *time);
/* BoundaryConditions for every reactor (reactor.py:150-186), host [WT_NB][N].  The handle keeps the bytes it last
 * uploaded and knows whether the device's block still is that block: a call with the same bytes (memcmp: -0.0 is not
 * 0.0, a NaN equals only the same NaN) then returns WT_OK without a device call.  The device's block stops being the
 * host's where the library writes it: a step call under plant I/O, a disturbance or a train program, and every host
 * operation of those two programs (set, clear, set_boundary itself, set_state under a train program, pipe_set); the
 * next call uploads whatever its bytes.  wt_ensemble_info(WT_INFO_BOUNDARY_UPLOADS) counts the calls that uploaded. */
int wt_ensemble_set_boundary(wt_ensemble *h, const double *bc);

/* IntegratedCSTR.step(dt, boundary) n_steps times (reactor.py:450-509); asynchronous, ordered after and
 * before other work on the handle's stream.  The boundary is held constant unless plant I/O is on (then the
 * command path rewrites rows 0 / 4 / 6 at every PLC scan) or a disturbance program is set (then it rewrites its
 * targeted rows after every outer step, wt_ensemble_disturb_set).  fused == 0 makes every outer step a PLC scan, as the reference's
 * loop does; otherwise a scan happens every chunk_steps outer steps and at the end of the call.  Results do not
 * depend on the schedule (tests assert bitwise equality).  A time series of boundaries goes through
 * wt_ensemble_step_scheduled. */
int wt_ensemble_step(wt_ensemble *h, double dt, int n_steps, int fused);
/* IntegratedCSTR.step(dt, bc_schedule[k]) for k = 0 .. n_steps-1: row k (host [n_steps][WT_NB][N]) is the boundary of
 * outer step k of this call (open-loop forcing: dosing pulses, inlet ramps, flow steps).  Same schedules, fused semantics
 * and results as n_steps calls of wt_ensemble_set_boundary(row k) + wt_ensemble_step(h, dt, 1, fused), bit for bit.
 * The rows are uploaded into a device buffer of the handle (grown on demand) and the call synchronises the stream before
 * its launches.  Afterwards the handle's boundary block is row n_steps-1 (wt_ensemble_get_boundary, wt_ensemble_rhs and
 * later wt_ensemble_step calls see it, and a wt_ensemble_set_boundary of that row has nothing to upload).  WT_E_STATE
 * while plant I/O is on (the command path owns the boundary) or a
 * disturbance program is set (its STEP and RAMP slots script events). */
int wt_ensemble_step_scheduled(wt_ensemble *h, double dt, int n_steps, int fused, const double *bc_schedule);
/* Trajectory recording.  From this call on, the state after every `every`-th outer step of later step calls (scheduled
 * or not) goes into record i = (steps since this call) / every - 1, for i < capacity; after that, recording stops.
 * A record holds what wt_ensemble_get_snapshot would have returned after that outer step: state, time, flow and the
 * status word (a stopped reactor keeps its frozen state and time, its status shows why).  Records are indexed by
 * reactor, whatever the placement.  capacity == 0 switches recording off and frees the buffers; calling it again
 * restarts the count.  Synchronises the stream. */
int wt_ensemble_record(wt_ensemble *h, int every, int capacity);
/* records [n_records][N][n] (pH, Cl, T), [n_records][N] (time, flow, status); any pointer may be NULL; synchronises.
 * n_records = min(capacity, steps since wt_ensemble_record / every).  WT_E_STATE when recording is off. */
int wt_ensemble_get_record(wt_ensemble *h, double *pH, double *Cl, double *T, double *time, double *flow,
                           uint32_t *status, int *n_records);
/* Schedule.  n_streams == 0 (default), WT_SCHED_QUEUE: one kernel launch per call; worker wavefronts take
 * (wavefront-group, next few outer steps) work items from a device-side FIFO, so no wavefront ever waits for a
 * launch boundary and a scan per outer step costs no launch.  n_streams >= 1, WT_SCHED_STREAMS (the round-1
 * schedule, kept for comparison): n_streams contiguous reactor ranges on internal HIP streams (fork/join around
 * the handle's stream), launches of at most chunk_steps outer steps.  chunk_steps is the PLC scan interval under
 * both (0 = one scan per call).  Default: queue, WT_DEFAULT_CHUNK. */
int wt_ensemble_set_schedule(wt_ensemble *h, int n_streams, int chunk_steps);
/* the schedule in force: mode (WT_SCHED_*), reactor ranges / streams (0 under WT_SCHED_QUEUE), scan interval,
 * worker wavefronts of the queue schedule (0 under WT_SCHED_STREAMS) */
enum { WT_SCHED_STREAMS = 0, WT_SCHED_QUEUE = 1 };
int wt_ensemble_get_schedule(wt_ensemble *h, int *mode, int *n_streams, int *chunk_steps, int *workers);
/* outer steps a wavefront-group's state stays in registers before it goes back to memory, for a call of n_steps:
 * the work-item length of the queue schedule (n_steps / 6, at most 32), the launch length of the stream schedule */
int wt_ensemble_item_steps(wt_ensemble *h, int n_steps);
/* Launch-completeness record, sticky for the life of the handle: bit 0 = a work-queue hand-off gave up waiting, bit 1 =
 * a launch ended with a wavefront-group short of its step count (checked on the device after every queue launch).
 * Never observed; while it is non-zero wt_ensemble_synchronize and every state download (get_state / get_snapshot /
 * get_status) return WT_E_HIP instead of passing an incomplete state off as WT_OK. */
int wt_ensemble_queue_error(wt_ensemble *h, int *error);
/* Kept for ABI compatibility, no effect: the reactors sharing a wavefront always start an outer step
 * together (they wait for the slowest of them), which is what makes the end of an outer step a
 * wavefront-uniform point for the sensor suite and the PLC scan.  Results never depended on it. */
int wt_ensemble_set_sync(wt_ensemble *h, int sync_outer);
/* Placement of reactors into wavefronts.  Reactors never interact (but for the stages of a train, which are dealt
 * together: wt_ensemble_train_set), so which of them share a wavefront changes no
 * result bit -- but a wavefront costs what its slowest reactor costs.  WT_PLACE_ADAPTIVE (default): once the cost
 * history (the solver's RHS evaluations per reactor) covers WT_PLACE_MIN_STEPS outer steps, the next wt_ensemble_step
 * call re-deals the wavefront slots in order of cost (device-side stable counting sort on the handle's stream, no
 * synchronisation) and restarts the history.  WT_PLACE_IDENTITY: reactor r sits in slot r, as in round 1.
 * wt_ensemble_get_placement: current mode and slot -> reactor table [N] (either pointer may be NULL; the table
 * synchronises the stream).  No counterpart in the reference (one reactor per process). */
#define WT_PLACE_IDENTITY 0
#define WT_PLACE_ADAPTIVE 1
#define WT_PLACE_MIN_STEPS 32
int wt_ensemble_set_placement(wt_ensemble *h, int mode);
int wt_ensemble_get_placement(wt_ensemble *h, int *mode, int32_t *perm);
/* how often the slots have been re-dealt so far, and how many outer steps the running cost history covers
 * (a short run -- fewer than WT_PLACE_MIN_STEPS steps before its timed call -- never re-deals) */
int wt_ensemble_placement_info(wt_ensemble *h, int64_t *redeals, int64_t *history_steps);

/* Guard the reference lacks.  Where the solution slides along a discontinuity of the RHS (the
 * 8 degC density branch, spatial.py:177-189, under strong heat loss) scipy's Radau takes millions
 * of internal steps for one outer step; the reference would grind through them for hours.  A
 * reactor that needs more than max_attempts step attempts (accepted + rejected) in one outer step
 * is stopped like a solver failure (WT_ST_SOLVER_FAILED | WT_ST_STEP_LIMIT).  Default 2000
 * (a normal step needs 2-4, a hard one a few dozen); 0 = unlimited, as the reference -- an explicit opt-in: the
 * step kernel cannot be cancelled, and a reactor on that discontinuity then holds its wavefront (and every download)
 * for as long as the reference would take. */
int wt_ensemble_set_step_limit(wt_ensemble *h, int max_attempts);
int wt_ensemble_synchronize(wt_ensemble *h);

/* ReactorState read-back (reactor.py:113-147).  Any pointer may be NULL.
 * pH/Cl/T [N][n]; time, flow [N]. Synchronises the stream.  Ensembles whose whole image fits 256 KiB (the single-reactor
 * drop-in above all) come back as one packed copy through pinned memory: one kernel, one copy, one synchronisation. */
int wt_ensemble_get_state(wt_ensemble *h, double *pH, double *Cl, double *T, double *time,
                          double *flow);
/* everything a ReactorState holds plus the status words, one synchronisation (any pointer may be NULL) */
int wt_ensemble_get_snapshot(wt_ensemble *h, double *pH, double *Cl, double *T, double *time, double *flow,
                             double *H, double *rho, double *kdecay, uint32_t *flags);
/* H_concentration, density, chlorine_decay_rate (reactor.py:511-524), [N][n] each. */
int wt_ensemble_get_derived(wt_ensemble *h, double *H, double *rho, double *kdecay);
int wt_ensemble_get_status(wt_ensemble *h, uint32_t *flags /* [N] */);
/* the temperature the reference's ValueError names (thermodynamics.py:151: the first out-of-range zone of the
 * evaluation that raised) for reactors flagged WT_ST_T_RANGE / WT_ST_T_RANGE_POST; [N], undefined elsewhere */
int wt_ensemble_get_bad_temperature(wt_ensemble *h, double *value /* [N] */);
int wt_ensemble_clear_status(wt_ensemble *h);
int wt_ensemble_get_stats(wt_ensemble *h, wt_solver_stats *stats /* [N] */);

/* IntegratedCSTR.derivatives(t, y, boundary) (reactor.py:272-448) for every
 * reactor at caller-supplied states (host [N][n]); uses the handle's constants
 * and boundary.  flags[N] gets WT_ST_T_RANGE where the reference would raise. */
int wt_ensemble_rhs(wt_ensemble *h, const double *pH, const double *Cl, const double *T,
                    double *dpH, double *dCl, double *dT, uint32_t *flags);

/* Device-side access for zero-copy consumers (RCCL gather, fused sensors):
 * copies the current state into caller DEVICE memory laid out [3][N][n]
 * (pH, Cl, T), asynchronously on the handle's stream. */
int wt_ensemble_export_state_device(wt_ensemble *h, void *dst_device);
/* Use a caller-owned hipStream_t (e.g. torch's current stream) for all work. */
int wt_ensemble_set_stream(wt_ensemble *h, void *hip_stream);

/* Per-launch HIP-event timing (start/stop events around every step-kernel launch on
 * the stream it is launched on).  launch_stats synchronises, returns the number of
 * launches since timing was switched on / last read, the sum and the maximum of their
 * durations, and resets the counters. */
int wt_ensemble_launch_timing(wt_ensemble *h, int enable);
int wt_ensemble_launch_stats(wt_ensemble *h, int64_t *n_launches, double *sum_ms, double *max_ms);

/* HIP-event bracketing on the handle's stream, for benchmarks. */
int wt_ensemble_timer_start(wt_ensemble *h);
int wt_ensemble_timer_stop(wt_ensemble *h, float *elapsed_ms /* synchronises */);

/* ---- fused sensor suite (SURVEY.md section 8(f) NEXT-1, BASELINE config 5; fp32 signal path) ----
 * create_realistic_sensor_suite + initialize_sensors (sensors/__init__.py:41-120, __main__.py:84-118) for
 * every reactor: pH inlet/outlet, chlorine amperometric inlet / DPD outlet, magnetic flow, RTD inlet/outlet,
 * calibrated at the current ensemble time.  From then on every outer step of wt_ensemble_step is followed
 * by read_all_sensors (__main__.py:121-163) on the device.  Randomness: Philox4x32-10, key = seed,
 * counter = (reactor_base + reactor, sensor, draw index).  cfg_* are host arrays [N] of
 * ReactorConfiguration.flow_rate / initial_chlorine / temperature.  history_capacity > 0 keeps the first
 * that many reads of every sensor on the device (tests, replay). */
#define WT_N_SENSORS 7  /* order: pH_inlet, pH_outlet, chlorine_inlet, chlorine_outlet, flow_main, temp_inlet, temp_outlet */
int wt_ensemble_sensors_enable(wt_ensemble *h, uint64_t seed, int64_t reactor_base, const double *cfg_flow,
                               const double *cfg_chlorine, const double *cfg_temperature, int history_capacity);
/* last SensorReading.value / status / fault of every sensor: [WT_N_SENSORS][N]; status and fault use the
 * declaration order of SensorStatus / SensorFault (sensors/base_sensor.py:49-75). */
int wt_ensemble_sensors_get(wt_ensemble *h, float *values, uint8_t *status, uint8_t *fault);
/* recorded reads [history_capacity][WT_N_SENSORS][N] and the number of reads taken per reactor [N] */
int wt_ensemble_sensors_history(wt_ensemble *h, float *values, uint8_t *status, uint8_t *fault, int32_t *n_filled);

/* ---- plant I/O around the step (SURVEY.md section 8(f) NEXT-2 driver loop, NEXT-3 register image) ----
 * One virtual Modbus slave per reactor, as the reference's loop body keeps it (__main__.py:398-427):
 * after every launch of wt_ensemble_step (= one PLC scan; wt_ensemble_set_schedule's chunk_steps, or
 * fused = 0 for a scan per outer step as in the reference) the device runs, for the reactors of the launch,
 *   update_modbus_inputs   (__main__.py:166-224; encoder modbus/protocols.py:35-58; map register_map.py:119-244,364-401)
 *   read_modbus_commands + apply_boundary_conditions (__main__.py:227-271; decoder protocols.py:155-177)
 * so a command written to the holding image acts from the next scan on.  Needs the sensor suite.
 * Input image: [N][WT_IR_WORDS] uint16, words 0..15 = input registers 0..15 (pH_inlet 0-1, pH_middle 2-3
 * (never written), pH_outlet 4-5, chlorine_inlet 6-7, chlorine_outlet 8-9, flow_rate 10-11, temperature_inlet
 * 12-13, temperature_outlet 14-15), 16-17 = simulation_time (registers 100-101: the loop's sim_time, which
 * lags ReactorState.time by one dt, __main__.py:413,446), 18 = system_status (register 102),
 * 19 = discrete inputs 0..2 (sensor_fault_pH_inlet, _pH_outlet, _chlorine) in bits 0..2.  float32 values
 * occupy (high word, low word).  Holding image: [N][WT_HR_WORDS] uint16 = holding registers 0..5
 * (acid_flow_rate, chlorine_flow_rate, inlet_flow_rate), all 0 at start like the reference's data block. */
#define WT_IR_WORDS 20
#define WT_HR_WORDS 6
int wt_ensemble_plc_enable(wt_ensemble *h);
/* what Modbus masters wrote since the last scan, for reactors [first_reactor, first_reactor + count) */
int wt_ensemble_plc_write_holding(wt_ensemble *h, const uint16_t *words, int64_t first_reactor, int64_t count);
/* input image [N][WT_IR_WORDS]; update_ok[N] = 0 where the last update raised in the reference
 * (a value outside +-1e9, modbus/slave.py:146-147: registers written before it are new, the rest stale) */
int wt_ensemble_plc_read_inputs(wt_ensemble *h, uint16_t *words, uint8_t *update_ok);
/* device pointers of both images for co-resident servers / controllers (synchronise first) */
int wt_ensemble_plc_device(wt_ensemble *h, void **input_image, void **holding_image);
/* current boundary block [WT_NB][N] (after the command path acted on it) */
int wt_ensemble_get_boundary(wt_ensemble *h, double *bc);

/* ---- what the handle holds, for callers that ask instead of remembering ----
 * One host value per code, no device call and no synchronisation: switches give 0 or 1, capacities the size the
 * download of that name fills (0 while its part is off).  WT_INFO_PROGRAM + WT_PROG_*: that program is set.
 * WT_INFO_SCORE_BINS is 0 without a curve, as the fan is.  WT_INFO_WAVE_DIAG: the wave diagnostics are allocated (the
 * next wt_ensemble_wave_diag call copies instead of switching on).  WT_INFO_BOUNDARY_UPLOADS: wt_ensemble_set_boundary
 * calls that uploaded since creation.  WT_INFO_MARK: a mark is set.  An unknown code gives WT_E_ARG. */
enum {
    WT_INFO_PLANT_IO = 0,
    WT_INFO_PROGRAM = 1,                  /* + WT_PROG_CONTROL .. WT_PROG_TREND: codes 1..8 */
    WT_INFO_TRAIN = 9, WT_INFO_PIPE = 10,
    WT_INFO_SENSOR_HISTORY = 11,          /* history_capacity of wt_ensemble_sensors_enable */
    WT_INFO_DISTURB_HISTORY = 12,         /* history_capacity of wt_ensemble_disturb_set */
    WT_INFO_SCORE_CURVE = 13, WT_INFO_SCORE_BINS = 14,   /* curve_capacity and bins of wt_ensemble_score_set */
    WT_INFO_TREND_CAPACITY = 15,          /* capacity of wt_ensemble_trend_set */
    WT_INFO_TRAIN_LENGTH = 16,            /* length of wt_ensemble_train_set */
    WT_INFO_WAVE_DIAG = 17,
    WT_INFO_BOUNDARY_UPLOADS = 18,
    WT_INFO_WIRE = 19,                    /* a wire program is set */
    WT_INFO_MARK = 20,                    /* a mark is set (wt_ensemble_mark) */
    WT_INFO_JUNCTION = 21,                /* a junction program is set */
    WT_INFO_SERVICE = 22,                 /* a sensor service program is set */
    WT_INFO_TUNE = 23,                    /* a tune program is set */
    WT_INFO_INSTALL = 24,                 /* an installation is set (wt_ensemble_install_set) */
    WT_INFO_MPC = 25,                     /* model predictive controllers are set (wt_ensemble_mpc_set) */
    WT_INFO_RESPOND = 26,                 /* a response program is set (wt_ensemble_respond_set) */
    WT_INFO_LINK = 27                     /* a link program is set (wt_ensemble_link_set) */
};
int wt_ensemble_info(wt_ensemble *h, int what, int64_t *value);

/* ---- per-reactor PI dosing programs on the device (closed loop without a host round trip) ----
 * The master side of the reference's loop (__main__.py:227-271) -- whatever a Modbus master computes from the input
 * image and writes into the holding registers between two scans -- as a "virtual PLC program" per reactor; the
 * reference has no controller of its own.  Up to two independent PI loops: loop 0 doses chlorine (holding words 2-3,
 * chlorine_flow_rate), loop 1 acid (words 0-1, acid_flow_rate).  At every PLC scan, for a reactor that stepped, after
 * that scan's update_modbus_inputs and read_modbus_commands, each enabled loop takes v = the scan's raw reading of its
 * sensor and f = its fault code, t_now = the loop time the scan stores, h = t_now - t_prev (t_prev = t_now afterwards;
 * one t_prev per reactor, set to the loop time at enable), and without fused multiply-adds:
 *   hold when v is not finite or f != 0: n_held += 1, nothing else changes, nothing is written;
 *   e = direction * (setpoint - (double)v);  Ic = integral + (ki * e) * h;  u = (bias + kp * e) + Ic;
 *   if ((u > out_max && e > 0) || (u < out_min && e < 0)) { Ic = integral; u = (bias + kp * e) + Ic; }
 *   y = fmin(fmax(u, out_min), out_max);  integral = Ic;  output = y;  holding words = float32(y) (high, low);
 *   ise += (e * e) * h;  iae += fabs(e) * h;  dose += y * h;  n_exec += 1;  n_sat += (y != u).
 * So the output acts from the next scan on, through the unchanged command path -- the same bits as a host master
 * that reads the readings after every call of one scan interval and writes its commands before the next.
 * params: host [WT_CTL_LOOPS][WT_NC][N]; all finite, enable 0 or 1, sensor an integer 0..6 (WT_N_SENSORS order),
 * direction +1 (direct) or -1 (reverse), kp, ki >= 0 (ki per second), out_min <= out_max; otherwise WT_E_ARG.
 * Needs plant I/O (WT_E_STATE).  enable: every enabled loop starts with integral 0, output and holding words the
 * float32 of fmin(fmax(bias, out_min), out_max), metrics 0.  A disabled loop never touches its words.  retune: new
 * parameters; state, metrics and t_prev stay, a loop it switches on starts as at enable.  retune reads the records in
 * force from the device, so it sees the gains and the integral a tune program commissioned (wt_ensemble_tune_set): a
 * loop it keeps on keeps its commissioned state, and wt_ensemble_program_params returns the commissioned kp and ki.
 * All synchronise. */
#define WT_CTL_LOOPS 2
enum {
    WT_C_ENABLE = 0, WT_C_SENSOR = 1, WT_C_DIRECTION = 2, WT_C_SETPOINT = 3, WT_C_KP = 4, WT_C_KI = 5, WT_C_BIAS = 6,
    WT_C_OUT_MIN = 7, WT_C_OUT_MAX = 8,
    WT_NC = 9
};
enum {
    WT_CS_INTEGRAL = 0, WT_CS_OUTPUT = 1, WT_CS_ISE = 2, WT_CS_IAE = 3, WT_CS_DOSE = 4, WT_CS_N_EXEC = 5,
    WT_CS_N_HELD = 6, WT_CS_N_SAT = 7,
    WT_NCS = 8
};
int wt_ensemble_control_enable(wt_ensemble *h, const double *params /* [WT_CTL_LOOPS][WT_NC][N] */);
int wt_ensemble_control_retune(wt_ensemble *h, const double *params /* [WT_CTL_LOOPS][WT_NC][N] */);
/* controller state by reactor: host [WT_CTL_LOOPS][WT_NCS][N]; synchronises; WT_E_STATE while control is off */
int wt_ensemble_control_get(wt_ensemble *h, double *state);
/* control off, buffers freed; the holding words keep the last outputs (no effect while control is off) */
int wt_ensemble_control_disable(wt_ensemble *h);

/* ---- per-reactor injection programs: scripted sensor spoofing and command tampering at every PLC scan ----
 * The cyber layer between the plant and its controller under attack or fault, in the spirit of the reference's
 * roadmap item "fault injection framework (scripted scenarios)"; its sensors only fail at random.  Up to
 * WT_INJ_SLOTS slots per reactor, each (mode, target, t_start, t_end, a, b).  Targets 0..6 are the sensors in
 * WT_N_SENSORS order, WT_INJ_CMD_ACID / _CHLORINE / _INLET the decoded acid, chlorine and inlet flow commands.  At
 * every PLC scan, for a reactor that stepped, with t = the loop time the scan stores (the PI programs' t_now), a slot
 * is active when t_start <= t < t_end; active slots apply in ascending order, each to its target's current value
 * (the previous slot's output).  One application takes x = (double) of the incoming float32 and, without fused
 * multiply-adds, gives x' rounded once to float32 (round to nearest even):
 *   1 BIAS x + a;  2 GAIN x * a;  3 CONSTANT a;  4 RAMP x + (a + b * (t - t_start));
 *   5 FREEZE held, the incoming value at the slot's first application (a replay);  6 DROPOUT NaN;
 *   7 FAULT (sensors only) the value unchanged, the fault code (int)a;  0 OFF: the slot is ignored.
 * and n_applied += 1, t_first = t at the first application, t_last = t.
 * Sensor targets act on the scan's copy of the readings before update_modbus_inputs: the input image and the PI
 * programs see the tampered value; the instrument (its state, wt_ensemble_sensors_get, the history) does not.  The
 * image follows update_input_register: a value outside +-1e9 raises there, which leaves the rest of the image stale
 * and update_ok 0.  Command targets act on the float32 each holding word pair decodes to, before
 * validate_flow_rate: the clamps, NaN -> 0 and the inlet's > 0.1 rule see the tampered value; the holding image
 * keeps the words the master (or the PI program) wrote.
 * params: host [WT_INJ_SLOTS][WT_NI][N]; mode an integer 0..7, target an integer 0..9, t_start finite, t_end finite
 * or +inf and >= t_start, a and b finite, a FAULT slot targets a sensor and has a an integer 1..6 (a SensorFault code); otherwise
 * WT_E_ARG.  Needs plant I/O and n <= 32 zones (WT_E_STATE: the n > 32 kernel has no registers for it).  set
 * resets the state (counts 0, times and held NaN); all synchronise. */
#define WT_INJ_SLOTS 4
enum {
    WT_INJ_OFF = 0, WT_INJ_BIAS = 1, WT_INJ_GAIN = 2, WT_INJ_CONSTANT = 3, WT_INJ_RAMP = 4, WT_INJ_FREEZE = 5,
    WT_INJ_DROPOUT = 6, WT_INJ_FAULT = 7
};
enum { WT_INJ_CMD_ACID = 7, WT_INJ_CMD_CHLORINE = 8, WT_INJ_CMD_INLET = 9, WT_INJ_N_TARGETS = 10 };
enum { WT_I_MODE = 0, WT_I_TARGET = 1, WT_I_T_START = 2, WT_I_T_END = 3, WT_I_A = 4, WT_I_B = 5, WT_NI = 6 };
enum { WT_IS_N_APPLIED = 0, WT_IS_T_FIRST = 1, WT_IS_T_LAST = 2, WT_IS_HELD = 3, WT_NIS = 4 };
int wt_ensemble_inject_set(wt_ensemble *h, const double *params /* [WT_INJ_SLOTS][WT_NI][N] */);
/* slot state by reactor: host [WT_INJ_SLOTS][WT_NIS][N]; synchronises; WT_E_STATE while no program is set */
int wt_ensemble_inject_get(wt_ensemble *h, double *state);
/* program off, buffers freed (no effect while none is set) */
int wt_ensemble_inject_clear(wt_ensemble *h);

/* ---- per-reactor alarm and interlock programs: limits on a reading and trips of the dosing pumps at every PLC scan ----
 * The safety side of the reference's control layer ("alarm logic and interlocks"), which it lists as missing.  Up to
 * WT_ALM_SLOTS slots per reactor.  Parameters [WT_ALM_SLOTS][WT_NA][N]: kind (0 OFF, 1 HIGH, 2 LOW), sensor (0..6,
 * WT_N_SENSORS order), source (0 IMAGE: the scan's copy of the readings after any injection program, what the input
 * image and the PI programs see; 1 FIELD: the instrument's own reading and fault code of this scan, what
 * wt_ensemble_sensors_get returns, an independent transmitter the man in the middle does not reach), setpoint,
 * deadband >= 0, on_delay >= 0 (seconds), latch (0 or 1), on_bad (0 HOLD, 1 ALARM), action (0 NONE, 1 TRIP_ACID,
 * 2 TRIP_CHLORINE), trip_value ([0, 2] for acid, [0, 1] for chlorine); all finite, otherwise WT_E_ARG.
 * Slot state [WT_ALM_SLOTS][WT_NAS][N]: active, cond, pending, n_act, t_first, t_last, time_active, n_bad.  Reactor
 * state [WT_NAR][N]: t_prev, first_out, ovr_acid, ovr_chlorine, n_ovr_acid, n_ovr_chlorine.  set resets both: all 0,
 * except pending, t_first, t_last, ovr_* NaN, first_out -1 and t_prev the reactor's loop time.
 * At every PLC scan of a reactor that stepped, after its PI program, with t = the loop time the scan stores and
 * without fused multiply-adds:
 *   h = t - t_prev; t_prev = t;
 *   for each slot s = 0..3 with kind != OFF, in ascending order:
 *     if active: time_active += h;
 *     v, f = float32 reading and fault code of sensor from source;  bad = !isfinite(v) || f != 0;
 *     if bad: n_bad += 1, and under HOLD nothing else changes for this slot;
 *     c = bad ? 1 : HIGH: active ? !((double)v < setpoint - deadband) : (double)v > setpoint
 *                   LOW:  active ? !((double)v > setpoint + deadband) : (double)v < setpoint;   cond = c;
 *     if !active: if c { if pending is NaN: pending = t;  if t - pending >= on_delay: active = 1, pending = NaN,
 *                        n_act += 1, t_first = t if NaN, first_out = s if -1 }  else pending = NaN;
 *     else if !c && latch == 0: active = 0;
 *     if active: t_last = t;
 *   ovr_acid = trip_value of the lowest active slot with action TRIP_ACID, else NaN; ovr_chlorine likewise.
 *   word = active bits 0-3 | cond bits 4-7 | (ovr_acid set) << 8 | (ovr_chlorine set) << 9 | (first_out + 1) << 12.
 * Interlock, from the next scan on: right after read_modbus_commands decoded and validated the holding words (and any
 * command tamper acted), ovr_acid not NaN gives acid command = validate_flow_rate((float)ovr_acid, 2.0), boundary
 * row 4 = that value, n_ovr_acid += 1; chlorine likewise (limit 1.0, row 6).  The inlet is never overridden and the
 * holding image keeps the master's words: a host master that writes float32(trip_value) gets the same commands.
 * Reactors that did not step at a scan get neither.  Needs plant I/O and n <= 32 zones (WT_E_STATE); all synchronise. */
#define WT_ALM_SLOTS 4
enum { WT_ALM_OFF = 0, WT_ALM_HIGH = 1, WT_ALM_LOW = 2 };
enum { WT_ALM_IMAGE = 0, WT_ALM_FIELD = 1 };
enum { WT_ALM_HOLD = 0, WT_ALM_ALARM = 1 };
enum { WT_ALM_NONE = 0, WT_ALM_TRIP_ACID = 1, WT_ALM_TRIP_CHLORINE = 2 };
enum {
    WT_A_KIND = 0, WT_A_SENSOR = 1, WT_A_SOURCE = 2, WT_A_SETPOINT = 3, WT_A_DEADBAND = 4, WT_A_ON_DELAY = 5,
    WT_A_LATCH = 6, WT_A_ON_BAD = 7, WT_A_ACTION = 8, WT_A_TRIP_VALUE = 9,
    WT_NA = 10
};
enum {
    WT_AS_ACTIVE = 0, WT_AS_COND = 1, WT_AS_PENDING = 2, WT_AS_N_ACT = 3, WT_AS_T_FIRST = 4, WT_AS_T_LAST = 5,
    WT_AS_TIME_ACTIVE = 6, WT_AS_N_BAD = 7,
    WT_NAS = 8
};
enum {
    WT_AR_T_PREV = 0, WT_AR_FIRST_OUT = 1, WT_AR_OVR_ACID = 2, WT_AR_OVR_CHLORINE = 3, WT_AR_N_OVR_ACID = 4,
    WT_AR_N_OVR_CHLORINE = 5,
    WT_NAR = 6
};
int wt_ensemble_alarm_set(wt_ensemble *h, const double *params /* [WT_ALM_SLOTS][WT_NA][N] */);
/* host [WT_ALM_SLOTS][WT_NAS][N] slot state and [WT_NAR][N] reactor state (either may be NULL); WT_E_STATE while no
 * program is set */
int wt_ensemble_alarm_get(wt_ensemble *h, double *slot_state, double *reactor_state);
/* for each reactor with mask[r] != 0 (mask NULL: all), every latched slot that is active and whose cond is 0 becomes
 * inactive (pending NaN); then ovr_* follow the remaining active slots, first_out returns to -1 when none is active,
 * and the word is rewritten.  A slot whose condition still stands stays active. */
int wt_ensemble_alarm_reset(wt_ensemble *h, const uint8_t *mask /* [N] or NULL */);
/* the alarm words, host uint16 [N] */
int wt_ensemble_alarm_words(wt_ensemble *h, uint16_t *words);
/* device pointer of the alarm words [N] for co-resident servers (synchronise first) */
int wt_ensemble_alarm_device(wt_ensemble *h, void **word);
/* program off, buffers freed (no effect while none is set) */
int wt_ensemble_alarm_clear(wt_ensemble *h);

/* ---- per-reactor actuator programs: the dosing pumps and the inlet valve between the command path and the plant ----
 * The reference's roadmap lists actuator dynamics (valves, pumps) next to its PID module.  One optional final element
 * per reactor and channel: 0 acid (boundary row 4, limit 2.0), 1 chlorine (row 6, limit 1.0), 2 inlet (row 0, limit
 * 20.0), the order of WT_INJ_CMD_*.  Parameters [WT_ACT_CHANNELS][WT_NV][N]: enable (0 or 1), tau >= 0 (seconds,
 * first-order lag), rate > 0 (units per second, +inf: none), backlash >= 0, delay (an integer 0..WT_ACT_MAX_DELAY,
 * scans), fault (0 NONE, 1 STUCK, 2 FAIL_TO), t_fault, t_repair >= t_fault (+inf: never), fail_value; all finite
 * except rate and t_repair; under FAIL_TO fail_value in [0, limit] for acid and chlorine and in (0.1, 20] for the
 * inlet; otherwise WT_E_ARG.  Channel state [WT_ACT_CHANNELS][WT_NVS][N]: position, applied, play, demand, delivered,
 * travel, n_exec, n_rate, n_fault.  set replaces any program: every channel starts with position = play = demand =
 * applied = its boundary row in force and the queue filled with that value, delivered, travel and the counts 0, and
 * t_prev the reactor's loop time.  wt_ensemble_set_boundary later moves no actuator state.
 * At every PLC scan of a reactor that stepped, right after read_modbus_commands decoded and validated the holding
 * words (after any command tamper) and the alarm program's trips, with t = the loop time the scan stores, in fp64
 * without fused multiply-adds:
 *   h = t - t_prev; t_prev = t;
 *   for each enabled channel k = 0..2:
 *     u = acid: the acid command; chlorine: the chlorine command;
 *         inlet: the validated inlet word if it is > 0.1, else demand (the positioner keeps its last setpoint);
 *     delivered += applied * h;  demand = u;
 *     ud = delay == 0 ? u : q[delay - 1];  q shifts by one, q[0] = u   (q: the last WT_ACT_MAX_DELAY demands, newest first)
 *     half = backlash * 0.5;  play = fmax(ud - half, fmin(ud + half, play));
 *     pl = tau > 0 ? (tau * position + h * play) / (tau + h) : play;           (backward Euler)
 *     lim = rate * h;  d = pl - position;
 *     pn = d > lim ? position + lim : d < -lim ? position - lim : pl;  n_rate += (pn != pl);
 *     if fault != NONE and t_fault <= t < t_repair: pn = STUCK ? position : fail_value, n_fault += 1;
 *     travel += fabs(pn - position);  position = pn;  n_exec += 1;
 *     a = fmin(fmax(position, 0.0), limit);
 *     acid, chlorine: applied = a, and a is the command and the boundary row;
 *     inlet: if a > 0.1: applied = a, and a is the command and row 0; otherwise row 0 keeps the value it had before
 *            the scan (the reference's inlet rule) and applied stays.
 * The position is a double, not a float32 register: a channel with tau 0, rate +inf, backlash 0, delay 0 and no fault
 * gives exactly the commands of no program.  A disabled channel never touches its row; reactors that did not step get
 * no evaluation and keep t_prev.  The holding image keeps the master's words.  Needs plant I/O and n <= 32 zones
 * (WT_E_STATE); all synchronise. */
#define WT_ACT_CHANNELS 3
#define WT_ACT_MAX_DELAY 8
enum { WT_ACT_ACID = 0, WT_ACT_CHLORINE = 1, WT_ACT_INLET = 2 };
enum { WT_ACT_NONE = 0, WT_ACT_STUCK = 1, WT_ACT_FAIL_TO = 2 };
enum {
    WT_V_ENABLE = 0, WT_V_TAU = 1, WT_V_RATE = 2, WT_V_BACKLASH = 3, WT_V_DELAY = 4, WT_V_FAULT = 5, WT_V_T_FAULT = 6,
    WT_V_T_REPAIR = 7, WT_V_FAIL_VALUE = 8,
    WT_NV = 9
};
enum {
    WT_VS_POSITION = 0, WT_VS_APPLIED = 1, WT_VS_PLAY = 2, WT_VS_DEMAND = 3, WT_VS_DELIVERED = 4, WT_VS_TRAVEL = 5,
    WT_VS_N_EXEC = 6, WT_VS_N_RATE = 7, WT_VS_N_FAULT = 8,
    WT_NVS = 9
};
int wt_ensemble_actuator_set(wt_ensemble *h, const double *params /* [WT_ACT_CHANNELS][WT_NV][N] */);
/* host [WT_ACT_CHANNELS][WT_NVS][N] channel state, [WT_ACT_CHANNELS][WT_ACT_MAX_DELAY][N] demand queues (newest
 * first) and [N] t_prev (any may be NULL); WT_E_STATE while no program is set */
int wt_ensemble_actuator_get(wt_ensemble *h, double *state, double *queue, double *t_prev);
/* program off, buffers freed (no effect while none is set) */
int wt_ensemble_actuator_clear(wt_ensemble *h);

/* ---- per-reactor disturbance programs: inlet and ambient disturbances generated on the device ----
 * Up to WT_DST_SLOTS slots per reactor move the boundary rows the command path does not own.  Parameters
 * [WT_DST_SLOTS][WT_ND][N]: kind (an integer 0..4: WT_DST_OFF, STEP, RAMP, SINE, OU), row (1 inlet_pH, 2
 * inlet_chlorine, 3 inlet_temperature, 5 acid_concentration, 7 chlorine_concentration, 8 ambient_temperature, 9
 * heat_loss_coefficient; rows 0, 4 and 6 belong to the command path or the master), t_start, t_end >= t_start (may be
 * +inf), a, b, c; all finite except t_end; SINE needs b > 0, OU a >= 0 and b > 0; otherwise WT_E_ARG.
 * Slot state [WT_DST_SLOTS][WT_NDS][N]: value (the offset d), x (the OU state), n_eval, n_draw.
 * The program keeps a base block [WT_NB][N]: the boundary in force at set time.  Every row that at least one non-OFF
 * slot targets is  clamp(base + d_s0 + d_s1 + ...)  over those slots in ascending order, in fp64 without fused
 * multiply-adds; the clamp is [0, 14] for pH, [0, 100] for inlet temperature, none for ambient temperature and >= 0 for
 * rows 2, 5, 7 and 9.  Rows no slot targets are never written.
 * After every outer step of a reactor that stepped (the sensor suite's test: no ReactorState failure after the step),
 * with t = its ReactorState.time after the step:  h = t - t_prev; t_prev = t;  then for every slot, "in window" being
 * t_start <= t < t_end:
 *   STEP  d = in window ? a : 0
 *   RAMP  d = t < t_start ? 0 : a + b * (fmin(t, t_end) - t_start)     (holds its end value after the window)
 *   SINE  d = in window ? a * sin(2 pi (t - t_start) / b + c) : 0
 *   OU    (a = stationary sigma, b = tau in seconds) in window: if h > 0 { phi = exp(-h/b);
 *         x = x * phi + (a * sqrt(-expm1(-2h/b))) * z;  n_draw += 1 }  d = x;  outside: d = 0, x kept
 *   n_eval += 1;  history entry n_eval - 1 = d (while below the capacity)
 * z is one standard normal deviate of the sensor suite's Philox4x32-10 + Box-Muller (fp32) on counter
 * (reactor_base + r, slot, n_draw, 1) and key = seed: word 3 = 1 keeps it off every sensor stream.  The composed rows
 * are the boundary of the reactor's next outer step (zero-order hold); with plant I/O that step integrates under both
 * this step's commands and these rows.  Reactors that did not step get no evaluation and keep their rows.
 * set replaces any program (the old one's rows go back to its base first, as clear does): x = 0, counts 0, t_prev =
 * ReactorState.time, then one evaluation at that time on the device (history entry 0: what the first step after set
 * integrates under).  Needs set_state and set_boundary and n <= 32 zones (WT_E_STATE); history_capacity >= 0
 * (WT_E_ARG).  With a program set, wt_ensemble_set_boundary replaces the base and recomposes the targeted rows from
 * the current offsets (no draw), and wt_ensemble_step_scheduled gives WT_E_STATE.  All calls synchronise. */
#define WT_DST_SLOTS 4
enum { WT_DST_OFF = 0, WT_DST_STEP = 1, WT_DST_RAMP = 2, WT_DST_SINE = 3, WT_DST_OU = 4 };
enum { WT_D_KIND = 0, WT_D_ROW = 1, WT_D_T_START = 2, WT_D_T_END = 3, WT_D_A = 4, WT_D_B = 5, WT_D_C = 6, WT_ND = 7 };
enum { WT_DS_VALUE = 0, WT_DS_X = 1, WT_DS_N_EVAL = 2, WT_DS_N_DRAW = 3, WT_NDS = 4 };
int wt_ensemble_disturb_set(wt_ensemble *h, const double *params /* [WT_DST_SLOTS][WT_ND][N] */, uint64_t seed,
                            int64_t reactor_base, int history_capacity);
/* host [WT_DST_SLOTS][WT_NDS][N] slot state, [WT_NB][N] base and [N] t_prev (any may be NULL); WT_E_STATE while no
 * program is set */
int wt_ensemble_disturb_get(wt_ensemble *h, double *slot_state, double *base, double *t_prev);
/* host [history_capacity][WT_DST_SLOTS][N] offsets (entry j: after evaluation j, entry 0 the one at set time; 0 while
 * not filled) and [N] entries filled (either may be NULL); WT_E_STATE while no program is set */
int wt_ensemble_disturb_history(wt_ensemble *h, double *offsets, int32_t *n_filled);
/* program off, buffers freed, targeted rows back to the base (no effect while none is set) */
int wt_ensemble_disturb_clear(wt_ensemble *h);

/* ---- per-reactor score programs: ground-truth excursion metrics and ensemble curves ----
 * Up to WT_SCR_SLOTS slots per reactor judge the true ReactorState after every outer step against a band; nothing in
 * the plant changes (state, readings, images and program states keep their bits).  Parameters [WT_SCR_SLOTS][WT_NSP][N]:
 * kind (0 WT_SCR_OFF, 1 WT_SCR_BAND), quantity (0 pH, 1 chlorine, 2 temperature: the ReactorState arrays after the
 * step and its clamps), reduce (0 ZONE, 1 MIN, 2 MAX, 3 MEAN over the reactor's zones), zone (an integer -1..31; -1 is
 * the last zone, the outlet; only ZONE reads it), lo <= hi (lo may be -inf, hi +inf, neither NaN), t_start, t_end >=
 * t_start (-inf and +inf allowed, NaN not); otherwise WT_E_ARG.  The set call also refuses zone >= n_zones.
 * Slot state [WT_SCR_SLOTS][WT_NSS][N]: n_eval, time, integral, t_low, t_high, area_low, area_high, v_min, v_max, last,
 * out, n_exc, t_first_out, run, run_max; and a per-reactor t_prev [N].  set zeroes everything except v_min, v_max,
 * last and t_first_out (NaN) and t_prev (ReactorState.time); nothing is evaluated at set time.
 * After every outer step of a reactor that stepped (the sensor suite's test: no ReactorState failure after the step),
 * with t = its ReactorState.time after the step, in fp64 without fused multiply-adds:
 *   h = t - t_prev;  t_prev = t
 *   for each slot s in ascending order with kind != OFF and t_start <= t < t_end:
 *     x[z] = quantity in zone z, n zones
 *     v = ZONE: x[zone < 0 ? n-1 : zone]
 *         MIN:  v = x[0]; for z = 1..n-1: v = x[z] < v ? x[z] : v          (MAX likewise with >)
 *         MEAN: (((x[0] + x[1]) + x[2]) + ... + x[n-1]) / n                 (ascending zone order)
 *     n_eval += 1;  time += h;  integral += v * h;  last = v
 *     v_min = n_eval == 1 ? v : (v < v_min ? v : v_min);   v_max likewise
 *     low = v < lo;  high = v > hi
 *     if low:  t_low  += h;  area_low  += (lo - v) * h
 *     if high: t_high += h;  area_high += (v - hi) * h
 *     if low or high: { if out == 0: n_exc += 1;  if t_first_out is NaN: t_first_out = t;
 *                       out = 1;  run += h;  run_max = run > run_max ? run : run_max }
 *     else:           { out = 0;  run = 0 }
 * Slots outside their window and reactors that did not step change nothing.  (integral of outlet chlorine is the CT
 * exposure, area_low the disinfection deficit, run_max the longest contiguous violation.)
 * Ensemble curve: with curve_capacity C > 0, let j be the number of outer steps the step calls have taken since set or
 * reset (counted for the whole ensemble, as wt_ensemble_record counts).  For j < C every slot evaluation in its window
 * adds 1 to the int32 counts[j][s][0] (scored), to [1] if low and to [2] if high; with bins B in 1..WT_SCR_MAX_BINS
 * also to fan[j][s][b],  b = v < fan_lo[s] ? 0 : v >= fan_hi[s] ? B + 1 : 1 + min(B - 1, (int)((v - fan_lo[s]) * scale)),
 * scale = B / (fan_hi[s] - fan_lo[s]) in fp64 (fan_lo < fan_hi, both finite, else WT_E_ARG; the fan needs C > 0).  The
 * counters are integers added atomically: their values depend neither on the schedule nor on the placement, and those
 * of the shards of one ensemble simply add.
 * set replaces any program.  Needs set_state and n <= 32 zones (WT_E_STATE); neither sensors nor plant I/O.  Works
 * with wt_ensemble_step and wt_ensemble_step_scheduled, every schedule and any split into calls.  All calls synchronise. */
#define WT_SCR_SLOTS 4
#define WT_SCR_MAX_BINS 32
enum { WT_SCR_OFF = 0, WT_SCR_BAND = 1 };
enum { WT_SQ_PH = 0, WT_SQ_CHLORINE = 1, WT_SQ_TEMPERATURE = 2 };
enum { WT_SR_ZONE = 0, WT_SR_MIN = 1, WT_SR_MAX = 2, WT_SR_MEAN = 3 };
enum { WT_SP_KIND = 0, WT_SP_QUANTITY = 1, WT_SP_REDUCE = 2, WT_SP_ZONE = 3, WT_SP_LO = 4, WT_SP_HI = 5, WT_SP_T_START = 6,
       WT_SP_T_END = 7, WT_NSP = 8 };
enum { WT_SS_N_EVAL = 0, WT_SS_TIME = 1, WT_SS_INTEGRAL = 2, WT_SS_T_LOW = 3, WT_SS_T_HIGH = 4, WT_SS_AREA_LOW = 5,
       WT_SS_AREA_HIGH = 6, WT_SS_V_MIN = 7, WT_SS_V_MAX = 8, WT_SS_LAST = 9, WT_SS_OUT = 10, WT_SS_N_EXC = 11,
       WT_SS_T_FIRST_OUT = 12, WT_SS_RUN = 13, WT_SS_RUN_MAX = 14, WT_NSS = 15 };
/* fan_lo, fan_hi: host [WT_SCR_SLOTS], read only for bins > 0 */
int wt_ensemble_score_set(wt_ensemble *h, const double *params /* [WT_SCR_SLOTS][WT_NSP][N] */, int curve_capacity, int bins,
                          const double *fan_lo, const double *fan_hi);
/* host [WT_SCR_SLOTS][WT_NSS][N] slot state and [N] t_prev (either may be NULL); WT_E_STATE while no program is set */
int wt_ensemble_score_get(wt_ensemble *h, double *slot_state, double *t_prev);
/* host [curve_capacity][WT_SCR_SLOTS][3] counts, [curve_capacity][WT_SCR_SLOTS][bins + 2] fan and n_steps = min(C, j), the
 * entries filled (any may be NULL; entries beyond n_steps are 0); WT_E_STATE while no program is set */
int wt_ensemble_score_curve(wt_ensemble *h, int32_t *counts, int32_t *fan, int *n_steps);
/* fan_lo and fan_hi of the set call, host [WT_SCR_SLOTS] each (either may be NULL; 0 without a fan); no device call;
 * WT_E_STATE while no program is set */
int wt_ensemble_score_fan_range(wt_ensemble *h, double *fan_lo, double *fan_hi);
/* accumulators and curve back to their set-time values, j = 0, t_prev = the current ReactorState.time; the parameters
 * stay (scoring after a warm-up); WT_E_STATE while no program is set */
int wt_ensemble_score_reset(wt_ensemble *h);
/* program off, buffers freed (no effect while none is set) */
int wt_ensemble_score_clear(wt_ensemble *h);

/* ---- per-reactor anomaly detector programs: a change-detection statistic at every PLC scan, judged against a label ----
 * What an intrusion- or fault-detection study evaluates: up to WT_DET_SLOTS slots per reactor keep a statistic of the
 * residual of one reading (a limit alarm has no memory of it), raise an alarm where it exceeds a threshold, and count
 * the scans against the reactor's ground-truth attack window.  The program is passive: nothing in the plant changes
 * (state, readings, images, boundary and the other programs' states keep their bits).
 * Parameters [WT_DET_SLOTS][WT_NK][N]: kind (0 OFF, 1 CUSUM, 2 EWMA, 3 FLATLINE), sensor (0..6, WT_N_SENSORS order),
 * source (0 IMAGE, 1 FIELD: the alarm program's meaning), ref (0 CONST, 1 SENSOR, 2 TRACK: what the reading is compared
 * with), ref_arg (CONST: the value; SENSOR: the second sensor's index 0..6; TRACK: the time constant tau > 0 in
 * seconds), ref_source (source of the second sensor, read only for SENSOR), mu (expected residual), sigma > 0 (residual
 * scale), slack (CUSUM: k >= 0; EWMA: lambda in (0, 1]; FLATLINE: eps >= 0 in the sensor's units), limit (CUSUM / EWMA:
 * threshold > 0 on the statistic; FLATLINE: seconds > 0), t_arm (the slot is skipped while t < t_arm: sensor warm-up;
 * finite or -inf), on_bad (0 HOLD, 1 ALARM).  No row may be NaN or infinite (t_arm may be -inf); the rows of an OFF
 * slot after kind are not read and not range-checked.  Otherwise WT_E_ARG.
 * Label [WT_NKR][N]: label_start, label_end, the attack window.  Neither is NaN, label_end >= label_start, both may be
 * infinite (+inf, +inf: never attacked).
 * Slot state [WT_DET_SLOTS][WT_NKS][N]: gp, gn, baseline, x_prev, stat, stat_max, alarm, n_eval, n_bad, n_alarm, n_raise,
 * t_first, t_detect, n_tp, n_fp, n_fn; and a per-reactor t_prev [N].  set gives all 0 except baseline, x_prev, t_first,
 * t_detect NaN and t_prev = the reactor's loop time.
 * At every PLC scan of a reactor that stepped, after its alarm program (last in the scan), with t = the loop time the
 * scan stores, in fp64 with IEEE add, multiply, divide, compare, fmax and fabs only, no fused multiply-adds:
 *   h = t - t_prev;  t_prev = t;  attacked = label_start <= t && t < label_end
 *   for each slot s ascending with kind != OFF and t >= t_arm:
 *     was = alarm
 *     v, f = float32 reading and fault code of `sensor` from `source`;  bad = !isfinite(v) || f != 0
 *     if ref == SENSOR: w, g = reading and fault of sensor (int)ref_arg from ref_source;  bad = bad || !isfinite(w) || g != 0
 *     if bad:  n_bad += 1;  if on_bad == ALARM: alarm = 1     (HOLD: alarm keeps its value; no statistic changes either way)
 *     else:
 *       x = (double)v
 *       base = CONST: ref_arg | SENSOR: (double)w | TRACK: (baseline is NaN ? x : baseline)
 *       if ref == TRACK: baseline = base + (h / (ref_arg + h)) * (x - base)       (after base was taken)
 *       z = ((x - base) - mu) / sigma
 *       CUSUM:    gp = fmax(0, (gp + z) - slack);  gn = fmax(0, (gn - z) - slack);  stat = fmax(gp, gn)
 *       EWMA:     gp = gp + slack * (z - gp);  stat = fabs(gp)
 *       FLATLINE: gp = (x_prev is not NaN && fabs(x - x_prev) <= slack) ? gp + h : 0;  stat = gp
 *       x_prev = x;  alarm = stat > limit;  stat_max = stat > stat_max ? stat : stat_max
 *     n_eval += 1
 *     if alarm: n_alarm += 1;  if !was: n_raise += 1;  if t_first is NaN: t_first = t
 *               if t >= label_start && t_detect is NaN: t_detect = t
 *     attacked ? (alarm ? n_tp : n_fn) += 1 : (alarm ? n_fp += 1 : nothing)      (true negatives = n_eval - n_tp - n_fn - n_fp)
 * Reactors that did not step and slots before t_arm change nothing.  Alarms do not latch and the statistics are not
 * reset by an alarm.  set replaces any program.  Needs plant I/O and n <= 32 zones (WT_E_STATE), neither an injection
 * nor a control program; all calls synchronise. */
#define WT_DET_SLOTS 4
enum { WT_DET_OFF = 0, WT_DET_CUSUM = 1, WT_DET_EWMA = 2, WT_DET_FLATLINE = 3 };
enum { WT_DET_IMAGE = 0, WT_DET_FIELD = 1 };
enum { WT_DET_CONST = 0, WT_DET_SENSOR = 1, WT_DET_TRACK = 2 };
enum { WT_DET_HOLD = 0, WT_DET_ALARM = 1 };
enum {
    WT_K_KIND = 0, WT_K_SENSOR = 1, WT_K_SOURCE = 2, WT_K_REF = 3, WT_K_REF_ARG = 4, WT_K_REF_SOURCE = 5, WT_K_MU = 6,
    WT_K_SIGMA = 7, WT_K_SLACK = 8, WT_K_LIMIT = 9, WT_K_T_ARM = 10, WT_K_ON_BAD = 11,
    WT_NK = 12
};
enum {
    WT_KS_GP = 0, WT_KS_GN = 1, WT_KS_BASELINE = 2, WT_KS_X_PREV = 3, WT_KS_STAT = 4, WT_KS_STAT_MAX = 5, WT_KS_ALARM = 6,
    WT_KS_N_EVAL = 7, WT_KS_N_BAD = 8, WT_KS_N_ALARM = 9, WT_KS_N_RAISE = 10, WT_KS_T_FIRST = 11, WT_KS_T_DETECT = 12,
    WT_KS_N_TP = 13, WT_KS_N_FP = 14, WT_KS_N_FN = 15,
    WT_NKS = 16
};
enum { WT_KR_LABEL_START = 0, WT_KR_LABEL_END = 1, WT_NKR = 2 };
int wt_ensemble_detect_set(wt_ensemble *h, const double *params /* [WT_DET_SLOTS][WT_NK][N] */, const double *labels /* [WT_NKR][N] */);
/* host [WT_DET_SLOTS][WT_NKS][N] slot state and [N] t_prev (either may be NULL); WT_E_STATE while no program is set */
int wt_ensemble_detect_get(wt_ensemble *h, double *slot_state, double *t_prev);
/* the label block of the set call, host [WT_NKR][N]; synchronises; WT_E_STATE while no program is set */
int wt_ensemble_detect_labels(wt_ensemble *h, double *labels);
/* slot state and t_prev back to their set-time values at the current loop time; parameters and labels stay (detection
 * after a warm-up); WT_E_STATE while no program is set */
int wt_ensemble_detect_reset(wt_ensemble *h);
/* program off, buffers freed (no effect while none is set) */
int wt_ensemble_detect_clear(wt_ensemble *h);

/* ---- per-reactor trend recorder programs: the historian, a time series per slot at the PLC scan rate ----
 * A fused call returns end-of-call state.  The series a study plots at the scan rate -- a PI output, a detector's
 * statistic, valve position against command, the alarm word -- are recorded inside the call: up to WT_TRD_SLOTS slots
 * per reactor each take one value of every scan, thin it and append (time, value) to a store of `capacity` samples per
 * slot and reactor.  The program is passive (it writes its own arrays only) and its values are copies, so a series is
 * bit for bit what a host loop of one call per scan reads from the getters named below.
 * Parameters [WT_TRD_SLOTS][WT_NT][N]: tag, index, every (whole, >= 1: a candidate every that many scans seen), deadband
 * (< 0: every candidate is recorded; otherwise only a value that differs from the last recorded one by more than it;
 * not NaN), t_start, t_end (the slot sees a scan while t_start <= t < t_end; neither NaN, t_end >= t_start, both may be
 * infinite).  The rows of an OFF slot after tag are not read and not checked.  Otherwise WT_E_ARG.
 * tag and the entries index selects (a whole number in the range given), the value taken as fp64:
 *   0 OFF
 *   1 IMAGE_VALUE  sensor 0..6 (WT_N_SENSORS order): this scan's copy of the reading after any injection program
 *   2 IMAGE_FAULT  sensor 0..6: its fault code
 *   3 FIELD_VALUE  sensor 0..6: the instrument's own reading of this step (wt_ensemble_sensors_get)
 *   4 FIELD_FAULT  sensor 0..6: its fault code
 *   5 COMMAND      channel 0 acid, 1 chlorine, 2 inlet (WT_INJ_CMD_* order): what this scan hands to the plant, the
 *                  value rows 4 / 6 / 0 of wt_ensemble_get_boundary hold after a call that ends at this scan
 *   6 CONTROL      loop * WT_NCS + row: that entry of the wt_ensemble_control_get block at the end of this scan
 *   7 INJECT       slot * WT_NIS + row: likewise of wt_ensemble_inject_get
 *   8 ALARM        slot * WT_NAS + row: likewise of the slot state of wt_ensemble_alarm_get
 *   9 ALARM_WORD   0: the reactor's alarm word (wt_ensemble_alarm_words)
 *  10 ACTUATOR     channel * WT_NVS + row: likewise of the channel state of wt_ensemble_actuator_get
 *  11 DETECT       slot * WT_NKS + row: likewise of the slot state of wt_ensemble_detect_get
 * Tags 6-11 read another program's record; while that program is off the value is NaN.
 * Slot state [WT_TRD_SLOTS][WT_NTS][N]: n_seen, n_recorded, n_dropped, last.  set gives 0, 0, 0, NaN.
 * At every PLC scan of a reactor that stepped, after every other program of the scan (last in the scan), with t = the
 * loop time the scan stores, for each slot ascending with tag != OFF and t_start <= t < t_end:
 *   n_seen += 1;  the scan is a candidate if (n_seen - 1) % every == 0
 *   x = the tag's value;  a candidate is taken if n_recorded == 0, or deadband < 0, or
 *       (x == x || last == last) && !(fabs(x - last) <= deadband)       (NaN to NaN: no change; NaN to or from a number: a change)
 *   a sample taken: wrap == 0 and n_recorded == capacity: n_dropped += 1, nothing stored;
 *                   otherwise (t, x) goes to position n_recorded % capacity (wrap != 0 overwrites the oldest) and n_recorded += 1;
 *                   last = x either way, so the deadband thins the same at any capacity
 * n_recorded counts the samples stored or overwritten; min(n_recorded, capacity) are held.  Reactors that did not step
 * and slots outside their window change nothing.  set replaces any program.  Needs plant I/O and n <= 32 zones
 * (WT_E_STATE); all calls synchronise. */
#define WT_TRD_SLOTS 8
enum {
    WT_TRD_OFF = 0, WT_TRD_IMAGE_VALUE = 1, WT_TRD_IMAGE_FAULT = 2, WT_TRD_FIELD_VALUE = 3, WT_TRD_FIELD_FAULT = 4,
    WT_TRD_COMMAND = 5, WT_TRD_CONTROL = 6, WT_TRD_INJECT = 7, WT_TRD_ALARM = 8, WT_TRD_ALARM_WORD = 9, WT_TRD_ACTUATOR = 10,
    WT_TRD_DETECT = 11
};
enum { WT_T_TAG = 0, WT_T_INDEX = 1, WT_T_EVERY = 2, WT_T_DEADBAND = 3, WT_T_T_START = 4, WT_T_T_END = 5, WT_NT = 6 };
enum { WT_TS_N_SEEN = 0, WT_TS_N_RECORDED = 1, WT_TS_N_DROPPED = 2, WT_TS_LAST = 3, WT_NTS = 4 };
/* capacity >= 1 samples per slot and reactor (WT_E_ARG otherwise, or if the store's size overflows int64) */
int wt_ensemble_trend_set(wt_ensemble *h, const double *params /* [WT_TRD_SLOTS][WT_NT][N] */, int64_t capacity, int wrap);
/* host [WT_TRD_SLOTS][WT_NTS][N] slot state; WT_E_STATE while no program is set */
int wt_ensemble_trend_get(wt_ensemble *h, double *slot_state);
/* host [WT_TRD_SLOTS][capacity][N] each (either may be NULL): every slot's samples in chronological order (a wrapped ring
 * is unwrapped: row k is the k-th oldest sample held); rows past the number held are NaN in both arrays.  WT_E_STATE
 * while no program is set */
int wt_ensemble_trend_data(wt_ensemble *h, double *time, double *value);
/* slot state and store as after set; the parameters, capacity and wrap stay (recording after a warm-up); WT_E_STATE
 * while no program is set */
int wt_ensemble_trend_reset(wt_ensemble *h);
/* program off, buffers freed (no effect while none is set) */
int wt_ensemble_trend_clear(wt_ensemble *h);

/* ---- the train program: reactors coupled into treatment trains ----
 * An ensemble of N reactors is read as N / length trains of `length` stages (rapid mix, contact tank, clearwell ...):
 * reactor r is stage r % length of train r / length, and the upstream of a stage s >= 1 is reactor r - 1.
 * Parameters [WT_NTR][N]: link (0 or 1; a first stage has no upstream, its link must be 0), rows (a whole number 0..7:
 * WT_TRN_PH 1 | WT_TRN_CHLORINE 2 | WT_TRN_TEMPERATURE 4, the rows a feed writes).  NULL: every stage after the first
 * linked, rows 7.
 * Feed.  After every outer step in which the upstream reactor stepped and did not end T_RANGE_POST (the sensor suite's
 * test), pH, Cl and T of the upstream's outlet zone (zone n - 1) are written into rows 1, 2, 3 (inlet_pH,
 * inlet_chlorine, inlet_temperature) of the linked downstream reactor's boundary block, each only if `rows` has its
 * bit, whether or not the downstream reactor itself stepped.  The fed rows are the boundary of the downstream
 * reactor's next outer step (zero-order hold); with plant I/O that step integrates under both this step's commands and
 * these rows.  The state is already clamped to the ranges the rows allow, so no clamp is applied.  An upstream that
 * did not step (a frozen reactor) feeds nothing: its downstream keeps the rows it holds and goes on stepping.
 * Flows are not carried by the train program itself: row 0 belongs to the command path or the master, and every tank
 * keeps its own inlet flow (a junction program on top may carry them, below).
 * Definition (the fused call gives its bits): on a handle without a program, feed every link from the current state,
 * then repeat { one outer step; wt_ensemble_get_state; for every linked reactor whose upstream stepped, rows 1..3 of
 * wt_ensemble_get_boundary <- the upstream's zone n - 1; wt_ensemble_set_boundary }.
 * Feeds outside a step, from the state in memory, to every link: wt_ensemble_train_set itself, wt_ensemble_set_boundary
 * with a program set (after it has stored rows 1..3 of the new block as the program's base), wt_ensemble_set_state.
 * State [WT_NTRS][N]: n_fed (feeds the step kernel wrote into this reactor; those outside a step do not count),
 * t_last (the upstream's ReactorState.time at the last of them, NaN before the first).
 * Where the stages sit.  A train's stages share a wavefront, so length is 2..floor(64 / n_zones) (no train above 32
 * zones) and N a multiple of length.  With a program set the handle holds length * k reactors per wavefront, k chosen
 * like the reactors per wavefront at creation but counted in trains; the placement deals whole trains into consecutive
 * slots in stage order (set starts from reactor r in slot r with an empty cost history).  Wave diagnostics and item
 * trace buffers of the old shape are released by set and clear; their next call starts them again.
 * set replaces any program (the old one's rows go back to its base first, as clear does) and needs set_state and
 * set_boundary (WT_E_STATE: "set_state and set_boundary must precede train_set").  Refused with WT_E_ARG:
 *   "length must be at least 2 and at most 64 / n_zones (the stages of a train share a wavefront)"
 *   "n_reactors must be a multiple of length (an ensemble holds whole trains)"
 *   "link must be 0 or 1"
 *   "the first stage of a train has no upstream: its link must be 0"
 *   "rows must be an integer in 0..7 (1 pH, 2 chlorine, 4 temperature)"
 * in this order, reactor by reactor.  A disturbance slot (not OFF) on row 1, 2 or 3 of a linked reactor whose rows
 * mask has that row would write the cell the train feeds: whichever of wt_ensemble_train_set / wt_ensemble_disturb_set
 * comes second gives WT_E_STATE, "a disturbance slot targets an inlet row (1, 2 or 3) that the train program feeds
 * into that reactor".  While a program is set wt_ensemble_step_scheduled gives WT_E_STATE, "a boundary schedule
 * cannot be combined with a train program (the run itself sets the linked rows)".
 * clear writes the base back into the linked rows (those of the rows mask) and restores the handle's shape; no effect
 * while no program is set.  get gives WT_E_STATE, "no train program is set (wt_ensemble_train_set)", while none is.
 * A shard of a sharded ensemble must hold whole trains.  The program takes no code of wt_program_check:
 * wt_train_check is its check.  All calls synchronise. */
enum { WT_TR_LINK = 0, WT_TR_ROWS = 1, WT_NTR = 2 };
enum { WT_TRS_N_FED = 0, WT_TRS_T_LAST = 1, WT_NTRS = 2 };
enum { WT_TRN_PH = 1, WT_TRN_CHLORINE = 2, WT_TRN_TEMPERATURE = 4 };
int wt_ensemble_train_set(wt_ensemble *h, int length, const double *params /* [WT_NTR][N] or NULL */);
/* the train length, the reactors per wavefront in force and the host [WT_NTRS][N] state (any may be NULL) */
int wt_ensemble_train_get(wt_ensemble *h, int *length, int *per_wavefront, double *state);
/* the parameter block in force, host [WT_NTR][N] (after a set with NULL: the default it stands for); a reactor that is
 * not linked reads rows 0, whatever the set call gave there (nothing reads them).  No device call; WT_E_STATE while no
 * program is set */
int wt_ensemble_train_params(wt_ensemble *h, double *params);
int wt_ensemble_train_clear(wt_ensemble *h);
/* the checks wt_ensemble_train_set makes on its arguments, with no handle and no device: WT_OK or WT_E_ARG with that
 * call's message (also "n_reactors must be >= 1", "n_zones must be in 2..64").  Makes no HIP call. */
int wt_train_check(int length, int n_zones, int64_t n_reactors, const double *params);

/* ---- the pipe program: dead time between the stages of a treatment train ----
 * On top of a set train program, link d (into reactor d, from reactor d - 1) may have a delay line of delay[d] = D
 * whole outer steps, 0..WT_PIPE_MAX_DELAY, between its upstream's outlet and its own inlet rows.  D must be 0 for a
 * reactor that is not linked; the first stage of a train is never linked, so it has no pipe.
 * Line.  The line of link d is a FIFO of exactly D samples.  A sample is (pH, Cl, T of the upstream's outlet zone, the
 * upstream's ReactorState.time when it was taken).  wt_ensemble_pipe_set fills it with D copies of the upstream's
 * outlet from the state in memory, time stamp NaN: the pipe starts full of the water the upstream holds now.
 * Feed.  A feed of link d is the train program's feed: after an outer step in which the upstream stepped and did not
 * end T_RANGE_POST, whether or not the downstream stepped.  The current sample is appended, the oldest is popped, and
 * the popped sample is written into rows 1 / 2 / 3 of reactor d as the link's rows mask says.  All three quantities
 * travel through the line whatever the mask says; the mask only limits what is written at delivery.  A link with
 * D = 0 has no line: it behaves in every call exactly as it does without a pipe program.  An upstream that does not
 * feed (frozen, T_RANGE) pushes nothing and pops nothing: the line stalls and the downstream keeps the rows it holds.
 * Definition (the fused call gives its bits): the train program's host loop with a FIFO per link between
 * wt_ensemble_get_state and wt_ensemble_set_boundary.
 * State [WT_NPS][N]: n_sent (feeds that went through this reactor's line inside step calls; 0 where D = 0), t_sent
 * (the time stamp of the sample last delivered by a step call; NaN before the first delivery and while samples of the
 * initial fill are still coming out).  n_fed / t_last of the train program keep their meaning: they count deliveries
 * and hold the upstream's time at the delivery.
 * Outside a step, with a pipe program set: wt_ensemble_set_state refills every line from the new state and restarts
 * the pipe state (a new state is a new plant); wt_ensemble_set_boundary stores rows 1..3 as the train program's base
 * and writes the linked rows again -- D = 0: the upstream's outlet from the state in memory, D >= 1: the sample the
 * line last delivered (after a set or a refill: the sample it was filled with).
 * wt_ensemble_pipe_set needs a train program (WT_E_STATE, "no train program is set (wt_ensemble_train_set)"), fills
 * the lines, delivers every link again from the state in memory and replaces any pipe program.  Refused with WT_E_ARG:
 *   "delay must be a whole number in 0..4095 (outer steps)"
 *   "a stage that is not linked has no pipe: its delay must be 0"
 * in this order, reactor by reactor.  wt_ensemble_pipe_clear turns the program off and frees the lines: the linked
 * rows stay as they are and the next feed is undelayed; no effect while none is set.  wt_ensemble_train_clear, and a
 * wt_ensemble_train_set over a program, clear the pipes first.  wt_ensemble_pipe_get gives WT_E_STATE, "no pipe
 * program is set (wt_ensemble_pipe_set)", while none is.  Not modelled: a dead time that follows the flow (V / Q),
 * dispersion or lag along the pipe.  All calls synchronise. */
#define WT_PIPE_MAX_DELAY 4095
enum { WT_PS_N_SENT = 0, WT_PS_T_SENT = 1, WT_NPS = 2 };
int wt_ensemble_pipe_set(wt_ensemble *h, const double *delay /* [N] */);
/* slots: the largest delay + 1; delay: host [N]; state: host [WT_NPS][N]; lines: host [slots - 1][4][N], the samples in
 * flight of every line (pH, Cl, T, time stamp), oldest first, NaN beyond a line's own D (any may be NULL) */
int wt_ensemble_pipe_get(wt_ensemble *h, int *slots, double *delay, double *state, double *lines);
int wt_ensemble_pipe_clear(wt_ensemble *h);
/* the checks wt_ensemble_pipe_set makes on delay [N], with no handle and no device, against the link row of a
 * [WT_NTR][N] parameter block of wt_ensemble_train_set: WT_OK or WT_E_ARG with that call's message (also
 * "n_reactors must be >= 1", "NULL argument").  Makes no HIP call. */
int wt_pipe_check(int64_t n_reactors, const double *train_params, const double *delay);

/* ---- the wire program: a stage's PLC inputs wired to another stage's instruments of the same train ----
 * On top of a set train program, with plant I/O on: a wiring diagram of each train's signal cables.  Per reactor and
 * input slot i (the seven sensors, WT_N_SENSORS order) the program says where the slot's reading comes from: the
 * reactor's own instrument i (stage -1, the default), or sensor s of stage g of the same train (g in 0..length - 1;
 * g may be the reactor's own stage with another s).
 * Parameters [WT_NSENS][WT_NW][N]: stage (-1, or a whole number 0..length - 1), sensor (a whole number 0..6; not read
 * where stage is -1, but checked).
 * Where it acts.  At a PLC scan, before everything else in the scan: for every reactor that took the outer step, each
 * wired slot of the reactor's controller-side copy of the readings is replaced by the source instrument's reading and
 * fault code of this outer step.  The source is always the instrument's own output, what the sensor suite left before
 * any wire or tamper: wires do not chain (a source slot that is itself wired still gives its own instrument), and a
 * spoof in the source stage's own image does not travel down the wire.
 * What sees the wired value: everything downstream in the scan, in the existing order -- the receiving reactor's
 * injection program (a spoof of the remote analyser is an injection at the receiver's slot), update_modbus_inputs
 * (the receiver's input registers show the remote value), the PI loops, the IMAGE slots of alarms and detectors, the
 * trend recorder's image tags.
 * What does not change: FIELD slots of alarms, detectors and trends, wt_ensemble_sensors_get and the sensor history
 * stay the reactor's own instrument.
 * A source that did not step.  If the source reactor did not take the outer step (frozen, or ended T_RANGE_POST), the
 * slot reads NaN with fault code 1 (open circuit), a dead current loop: PI loops on it hold, its image word reads 0.0
 * and the system status reads faulted.
 * State [WT_NSENS][WT_NWS][N]: n_routed (scans that delivered the source's reading), n_lost (scans that found the
 * source stopped); both 0 at set, and again after wt_ensemble_set_state; 0 in slots that are not wired.
 * Definition (the fused call gives its bits): on a handle without the program, calls of one scan interval; after each
 * the host routes wt_ensemble_sensors_get as above and runs the scan programs on the result as a host master.
 * wt_ensemble_wire_set replaces any wire program.  Refused with WT_E_STATE:
 *   "no train program is set (wt_ensemble_train_set)"
 *   "wires carry readings into the plant I/O scan: enable plant I/O first"
 * and with WT_E_ARG:
 *   "wire parameters must be finite"
 *   "stage must be -1 (the reactor's own instrument) or a whole number in 0..length - 1 (a stage of the same train)"
 *   "a wire's sensor must be a whole number in 0..6"
 * in this order: reactor by reactor, and at one reactor rule by rule over its seven slots, so the message of a block
 * with several faults does not depend on the slots they sit in.  wt_ensemble_wire_clear turns the program off: every
 * slot is the reactor's own instrument again; no effect while none is set.  wt_ensemble_train_clear, and a
 * wt_ensemble_train_set over a program, clear the wires first.  wt_ensemble_wire_get gives WT_E_STATE, "no wire program
 * is set (wt_ensemble_wire_set)", while none is.  The program takes no code of wt_program_check: wt_wire_check is its
 * check.  Not modelled: wires between trains or without a train program, signal lag or dead time on the wire (the
 * sensors' own sample lines exist already), FIELD slots that follow a wire, and the n > 32 kernel, where no train
 * fits.  All calls synchronise. */
#define WT_NSENS WT_N_SENSORS
enum { WT_W_STAGE = 0, WT_W_SENSOR = 1, WT_NW = 2 };
enum { WT_WS_N_ROUTED = 0, WT_WS_N_LOST = 1, WT_NWS = 2 };
int wt_ensemble_wire_set(wt_ensemble *h, const double *params /* [WT_NSENS][WT_NW][N] */);
/* the program in force, host [WT_NSENS][WT_NW][N] (sensor reads i where stage is -1), and the host
 * [WT_NSENS][WT_NWS][N] state (either may be NULL) */
int wt_ensemble_wire_get(wt_ensemble *h, double *params, double *state);
int wt_ensemble_wire_clear(wt_ensemble *h);
/* the checks wt_ensemble_wire_set makes on params for trains of `length` stages, with no handle and no device: WT_OK
 * or WT_E_ARG with that call's message (also "n_reactors must be >= 1", "length must be in 2..32 (the length of the
 * train program)", "NULL argument").  Makes no HIP call. */
int wt_wire_check(int length, int64_t n_reactors, const double *params);

/* ---- the junction program: flow-weighted merges and splits in a treatment train ----
 * On top of a set train program, a linked reactor may be fed by up to WT_JCT_SLOTS other stages of its own train
 * instead of stage - 1: parallel tanks merging into a clearwell, a bypass, a recycle.  A split needs nothing of its
 * own: several junctions name the same source, each with the share of its flow they take.
 * Parameters [WT_JCT_SLOTS][WT_NJ][N]: per source slot the stage g (-1: the slot is unused; else a whole number in
 * 0..length - 1, not the reactor's own stage, each stage in one slot at most) and the share f in (0, 1] of that
 * stage's inlet flow; and carry [N], 0 or 1.  A reactor with at least one used slot is a junction: its slots replace
 * the default upstream r - 1 (which may be one of them).  It must be a reactor the train program links, and it uses
 * that program's rows mask.  g may be a later stage (a recycle): a feed reads the states after the outer step and the
 * fed rows are a zero-order hold, so the order of the stages does not matter.  A linked reactor without a used slot
 * is fed by r - 1 as without the program, with the same stores and the same bits.
 * Blend of the sources k = 0..m-1, in slot order, in fp64 with every product and sum rounded (no fused multiply-add)
 * and IEEE division:
 *   Q_k = f_k * row 0 of source k (its own inlet flow, as in force during the outer step just taken),
 *   Qs = ((Q_0 + Q_1) + Q_2) + Q_3 (sums start from 0.0);
 *   m = 1: the sample is the source's outlet zone (pH, Cl, T), unchanged -- a chain written as junctions gives the
 *          train program's bits;
 *   m >= 2: Cl = (sum Q_k Cl_k) / Qs, T = (sum Q_k T_k) / Qs, pH = -log10((sum Q_k 10^(-pH_k)) / Qs), 10^x the
 *          library's own (the one that turns the inlet pH into H+), log10 the device library's; then pH is clamped to
 *          [0, 14], T to [0, 100], Cl to >= 0 (the clamps of the disturbance program's rows 1..3).
 * Every inlet term of the reference's right-hand side is Q / V (x_inlet - x_0) with H+ = 10^-pH (reactor.py:361-420),
 * so this is exact where the tank's inlet flow is the sum of the streams, which `carry` provides.  The sample's time
 * stamp is the first used slot's source time.
 * Feed inside a step.  After an outer step a junction is fed if and only if every source is live (it stepped and did
 * not end T_RANGE_POST, the train program's test) and Qs > 0; otherwise it keeps its rows.  The sample goes through
 * the reactor's pipe line if it has one (the line carries blended samples), then into rows 1 / 2 / 3 as the rows mask
 * says.  With carry = 1, row 0 of the junction becomes Qs.  All reads of row 0 and of source states of one outer step
 * precede every store of that step (a source may itself be a carrying junction).  n_fed and t_last of the train program keep their meaning (t_last: the
 * sample's time stamp).
 * State [WT_NJS][N]: n_blend (feeds a junction got inside step calls), n_held (outer steps in which at least one
 * source was live but nothing was fed), q_last (Qs of the last feed, NaN before the first); 0, 0, NaN elsewhere.
 * Definition (the fused call gives its bits in chlorine, temperature, flows, counters and stamps; a blended pH within
 * 2e-14 of a host that uses its own exp10 and log10): the train program's host loop, with the row 0 read before the
 * step and every junction's rows (and carried row 0) computed from the state after it before any is written.
 * Outside a step.  wt_ensemble_junction_set writes the base back into every linked row and then feeds; the feeds of
 * wt_ensemble_train_set, wt_ensemble_set_state, wt_ensemble_set_boundary and this one blend every junction from the
 * state and the row 0 in memory, whether or not the sources are live; Qs = 0 (or less) leaves the junction's rows as
 * they are; these feeds are not counted.  wt_ensemble_set_boundary stores row 0 as the base of the carriers, as it
 * stores rows 1..3.  wt_ensemble_junction_clear, and a set over a program, write the bases back first (rows 1..3 of
 * the rows mask, row 0 of the carriers); clear then feeds every link as the train program does.
 * With other programs.  wt_ensemble_junction_set needs a train program (WT_E_STATE, "no train program is set
 * (wt_ensemble_train_set)") and replaces any junction program.  set and clear give WT_E_STATE while a pipe program is
 * set: "junctions must be set before the pipes (a line holds what its junction delivered)".  wt_ensemble_pipe_set
 * over junctions fills a junction's line with D copies of the blend from memory (Qs = 0: of the first used slot's
 * outlet).  wt_ensemble_train_clear, and a wt_ensemble_train_set over a program, clear the junctions first.  A carried
 * flow and plant I/O exclude each other, whichever comes second (WT_E_STATE): "a carried flow cannot be combined with
 * plant I/O (the scan's command path writes row 0 in the same outer step)".  The disturbance program never targets
 * row 0 (wt_program_check refuses the row), so it and a carried flow cannot meet; its slots on rows 1..3 of a junction
 * fall under the train program's refusal.  Wires, placement and the queue are untouched.  Checkpoints, copies and
 * marks carry the program.
 * Refused with WT_E_ARG, reactor by reactor, at one reactor in this order:
 *   "a source's stage must be -1 (the slot is unused) or a whole number in 0..length - 1 (a stage of the same train)"
 *   "a junction cannot be its own source"
 *   "a stage can be a source of a junction once only"
 *   "a source's share must be finite and in (0, 1]"
 *   "a junction needs a linked reactor (the train program's link; a first stage has none)"
 *   "carry must be 0 or 1"
 *   "carry needs a junction: a reactor without a used slot carries no flow"
 * get and params give WT_E_STATE, "no junction program is set (wt_ensemble_junction_set)", while none is.  The program
 * takes no code of wt_program_check: wt_junction_check is its check.  Not modelled: raw water as a blend partner at a
 * first stage, junctions across trains, more than four sources, buffered (alkalinity-aware) pH mixing, a dead time
 * that follows the flow.  All calls synchronise. */
#define WT_JCT_SLOTS 4
enum { WT_J_STAGE = 0, WT_J_SHARE = 1, WT_NJ = 2 };
enum { WT_JS_N_BLEND = 0, WT_JS_N_HELD = 1, WT_JS_Q_LAST = 2, WT_NJS = 3 };
int wt_ensemble_junction_set(wt_ensemble *h, const double *params /* [WT_JCT_SLOTS][WT_NJ][N] */, const double *carry /* [N] */);
/* the host [WT_NJS][N] state */
int wt_ensemble_junction_get(wt_ensemble *h, double *state);
/* the program in force: host [WT_JCT_SLOTS][WT_NJ][N] (an unused slot reads stage -1, share 0) and carry [N] */
int wt_ensemble_junction_params(wt_ensemble *h, double *params, double *carry);
int wt_ensemble_junction_clear(wt_ensemble *h);
/* the checks wt_ensemble_junction_set makes on params and carry for trains of `length` stages, with no handle and no
 * device, against the link row of a [WT_NTR][N] parameter block of wt_ensemble_train_set: WT_OK or WT_E_ARG with that
 * call's message (also "n_reactors must be >= 1", "length must be in 2..32 (the length of the train program)", "NULL
 * argument").  Makes no HIP call. */
int wt_junction_check(int length, int64_t n_reactors, const double *train_params, const double *params, const double *carry);

/* ---- the sensor service program: calibrate, clean and replace the instruments inside fused runs ----
 * The maintenance half of the reference's sensor interface, which its loop would call between two iterations:
 * BaseSensor.calibrate (base_sensor.py:701-755), pHSensor.calibrate_two_point and clean_electrode (ph_sensor.py:338-434),
 * ChlorineSensor.replace_membrane and replace_reagent (chlorine_sensor.py:486-537).  All are deterministic and draw
 * nothing.  With t the suite time (ReactorState.time minus its value at wt_ensemble_sensors_enable) and x the float32
 * reference value, an action does to its sensor what the reference call does to the fields a reading depends on:
 *   WT_SVC_CALIBRATE         cal_offset = x - current; cal_time = power_on = t; status NORMAL; fault NONE
 *   WT_SVC_TWO_POINT         reference_contamination = 0, then CALIBRATE with x = (ref + ref2) / 2
 *   WT_SVC_RINSE / _ACID_CLEAN / _PEPSIN_CLEAN   membrane_fouling *= 0.5 / 0.1 / 0.2; days_since_cleaning = 0; power_on = t
 *   WT_SVC_REPLACE_MEMBRANE  membrane_fouling = membrane_age = 0, then CALIBRATE with x = 0
 *   WT_SVC_REPLACE_REAGENT   reagent_potency = 1; light exposure = reagent age = 0, then CALIBRATE with x = 0
 * calibrate replaces the offset as the reference does (it does not accumulate): a trim is WT_SVC_REF_TRIM.
 * Reference value: WT_SVC_REF_CONSTANT x = ref; _SAMPLE x = tap + ref; _TRIM x = (tap + cal_offset) + ref, in fp64 and
 * rounded once to float32, tap being the float32 true value at the sensor's own tap (zone 0 or the last zone, or the
 * flow) and cal_offset the offset in force.
 * Program.  Up to WT_SVC_SLOTS slots per reactor, parameters [WT_SVC_SLOTS][WT_NSV][N]: enable (0 or 1), sensor (0..6,
 * WT_N_SENSORS order), action, trigger, t_first, period, count, status, delay, ref_mode, ref, ref2.  Slot state
 * [WT_SVC_SLOTS][WT_NSVS][N]: n_done, t_last, t_due, t_seen; at set and reset 0, NaN, t_first, NaN.  After every read
 * of a reactor that stepped (a read that ended in WARMING_UP or POWER_FAULT included), at the read's suite time t and
 * with s the status that read returned, the enabled slots are walked in ascending order, in fp64 without fused
 * multiply-adds:
 *   if count > 0 and n_done >= count: nothing;
 *   AT_TIME:   due = t >= t_due
 *   ON_STATUS: if t_seen is NaN and s == status: t_seen = t;   due = t - t_seen >= delay   (NaN: not due; the order
 *              stands even if the status clears)
 *   if due: the action is applied (a later slot of the same sensor sees its result), n_done += 1, t_last = t, and
 *     AT_TIME:   t_due = period > 0 ? t_due + (floor((t - t_due) / period) + 1) * period, plus period once more if
 *                that is not > t : +inf          ON_STATUS: t_seen = NaN
 * A service acts on the next read, never on the one just taken: the bits of a host that makes one-step calls and calls
 * wt_ensemble_sensors_service in between.  Needs the sensor suite and n <= 32 zones (WT_E_STATE: "the sensor suite is
 * not enabled (wt_ensemble_sensors_enable)", "service programs run in the kernels for up to 32 zones"), not plant I/O.
 * set replaces any program; reset puts the slot state back to its set-time values; get, params and reset give
 * WT_E_STATE, "no service program is set (wt_ensemble_service_set)", while none is.  wt_ensemble_sensors_enable starts
 * without a program.  Checkpoints, copies and marks carry the program.  The program takes no code of wt_program_check:
 * wt_service_check is its check, with no handle and no device.  Refused with WT_E_ARG, slot by slot over the reactors, at
 * one slot and reactor in this order ("n_reactors must be >= 1" and "NULL argument" before them):
 *   "enable must be 0 or 1"                                     (a slot with enable 0 is not looked at further)
 *   "sensor must be an integer in 0..6"
 *   "action must be an integer in 0..6"
 *   "trigger must be 0 (at_time) or 1 (on_status)"
 *   "ref_mode must be 0 (constant), 1 (sample) or 2 (trim)"
 *   "two-point calibration and cleaning are for the pH sensors (0, 1)"
 *   "only the amperometric chlorine sensor (2) has a membrane to replace"
 *   "only the DPD chlorine sensor (3) has a reagent to replace"
 *   "a two-point calibration takes its buffers as constants (ref_mode 0)"
 *   "t_first, period and delay must be finite and >= 0"
 *   "period must be 0 (once) or at least 0.001 s"
 *   "count must be a whole number >= 0 (0: no cap)"
 *   "status must be an integer in 0..11 (a SensorStatus code)"
 *   "ref and ref2 must be finite"
 * Immediate service.  wt_ensemble_sensors_service applies one action now to one sensor of every reactor with
 * mask[r] != 0 (NULL: all), at t = ReactorState.time - the enable time and with the taps of the stored state: for a
 * reactor that has just stepped, what the fused read used.  ref / ref2: host [N] or NULL for 0.  Any zone count; the
 * action, sensor and ref_mode rules above apply (WT_E_ARG).  wt_ensemble_sensors_health downloads what the reference's
 * maintenance decisions look at, [WT_N_SENSORS][WT_NSH][N]: cal_offset, cal_time, power_on, the three slow ageing
 * fields of the sensor's kind (pH: fouling, days since cleaning, reference contamination; amperometric: fouling,
 * membrane age; DPD: potency, light hours, reagent age; flow: electrode fouling), status and fault of the instrument.
 * All calls synchronise. */
#define WT_SVC_SLOTS 4
enum {
    WT_SVC_CALIBRATE = 0, WT_SVC_TWO_POINT = 1, WT_SVC_RINSE = 2, WT_SVC_ACID_CLEAN = 3, WT_SVC_PEPSIN_CLEAN = 4,
    WT_SVC_REPLACE_MEMBRANE = 5, WT_SVC_REPLACE_REAGENT = 6
};
enum { WT_SVC_AT_TIME = 0, WT_SVC_ON_STATUS = 1 };
enum { WT_SVC_REF_CONSTANT = 0, WT_SVC_REF_SAMPLE = 1, WT_SVC_REF_TRIM = 2 };
enum {
    WT_SV_ENABLE = 0, WT_SV_SENSOR = 1, WT_SV_ACTION = 2, WT_SV_TRIGGER = 3, WT_SV_T_FIRST = 4, WT_SV_PERIOD = 5,
    WT_SV_COUNT = 6, WT_SV_STATUS = 7, WT_SV_DELAY = 8, WT_SV_REF_MODE = 9, WT_SV_REF = 10, WT_SV_REF2 = 11,
    WT_NSV = 12
};
enum { WT_SVS_N_DONE = 0, WT_SVS_T_LAST = 1, WT_SVS_T_DUE = 2, WT_SVS_T_SEEN = 3, WT_NSVS = 4 };
enum {
    WT_SH_CAL_OFFSET = 0, WT_SH_CAL_TIME = 1, WT_SH_POWER_ON = 2, WT_SH_SLOW0 = 3, WT_SH_SLOW1 = 4, WT_SH_SLOW2 = 5,
    WT_SH_STATUS = 6, WT_SH_FAULT = 7,
    WT_NSH = 8
};
int wt_ensemble_service_set(wt_ensemble *h, const double *params /* [WT_SVC_SLOTS][WT_NSV][N] */);
/* host [WT_SVC_SLOTS][WT_NSVS][N] slot state */
int wt_ensemble_service_get(wt_ensemble *h, double *state);
/* the program in force as set took it: host [WT_SVC_SLOTS][WT_NSV][N] */
int wt_ensemble_service_params(wt_ensemble *h, double *params);
int wt_ensemble_service_reset(wt_ensemble *h);
/* program off (no effect while none is set); what the services did to the sensors stays */
int wt_ensemble_service_clear(wt_ensemble *h);
int wt_service_check(int64_t n_reactors, const double *params);
int wt_ensemble_sensors_service(wt_ensemble *h, int sensor, int action, int ref_mode, const double *ref /* [N] or NULL */,
                                const double *ref2 /* [N] or NULL */, const uint8_t *mask /* [N] or NULL */);
int wt_ensemble_sensors_health(wt_ensemble *h, double *out /* [WT_N_SENSORS][WT_NSH][N] */);

/* ---- the installation of the sensor suite: sample lines and instrument installation per reactor ----
 * create_realistic_sensor_suite (sensors/__init__.py:41-120) builds one fixed installation: two 250 mL sample lines at
 * 500 mL/min (30 s of dead time; the pH electrode and the RTD of the inlet share one, those of the outlet the other)
 * and one InstallationQuality for all seven sensors: 0.5 m/s, no bubbles, grounding 0.9, vibration 0.1 g, ambient
 * 30 degC.  That is what a handle computes while no installation is set.  An installation gives every reactor its
 * own, [WT_NINS][N]: the two lines' volume [mL] and flow [mL/min], flow_velocity [m/s], air_bubble_frequency
 * [1/min], grounding_quality, pipe_vibration_g, ambient_temperature [degC].  From the next read on:
 *   line delay     (volume / 1000) / (flow / 1000 / 60) in fp64, 0 for a flow of 0 (base_sensor.py:167-171); both
 *                  sensors of the line look for the sample closest to t - delay in the line's 100 entries
 *   effects        between lag and rate of change (base_sensor.py:464-507), one draw each in this order:
 *                  flow_velocity < 0.1: normal(2 precision); air_bubble_frequency > 0: uniform() < frequency / 60
 *                  makes the value NaN and ends the effects; grounding_quality < 0.8: normal(precision (2 -
 *                  grounding)); pipe_vibration_g > 0.2: normal(vibration precision).  The NaN stays in the sensor's
 *                  lag, as in the reference: such a sensor reads NaN from then on (and goes on drawing).
 *   ageing         flow_velocity < 0.1: pH mineral scaling 100 * 0.0001 per day in place of 100 * 0.00001
 *                  (ph_sensor.py:203-206), amperometric fouling 0.05 per day in place of 0.01 (chlorine_sensor.py:335-338)
 *   flowmeter      air_bubble_frequency > 0: after its noise draw one more uniform(); below frequency / 60 the reading
 *                  is 0.0 for this read (flow_sensor.py:150-159)
 *   RTD            stem error 0.01 (T - ambient_temperature) (temperature_sensor.py:126)
 * The three thresholds are decided on the doubles as given.  SampleLine.ambient_temp reaches no reading in the
 * reference (base_sensor.py:611-614 drops the cooled temperature) and has no field.  Needs the sensor suite (WT_E_STATE,
 * "the sensor suite is not enabled (wt_ensemble_sensors_enable)"), any zone count, not plant I/O.  set replaces the
 * installation in force, mid-run too: the lines keep their samples and only the delay changes.  get returns the block in
 * force, the defaults while none is set.  clear goes back to the suite's build (no effect without a suite).  A block
 * of defaults and no installation give the same bits.  wt_ensemble_sensors_enable starts without one; checkpoints,
 * copies and marks carry it.  wt_install_check is the check of a block, with no handle and no device.  Refused with
 * WT_E_ARG, reactor by reactor, the message naming the field and the reactor ("grounding_quality must be in 0..1
 * (reactor 3)"), at one reactor in this order ("n_reactors must be >= 1" and "NULL argument" before them):
 *   "<field> must be finite"                           every field
 *   "<field> must be >= 0"                             the lines' volumes and flows
 *   "<line>_line_volume_mL and flow give a delay of 91 s or more: the reference's buffer grows beyond 100 entries
 *    (int(delay) + 10 > 100), the device's ring does not"      (base_sensor.py:174)
 *   "flow_velocity must be in 0..5 m/s", "air_bubble_frequency must be >= 0", "grounding_quality must be in 0..1",
 *   "pipe_vibration_g must be >= 0"                    (InstallationQuality.validate, base_sensor.py:138-145)
 * All calls synchronise. */
enum {
    WT_INS_LINE_VOLUME_INLET = 0, WT_INS_LINE_FLOW_INLET = 1, WT_INS_LINE_VOLUME_OUTLET = 2, WT_INS_LINE_FLOW_OUTLET = 3,
    WT_INS_FLOW_VELOCITY = 4, WT_INS_AIR_BUBBLE_FREQUENCY = 5, WT_INS_GROUNDING_QUALITY = 6, WT_INS_PIPE_VIBRATION_G = 7,
    WT_INS_AMBIENT_TEMPERATURE = 8,
    WT_NINS = 9
};
int wt_ensemble_install_set(wt_ensemble *h, const double *params /* [WT_NINS][N] */);
/* the installation in force: host [WT_NINS][N] */
int wt_ensemble_install_get(wt_ensemble *h, double *params);
int wt_ensemble_install_clear(wt_ensemble *h);
int wt_install_check(int64_t n_reactors, const double *params);

/* ---- the tune program: a relay (Astrom-Hagglund) autotuner per PI loop inside fused runs ----
 * The reference's roadmap lists "Control tuning utilities (Ziegler-Nichols, Lambda)"; it has none.  Two tuners per
 * reactor, one per PI loop, with the loop indices and holding words of the PI programs: loop 0 chlorine (words 2-3),
 * loop 1 acid (words 0-1).  A tuner replaces the controller by a relay with hysteresis around the setpoint, lets the
 * loop settle into its limit cycle, reads the ultimate period Pu and the amplitude a, takes Ku = 4 d / (pi sqrt(a^2 -
 * eps^2)) and applies a tuning rule given as two factors: kp = kp_factor * Ku, ki = kp / (ti_factor * Pu).
 * Parameters [WT_TUN_LOOPS][WT_NU][N]: enable (0 or 1), sensor (0..6, WT_N_SENSORS order), direction (+1 or -1),
 * setpoint, bias (the relay's centre), amplitude d, hysteresis eps, t_start (loop time at which the experiment begins),
 * t_max (time allowed from the first running scan), settle (whole cycles discarded), cycles (whole cycles measured),
 * kp_factor, ti_factor (0: ki = 0), commission (0 or 1).  State [WT_TUN_LOOPS][WT_NUS][N]: phase (WT_TUN_WAITING,
 * _RUNNING, _DONE, _FAILED), relay (-1, 0, +1), output, n_up, t_up, e_max, e_min, sum_period, sum_amp, n_cycles, period,
 * amplitude, ku, kp, ki, t_begin, t_done, n_exec, n_held, commissioned; all 0 at set and reset.
 * One scan, for a reactor that stepped and an enabled loop, immediately before the PI programs and with their inputs
 * (v = the scan's possibly tampered reading of the sensor, f = its fault code, t = the loop time the scan stores),
 * without fused multiply-adds, the divisions and the square root correctly rounded:
 *   phase >= 2: nothing.  phase 0 and t < t_start: nothing.  phase 0 and t >= t_start: phase = 1, t_begin = t,
 *   relay = 0, output = bias, e_max = -inf, e_min = +inf, words written; then as a running scan:
 *   the tuner owns the loop: the PI program skips it in this scan (no state change, no word; its t_prev advances);
 *   hold when v is not finite or f != 0: n_held += 1, relay and output stay, nothing more is written; otherwise
 *   e = direction * (setpoint - (double)v);  n_exec += 1;  if (relay == 0) relay = e >= 0 ? +1 : -1;
 *   e_max = fmax(e_max, e);  e_min = fmin(e_min, e);
 *   if (relay < 0 && e > eps) { relay = +1; up-switch } else if (relay > 0 && e < -eps) relay = -1;
 *   up-switch: n_up += 1; if (n_up >= 2 && n_up - 1 > settle) { sum_period += t - t_up; sum_amp += (e_max - e_min) * 0.5;
 *              n_cycles += 1; }  t_up = t; e_max = -inf; e_min = +inf;
 *   if (n_cycles == cycles) finish; else { output = bias + relay * d; words written }
 *   finish: period = sum_period / n_cycles; amplitude = sum_amp / n_cycles; arg = amplitude * amplitude - eps * eps;
 *           !(arg > 0): phase = 3; otherwise ku = (4.0 * d) / (3.141592653589793 * sqrt(arg)); kp = kp_factor * ku;
 *           ki = ti_factor > 0 ? kp / (ti_factor * period) : 0; phase = 2.  Both: t_done = t, output = bias, words written.
 *   time-out, after a held or an executed scan that left phase 1: t - t_begin >= t_max: phase = 3, t_done = t,
 *           output = bias, words written.
 * The words are float32(output) (high, low), as the PI's.  Commissioning, at the finish with phase 2, commission 1,
 * the control program on and this reactor's PI loop enabled: kp and ki go into the PI loop's parameter record on the
 * device, the PI's integral becomes bias - pi_bias, commissioned = 1; the PI resumes at the next scan from the relay's
 * centre output with the gains found.  Without it the PI resumes as it was.  Needs plant I/O (WT_E_STATE, "tuners act
 * on the plant I/O scan: enable plant I/O first") and n <= 32 zones ("tune programs run in the kernels for up to 32
 * zones"); runs with or without the control program.  set replaces any program and zeroes the state; reset zeroes the
 * state, so an experiment whose t_start has passed begins again at the next scan, and commissioned PI gains stay;
 * clear switches the program off and leaves the holding words as they are.  get, params and reset give WT_E_STATE,
 * "no tune program is set (wt_ensemble_tune_set)", while none is.  wt_ensemble_plc_enable starts without a program;
 * checkpoints carry it with plant I/O.  All synchronise.
 * wt_tune_check is its check, with no handle and no device.  Refused with WT_E_ARG, loop by loop over the reactors, at
 * the first of: "enable must be 0 or 1"; then for an enabled loop "sensor must be an integer in 0..6"; "direction must
 * be +1 or -1"; "setpoint and bias must be finite"; "amplitude must be finite and > 0"; "bias - amplitude must be >= 0
 * and bias + amplitude at most the loop's command limit (1.0 chlorine, 2.0 acid)"; "hysteresis must be finite and >= 0";
 * "t_start must be finite"; "t_max must be > 0 (+inf: no time-out)"; "settle must be a whole number >= 0"; "cycles must
 * be an integer in 1..4096"; "kp_factor and ti_factor must be finite and >= 0"; "commission must be 0 or 1". */
#define WT_TUN_LOOPS 2
#define WT_TUN_MAX_CYCLES 4096
enum {
    WT_TUN_ENABLE = 0, WT_TUN_SENSOR = 1, WT_TUN_DIRECTION = 2, WT_TUN_SETPOINT = 3, WT_TUN_BIAS = 4, WT_TUN_AMPLITUDE = 5,
    WT_TUN_HYSTERESIS = 6, WT_TUN_T_START = 7, WT_TUN_T_MAX = 8, WT_TUN_SETTLE = 9, WT_TUN_CYCLES = 10, WT_TUN_KP_FACTOR = 11,
    WT_TUN_TI_FACTOR = 12, WT_TUN_COMMISSION = 13,
    WT_NU = 14
};
enum {
    WT_TUNS_PHASE = 0, WT_TUNS_RELAY = 1, WT_TUNS_OUTPUT = 2, WT_TUNS_N_UP = 3, WT_TUNS_T_UP = 4, WT_TUNS_E_MAX = 5,
    WT_TUNS_E_MIN = 6, WT_TUNS_SUM_PERIOD = 7, WT_TUNS_SUM_AMP = 8, WT_TUNS_N_CYCLES = 9, WT_TUNS_PERIOD = 10,
    WT_TUNS_AMPLITUDE = 11, WT_TUNS_KU = 12, WT_TUNS_KP = 13, WT_TUNS_KI = 14, WT_TUNS_T_BEGIN = 15, WT_TUNS_T_DONE = 16,
    WT_TUNS_N_EXEC = 17, WT_TUNS_N_HELD = 18, WT_TUNS_COMMISSIONED = 19,
    WT_NUS = 20
};
enum { WT_TUN_WAITING = 0, WT_TUN_RUNNING = 1, WT_TUN_DONE = 2, WT_TUN_FAILED = 3 };
int wt_ensemble_tune_set(wt_ensemble *h, const double *params /* [WT_TUN_LOOPS][WT_NU][N] */);
/* host [WT_TUN_LOOPS][WT_NUS][N] loop state */
int wt_ensemble_tune_get(wt_ensemble *h, double *state);
/* the program in force as set took it: host [WT_TUN_LOOPS][WT_NU][N] */
int wt_ensemble_tune_params(wt_ensemble *h, double *params);
int wt_ensemble_tune_reset(wt_ensemble *h);
/* program off (no effect while none is set); holding words and commissioned gains stay */
int wt_ensemble_tune_clear(wt_ensemble *h);
int wt_tune_check(int64_t n_reactors, const double *params);

/* ---- model predictive control: a dynamic matrix controller (DMC) per dosing loop inside fused runs ----
 * The reference's roadmap lists an "MPC controller module"; it has none.  Two controllers per reactor, one per dosing
 * loop, with the loop indices and holding words of the PI programs: loop 0 chlorine (words 2-3), loop 1 acid (words
 * 0-1).  A controller carries a per-reactor step-response model and a prediction of the reading over the next WT_MPC_H
 * = 64 controller periods, so the dead time of sample lines, pipes and wires is inside its model.  It is not a program
 * of wt_program_check: it has calls of its own, as the installation has.
 * Parameters [WT_MPC_LOOPS][WT_NM][N]: enable (0 or 1), sensor (0..6, WT_N_SENSORS order), setpoint, every (controller
 * period in scans, a whole number >= 1), horizon p (a whole number in 1..64), u0 (output before the first move),
 * out_min, out_max, du_max (largest move, > 0, +inf: none), t_start (loop time from which the controller has the loop).
 * Model: step [WT_MPC_LOOPS][WT_MPC_H][N], entry i the change of the reading i + 1 controller periods after a unit move
 * of the output (the sign carries the direction: an acid step response is negative), and gain
 * [WT_MPC_LOOPS][WT_MPC_H][N], the row the predicted errors are weighted with; entries at and after p are ignored.
 * State [WT_MPC_LOOPS][WT_NMS][N]: phase (WT_MPC_WAITING, _RUNNING), output, count, bias, move, t_exec, ise, iae, dose,
 * n_exec, n_held, n_sat, n_rate, n_skipped; and the prediction pred [WT_MPC_LOOPS][WT_MPC_H][N]; all 0 at set and reset.
 * One scan, for a reactor that stepped and an enabled loop with t >= t_start, after the tune program and before the PI
 * programs and with their inputs (v = the scan's possibly tampered reading of the sensor, a float32 widened to fp64,
 * f = its fault code, t = the loop time the scan stores), in fp64 without fused multiply-adds:
 *   the tune program owned the loop in this scan: n_skipped += 1, nothing else.  Otherwise
 *   the controller owns the loop: the PI program skips it in this scan (no state change, no word; its t_prev advances),
 *   on scans that are not due as well.  The scan is due when count == 0.
 *   due, and v not finite or f != 0: n_held += 1; if (phase == 1) pred[i] = pred[min(i + 1, 63)] for all i; no move, no
 *   word.  due otherwise:
 *     1. if (phase == 0) { pred[i] = v for all i; output = fmin(fmax(u0, out_min), out_max); phase = 1; }
 *     2. d = v - pred[0];
 *     3. s[i] = pred[min(i + 1, 63)];
 *     4. term[i] = i < p ? gain[i] * ((setpoint - s[i]) - d) : +0.0;
 *     5. du = the balanced-tree sum of the 64 terms: for half = 32, 16, 8, 4, 2, 1: x[i] = x[i] + x[i + half], i < half;
 *     6. dc = fmin(fmax(du, -du_max), du_max);  if (dc != du) n_rate += 1;
 *     7. u = output + dc;  y = fmin(fmax(u, out_min), out_max);  if (y != u) n_sat += 1;
 *     8. move = y - output;                        (the move as applied: the anti-windup)
 *     9. pred[i] = s[i] + step[i] * move for all 64 entries;
 *    10. output = y;  bias = d;
 *    11. the loop's words = float32(y) (high, low), as the PI's;
 *    12. e = setpoint - v;  h = t - t_exec, 0 at the first execution;  ise += (e * e) * h;  iae += fabs(e) * h;
 *        dose += y * h;  t_exec = t;  n_exec += 1.
 *   Then, in every scan the controller owned and leaves with phase 1: count = count + 1 >= every ? 0 : count + 1.
 *   A waiting loop (phase 0) keeps count 0: it is due at every scan until its first valid reading.
 * Commands written act from the next scan on, like the PI's and the tuner's.  Needs plant I/O (WT_E_STATE, "model
 * predictive controllers act on the plant I/O scan: enable plant I/O first") and n <= 32 zones ("model predictive
 * controllers run in the kernels for up to 32 zones"); runs with or without the control and tune programs.  set
 * replaces any controllers and zeroes state and prediction; reset zeroes them, so every controller is waiting again,
 * and keeps the holding words; clear switches the controllers off and leaves the holding words as they are, and the PI
 * resumes.  get, prediction, params and reset give WT_E_STATE, "no model predictive controller is set
 * (wt_ensemble_mpc_set)", while none is.  wt_ensemble_plc_enable starts without one; checkpoints carry parameters,
 * model, state and prediction with plant I/O.  All synchronise.
 * wt_mpc_check is the one check of the three blocks, with no handle and no device.  Refused with WT_E_ARG, loop by loop
 * over the reactors, at the first of the following, each followed by " (loop L, reactor R)": "enable must be 0 or 1";
 * "sensor must be an integer in 0..6"; "every must be a whole number >= 1"; "horizon must be an integer in 1..64";
 * "setpoint and u0 must be finite"; "out_min and out_max must be finite and out_min <= out_max"; "du_max must be > 0
 * (+inf: no limit)"; "t_start must not be NaN"; then for an enabled loop "step and gain must be finite"; "gain must not
 * be all zero over the horizon". */
#define WT_MPC_LOOPS 2
#define WT_MPC_H 64
enum {
    WT_MPC_ENABLE = 0, WT_MPC_SENSOR = 1, WT_MPC_SETPOINT = 2, WT_MPC_EVERY = 3, WT_MPC_HORIZON = 4, WT_MPC_U0 = 5,
    WT_MPC_OUT_MIN = 6, WT_MPC_OUT_MAX = 7, WT_MPC_DU_MAX = 8, WT_MPC_T_START = 9,
    WT_NM = 10
};
enum {
    WT_MPCS_PHASE = 0, WT_MPCS_OUTPUT = 1, WT_MPCS_COUNT = 2, WT_MPCS_BIAS = 3, WT_MPCS_MOVE = 4, WT_MPCS_T_EXEC = 5,
    WT_MPCS_ISE = 6, WT_MPCS_IAE = 7, WT_MPCS_DOSE = 8, WT_MPCS_N_EXEC = 9, WT_MPCS_N_HELD = 10, WT_MPCS_N_SAT = 11,
    WT_MPCS_N_RATE = 12, WT_MPCS_N_SKIPPED = 13,
    WT_NMS = 14
};
enum { WT_MPC_WAITING = 0, WT_MPC_RUNNING = 1 };
int wt_mpc_check(int64_t n_reactors, const double *params /* [WT_MPC_LOOPS][WT_NM][N] */,
                 const double *step /* [WT_MPC_LOOPS][WT_MPC_H][N] */, const double *gain /* [WT_MPC_LOOPS][WT_MPC_H][N] */);
int wt_ensemble_mpc_set(wt_ensemble *h, const double *params, const double *step, const double *gain);
/* host [WT_MPC_LOOPS][WT_NMS][N] loop state */
int wt_ensemble_mpc_get(wt_ensemble *h, double *state);
/* host [WT_MPC_LOOPS][WT_MPC_H][N]: entry i the reading predicted i controller periods after the last execution */
int wt_ensemble_mpc_prediction(wt_ensemble *h, double *pred);
/* the controllers in force as set took them; each pointer may be NULL (not wanted) */
int wt_ensemble_mpc_params(wt_ensemble *h, double *params, double *step, double *gain);
int wt_ensemble_mpc_reset(wt_ensemble *h);
/* controllers off (no effect while none is set); the holding words stay */
int wt_ensemble_mpc_clear(wt_ensemble *h);

/* ---- response programs: the reaction to an alarm, a detection or a bad reading inside fused runs ----
 * What an operator or a safety PLC does about what the alarm and detector programs noticed: on a cause that has stood
 * for a reaction time, a slot takes a dosing loop out of automatic, holds or drives its output, and hands the loop back
 * when the cause is gone.  Up to WT_RSP_SLOTS = 4 slots per reactor, evaluated at every PLC scan of a reactor that
 * stepped, directly after the tune program and before the model predictive controllers and the PI programs, with their
 * inputs.  Loop 0 is chlorine (holding words 2-3), loop 1 acid (words 0-1).  It is not a program of wt_program_check:
 * it has calls of its own, as the model predictive controllers have.
 * Parameters [WT_RSP_SLOTS][WT_NR][N]: cause (WT_RSP_OFF, _ALARM, _DETECTOR, _BAD), index (the alarm slot, detector slot
 * or sensor the cause refers to), delay (s the cause must have stood without interruption before the slot engages; 0
 * engages on the scan that first sees it), loop, action (WT_RSP_HOLD, _MANUAL, _RAMP), value (target output of MANUAL
 * and RAMP), rate (of a RAMP, per second), latch (1: engaged until reset), clear_delay, min_hold (s), handback
 * (WT_RSP_BUMP, _BUMPLESS).
 * State [WT_RSP_SLOTS][WT_NRS][N]: phase (WT_RSP_IDLE, _ENGAGED), pending and clearing (the loop times since which the
 * cause has stood, or has been clear; NaN: none), output (the forced output), t_first, t_engaged (first and last
 * engagement), t_released (last release; NaN: never), n_engaged, time_engaged (s), n_owned, n_blocked, n_cause, n_tracked,
 * n_handback (scans and events); and per reactor [WT_NRR][N]: t_prev, owner_chlorine, owner_acid (the slot that owned the
 * loop in the last scan, -1: none).  At set and reset: counts 0, times NaN, owners -1, t_prev the loop time.
 * One scan, slot by slot from 0 to 3, in fp64 without fused multiply-adds (t: the loop time the scan stores;
 * h = t - t_prev, then t_prev = t; every slot whose cause is not OFF, l its loop):
 *   1. the cause c.  ALARM: the alarm program is on and its slot `index` is active; DETECTOR: the detector program is on
 *      and its slot `index` has its alarm set -- both as the previous scan left them, since those programs run later in
 *      the scan; BAD: this scan's image copy of sensor `index` (after any wire and injection program) is not finite or
 *      carries a fault code.  A cause whose program is off is false.  if (c) n_cause += 1.
 *   2. a slot that entered the scan engaged: time_engaged += h.  If latch == 0: if (c) clearing = NaN; else { if clearing
 *      is NaN, clearing = t; if (t - clearing >= clear_delay && t - t_engaged >= min_hold) the slot releases: phase = 0,
 *      t_released = t, clearing = NaN, then the hand-back. }
 *   3. a slot that entered the scan idle: if (!c) pending = NaN; else { if pending is NaN, pending = t;
 *      if (t - pending >= delay) the slot engages: phase = 1, pending = clearing = NaN, n_engaged += 1, t_first = t if it
 *      is NaN, t_engaged = t, output = the float32 the loop's holding words decode to (widened to fp64). }  A slot does
 *      not engage and release, or release and engage, in one scan.
 *   4. a slot that is engaged now: if the tune program owned loop l in this scan: n_blocked += 1, nothing is written;
 *      else if a lower slot owns loop l in this scan: output = that slot's output, n_tracked += 1 (a later take-over
 *      does not bump); else the slot owns the loop: HOLD y = output; MANUAL y = value; RAMP step = rate * h,
 *      d = value - output, y = d > step ? output + step : d < -step ? output - step : value; then output = y, the loop's
 *      words = float32(y) (high, low), n_owned += 1.
 *   Then owner_chlorine / owner_acid = the slot that owned the loop in this scan, -1 for none.
 * A loop a slot owns is skipped by the model predictive controllers (they count n_skipped) and by the PI programs (no
 * state change, no word) exactly like a loop a relay experiment has.  An alarm trip still replaces whatever command the
 * words decode to.  Commands written act from the next scan on.
 * The hand-back of a releasing BUMPLESS slot that owned its loop in the previous scan, where neither the tune program
 * nor a lower slot has the loop in this scan: n_handback += 1; if the control program is on and its loop l enabled,
 * integral = output - (bias + kp * e), e = direction * (setpoint - v) of this scan's reading v as the PI computes it, or
 * output - bias where that reading is not finite or faulted, so that the PI's output of this same scan continues from
 * the forced value; an enabled, running model predictive controller of loop l gets its output = output.  Every other
 * release leaves the controllers as they are.
 * Needs plant I/O (WT_E_STATE, "response programs act on the plant I/O scan: enable plant I/O first") and n <= 32 zones
 * ("response programs run in the kernels for up to 32 zones").  set replaces any program and restarts the state; reset
 * restarts it, which releases latched slots, and keeps the holding words; clear switches the program off and leaves the
 * words.  state, params and reset give WT_E_STATE, "no response program is set (wt_ensemble_respond_set)", while none
 * is.  wt_ensemble_plc_enable starts without one; checkpoints carry parameters and state with plant I/O.  All synchronise.
 * wt_respond_check is the one check of the block, with no handle and no device.  Refused with WT_E_ARG, slot by slot over
 * the reactors, at the first of the following, each followed by " (slot S, reactor R)": "cause must be 0 (off), 1
 * (alarm), 2 (detector) or 3 (bad)"; then for a slot that is not off "an ALARM cause's index must be an alarm slot in
 * 0..3"; "a DETECTOR cause's index must be a detector slot in 0..3"; "a BAD cause's index must be a sensor index in
 * 0..6"; "loop must be 0 (chlorine) or 1 (acid)"; "action must be 0 (hold), 1 (manual) or 2 (ramp)"; "latch must be 0
 * or 1"; "handback must be 0 (bump) or 1 (bumpless)"; "delay, clear_delay, min_hold and rate must be >= 0 and not NaN"
 * (+inf is allowed: a delay never reached); "value must be within 0 and the loop's command limit (1.0 chlorine, 2.0
 * acid)". */
#define WT_RSP_SLOTS 4
enum {
    WT_RSP_CAUSE = 0, WT_RSP_INDEX = 1, WT_RSP_DELAY = 2, WT_RSP_LOOP = 3, WT_RSP_ACTION = 4, WT_RSP_VALUE = 5,
    WT_RSP_RATE = 6, WT_RSP_LATCH = 7, WT_RSP_CLEAR_DELAY = 8, WT_RSP_MIN_HOLD = 9, WT_RSP_HANDBACK = 10,
    WT_NR = 11
};
enum {
    WT_RSPS_PHASE = 0, WT_RSPS_PENDING = 1, WT_RSPS_CLEARING = 2, WT_RSPS_OUTPUT = 3, WT_RSPS_T_FIRST = 4,
    WT_RSPS_T_ENGAGED = 5, WT_RSPS_T_RELEASED = 6, WT_RSPS_N_ENGAGED = 7, WT_RSPS_TIME_ENGAGED = 8, WT_RSPS_N_OWNED = 9,
    WT_RSPS_N_BLOCKED = 10, WT_RSPS_N_CAUSE = 11, WT_RSPS_N_TRACKED = 12, WT_RSPS_N_HANDBACK = 13,
    WT_NRS = 14
};
enum { WT_RSPR_T_PREV = 0, WT_RSPR_OWNER_CHLORINE = 1, WT_RSPR_OWNER_ACID = 2, WT_NRR = 3 };
enum { WT_RSP_OFF = 0, WT_RSP_ALARM = 1, WT_RSP_DETECTOR = 2, WT_RSP_BAD = 3 };
enum { WT_RSP_HOLD = 0, WT_RSP_MANUAL = 1, WT_RSP_RAMP = 2 };
enum { WT_RSP_BUMP = 0, WT_RSP_BUMPLESS = 1 };
enum { WT_RSP_IDLE = 0, WT_RSP_ENGAGED = 1 };
int wt_respond_check(int64_t n_reactors, const double *params /* [WT_RSP_SLOTS][WT_NR][N] */);
int wt_ensemble_respond_set(wt_ensemble *h, const double *params);
/* host [WT_RSP_SLOTS][WT_NRS][N] slot state and [WT_NRR][N] reactor state; each pointer may be NULL (not wanted) */
int wt_ensemble_respond_state(wt_ensemble *h, double *state, double *reactor_state);
/* host [WT_RSP_SLOTS][WT_NR][N]: the program in force as set took it */
int wt_ensemble_respond_params(wt_ensemble *h, double *params);
int wt_ensemble_respond_reset(wt_ensemble *h);
/* program off (no effect while none is set); the holding words stay */
int wt_ensemble_respond_clear(wt_ensemble *h);

/* ---- link programs: delay, loss and replay on the plant's I/O inside fused runs ----
 * What the fieldbus between the plant and its controller does to a signal in time.  Up to WT_LNK_SLOTS = 4 slots per
 * reactor; a slot sits on one channel -- the injection program's targets with its codes: the seven readings 0..6,
 * acid_flow_rate 7, chlorine_flow_rate 8, inlet_flow_rate 9 -- keeps a ring of the channel's last WT_LNK_DEPTH = 64
 * samples and decides at every PLC scan of a reactor that stepped what the receiving end gets.  Reading slots act on
 * the scan's copy of the readings after the wire program and directly before the injection program's sensor slots: the
 * input image, the controllers, IMAGE slots of alarms and detectors and the trend tags see the linked value, FIELD slots
 * and wt_ensemble_sensors_get keep the instrument's own.  Command slots act on the three float32 commands decoded from
 * the holding words, before the injection program's command slots and the validation; the holding image is not touched.
 * Slots run in slot order; two slots on one channel chain.  It is not a program of wt_program_check: it has calls of
 * its own, as the response programs have.
 * Parameters [WT_LNK_SLOTS][WT_NL][N]: mode (WT_LNK_OFF, _DELAY, _LOSS, _REPLAY), target, start, end (the window
 * start <= t < end in loop time, t the loop time the scan stores: the injection program's), a, b, timeout, fail.
 * Defaults: end = +inf, timeout = +inf, the others 0.
 * State [WT_LNK_SLOTS][WT_NLS][N]: n_rec (samples recorded), n_applied (in-window scans), n_fresh, n_lost, n_timeout,
 * n_draw, t_fresh (loop time of the last fresh delivery), held_value, held_fault (the last fresh delivery), tape_end
 * (n_rec when the replay window opened; NaN outside one).  At set and reset: t_fresh, held_value and tape_end NaN,
 * held_fault and the counts 0, the rings empty.
 * One scan of one slot on the sample (x, f) of its channel, x a float32 and f its fault code (0 for a command), counts
 * in fp64:
 *   1. record: ring[n_rec % 64] = (x, f), n_rec += 1 -- except a REPLAY slot inside its window, whose tape must survive.
 *      Recording runs from set on, inside and outside the window, whatever the mode.
 *   2. outside the window (start <= t < end does not hold, or the mode is OFF): (x, f) passes; held = (x, f),
 *      t_fresh = t, tape_end = NaN.
 *   3. inside: j = n_applied, n_applied += 1, then
 *      DELAY (a scans, jitter b scans, both whole, a + b <= 63): d = a where b == 0, else a + floor(u * (b + 1)); the
 *        sample recorded d scans ago is delivered, ring[max(n_rec - 1 - d, 0) % 64] (the oldest while there are fewer);
 *        fresh.
 *      LOSS (probability a in [0, 1], timeout in s or +inf, fail): one draw u per in-window scan; the update is lost iff
 *        u < a (a = 0 never loses, a = 1 always does).  Not lost: (x, f) is delivered, fresh.  Lost: n_lost += 1; if
 *        nothing was ever delivered (t_fresh is NaN) the sample passes, fresh; else if t - t_fresh > timeout the fail
 *        state is delivered and n_timeout += 1 -- a reading becomes NaN with fault code fail (1..6), a command the
 *        value float32(fail); else held is delivered.
 *      REPLAY (a = tape length in scans, 1..63): if tape_end is NaN (the window's first scan): if n_rec == 0 this
 *        sample is recorded first; then tape_end = n_rec.  L = min(a, tape_end), at least 1; in-window scan j delivers
 *        ring[(tape_end - L + j % L) % 64]; fresh.
 *      A fresh delivery (y, g) sets held = (y, g), t_fresh = t and n_fresh += 1.
 *   u is word 0 of Philox4x32-10 on the counter (reactor_base + r, slot, n_draw, 2) with the key (seed & 0xffffffff,
 *   seed >> 32), times 2^-32 (exact in fp64); reactor_base is the sensor suite's; n_draw += 1 per draw.  DELAY without
 *   jitter, REPLAY and OFF draw nothing.
 * A count used as an index is taken as 0 unless it is a number in [0, 2^32), and every ring index is reduced modulo 64
 * on the device: no restored or edited state addresses outside the ring.  A fault code is kept in a byte.
 * Needs plant I/O (WT_E_STATE, "link programs act on the plant I/O scan: enable plant I/O first") and n <= 32 zones
 * ("link programs run in the kernels for up to 32 zones").  set replaces any program and restarts state and rings;
 * reset restarts them; clear switches the program off.  state, params, ring and reset give WT_E_STATE, "no link program
 * is set (wt_ensemble_link_set)", while none is.  wt_ensemble_plc_enable starts without one; checkpoints carry
 * parameters, seed, state and rings with plant I/O.  All synchronise.
 * wt_link_check is the one check of the block, with no handle and no device.  Refused with WT_E_ARG, slot by slot over
 * the reactors, at the first of the following, each followed by " (slot S, reactor R)": "mode must be 0 (off), 1
 * (delay), 2 (loss) or 3 (replay)"; "target must be an integer in 0..9"; "start must be finite and end a number (end may
 * be +inf)"; "start must not exceed end"; then by mode -- a field a mode does not use must be at its default --
 * OFF: "a slot that is off takes no a, b, timeout or fail"; DELAY: "a DELAY slot's delay (a) and jitter (b) must be
 * whole numbers of scans with a + b <= 63", "a DELAY slot takes no timeout or fail"; LOSS: "a LOSS slot's probability (a)
 * must be within 0 and 1", "a LOSS slot takes no b", "a LOSS slot's timeout must be >= 0 or +inf", and with timeout
 * +inf "a LOSS slot without a timeout takes no fail", else on a reading "a LOSS slot on a reading fails to a fault code
 * (fail) in 1..6", on a command "a LOSS slot on a command fails to a finite value (fail)"; REPLAY: "a REPLAY slot's tape
 * length (a) must be a whole number of scans in 1..63", "a REPLAY slot takes no b, timeout or fail". */
#define WT_LNK_SLOTS 4
#define WT_LNK_DEPTH 64
enum {
    WT_LNK_MODE = 0, WT_LNK_TARGET = 1, WT_LNK_START = 2, WT_LNK_END = 3, WT_LNK_A = 4, WT_LNK_B = 5, WT_LNK_TIMEOUT = 6,
    WT_LNK_FAIL = 7,
    WT_NL = 8
};
enum {
    WT_LNKS_N_REC = 0, WT_LNKS_N_APPLIED = 1, WT_LNKS_N_FRESH = 2, WT_LNKS_N_LOST = 3, WT_LNKS_N_TIMEOUT = 4,
    WT_LNKS_N_DRAW = 5, WT_LNKS_T_FRESH = 6, WT_LNKS_HELD_VALUE = 7, WT_LNKS_HELD_FAULT = 8, WT_LNKS_TAPE_END = 9,
    WT_NLS = 10
};
enum { WT_LNK_OFF = 0, WT_LNK_DELAY = 1, WT_LNK_LOSS = 2, WT_LNK_REPLAY = 3 };
int wt_link_check(int64_t n_reactors, const double *params /* [WT_LNK_SLOTS][WT_NL][N] */);
int wt_ensemble_link_set(wt_ensemble *h, const double *params, uint64_t seed);
/* host [WT_LNK_SLOTS][WT_NLS][N] */
int wt_ensemble_link_state(wt_ensemble *h, double *state);
/* host [WT_LNK_SLOTS][WT_NL][N]: the program in force as set took it, and its seed; each pointer may be NULL */
int wt_ensemble_link_params(wt_ensemble *h, double *params, uint64_t *seed);
/* the rings in recording order: values, faults host [WT_LNK_SLOTS][WT_LNK_DEPTH][N], entry k the k-th oldest sample a
 * ring still holds (min(n_rec, 64) of them; NaN and 0 past those), n_rec host [WT_LNK_SLOTS][N]; each may be NULL */
int wt_ensemble_link_ring(wt_ensemble *h, double *values, double *faults, double *n_rec);
int wt_ensemble_link_reset(wt_ensemble *h);
/* program off (no effect while none is set) */
int wt_ensemble_link_clear(wt_ensemble *h);

/* ---- the parameter checks of the scan programs, the disturbance and the score program, without a handle or a device ----
 * params: host, the block the program's set or enable call takes, for n_reactors reactors (WT_PROG_CONTROL:
 * wt_ensemble_control_enable / retune, WT_PROG_INJECT: wt_ensemble_inject_set, WT_PROG_ALARM: wt_ensemble_alarm_set,
 * WT_PROG_ACTUATOR: wt_ensemble_actuator_set, WT_PROG_DISTURB: wt_ensemble_disturb_set, WT_PROG_SCORE:
 * wt_ensemble_score_set, WT_PROG_DETECT: the slot block of wt_ensemble_detect_set, whose label block that call checks
 * itself, WT_PROG_TREND: wt_ensemble_trend_set, WT_PROG_SERVICE: wt_ensemble_service_set, WT_PROG_TUNE:
 * wt_ensemble_tune_set).  WT_OK when the block passes that call's checks; otherwise WT_E_ARG and wt_last_error() is the
 * message the call gives for it.  A NULL params, n_reactors < 1 or an unknown program also give WT_E_ARG.  Makes no HIP
 * call.  wt_service_check and wt_tune_check are this check under the two programs' own names: the same codes and
 * texts, but n_reactors is looked at first and a NULL params is "NULL argument". */
enum { WT_PROG_CONTROL = 0, WT_PROG_INJECT = 1, WT_PROG_ALARM = 2, WT_PROG_ACTUATOR = 3, WT_PROG_DISTURB = 4, WT_PROG_SCORE = 5,
       WT_PROG_DETECT = 6, WT_PROG_TREND = 7, WT_PROG_SERVICE = 8, WT_PROG_TUNE = 9 };
int wt_program_check(int program, const double *params, int64_t n_reactors);
/* the parameter block of a set program as its set (enable, retune) call took it, bit for bit: host, the shape
 * wt_program_check names for `program`; synchronises.  WT_E_STATE with the program's "not set" message while it is off,
 * WT_E_ARG for an unknown program. */
int wt_ensemble_program_params(wt_ensemble *h, int program, double *params);

/* ---- checkpoint, copy and rewind of a whole ensemble ----
 * A checkpoint holds everything that decides the next bits of a run: the state, the boundary block, status and solver
 * counters, the placement with its cost history, the schedule, the step limit, the sensor suite with its draw counters
 * and rings, the register images, the trajectory records, every program's parameters, state and stores, the train
 * shape with its pipes and wires, and the host counters that go with them.  It holds no developer instrumentation
 * (wave diagnostics, item trace, launch timing, the environment knobs read at creation) and no scratch; after a load
 * the instrumentation is off, and WT_INFO_BOUNDARY_UPLOADS and the re-deal count stay the destination's own.
 *
 * The blob is little-endian: the 64-byte wt_checkpoint_header below, then the handle's parts in a fixed order.  A part
 * is {uint32 tag, uint32 n_scalars, n_scalars x 8 bytes (integers as int64, doubles as they are), uint32 n_arrays,
 * uint32 0, then per array int64 bytes and the data, zero-padded to a multiple of 8}; a part that is off has
 * n_arrays = 0.  No address is ever written.  `layout` is a hash over the parts' tags, scalar kinds and the byte
 * counts of every array at the unit shape, so a library whose records differ refuses the blob.  `checksum` is the
 * 64-bit FNV-1a of every byte after the header.  Two saves of one state give the same bytes.
 *
 * size:  bytes a save of the handle as it is now needs; no synchronisation.
 * save:  synchronises; WT_E_ARG "checkpoint_save: the buffer is smaller than wt_ensemble_checkpoint_size" when
 *        bytes is too small (more is fine), WT_E_HIP when a launch has left the state incomplete.
 * check: host only, no device call.  Refusals in this order, all WT_E_ARG: "checkpoint: NULL argument",
 *        "checkpoint: shorter than its header", "checkpoint: bad magic", "checkpoint: unknown format version",
 *        "checkpoint: the header's byte count is not the blob's length", "checkpoint: the layout fingerprint is
 *        not this library's", "checkpoint: checksum mismatch", "checkpoint: n_reactors must be positive",
 *        "checkpoint: n_zones must be in 2..64", "checkpoint: a part's switches or capacities are out of range",
 *        "checkpoint: a part's arrays do not match the capacities it declares".  n_reactors / n_zones may be NULL.
 * load:  into a handle of equal N, n and reactor constants (WT_E_ARG "checkpoint_load: the checkpoint's n_reactors or
 *        n_zones differ from the handle's", "checkpoint_load: the reactor constants differ from the handle's"), on
 *        any device.  The whole blob is validated as `check` does before the first device call; a refusal changes
 *        nothing.  Then the load replaces the configuration: the destination's optional parts are released, the
 *        blob's switches and capacities take their place, the train shape is rebuilt under the destination's own
 *        packing rule, and the payload is uploaded.
 * copy:  dst becomes what load(save(src)) would make it, device to device.  Two distinct handles on one device with
 *        equal N, n and constants; otherwise WT_E_ARG ("copy: dst and src are the same handle", "copy: the handles
 *        differ in n_reactors or n_zones", "copy: the handles are on different devices", "copy: the reactor
 *        constants differ").  The mark of src is not copied.
 * mark:  a checkpoint kept in device memory inside the handle; replaces an earlier mark; freed by unmark and destroy.
 *        WT_E_HIP when the second copy cannot be allocated (the handle is untouched).
 * rewind: back to the mark, any number of times; WT_E_STATE "rewind: no mark is set (wt_ensemble_mark)".  Where the
 *        switches and capacities are those of the mark, one kernel launch and no allocation; otherwise the load path
 *        from the device-resident payload.
 * unmark: no effect without a mark. */
#define WT_CKP_MAGIC "WTCK"
#define WT_CKP_FORMAT 1
#define WT_CKP_HEADER_BYTES 64
typedef struct {
    char magic[4];                        /*  0  "WTCK" */
    uint32_t format;                      /*  4  WT_CKP_FORMAT */
    uint32_t abi;                         /*  8  WT_ABI_VERSION */
    uint32_t n_zones;                     /* 12 */
    int64_t n_reactors;                   /* 16 */
    int64_t bytes;                        /* 24  of the whole blob, header included */
    uint64_t layout;                      /* 32  layout fingerprint */
    uint64_t checksum;                    /* 40  FNV-1a 64 of bytes 64 .. bytes - 1 */
    uint32_t n_parts;                     /* 48 */
    uint32_t reserved0;                   /* 52  0 */
    uint64_t reserved1;                   /* 56  0 */
} wt_checkpoint_header;
int wt_ensemble_checkpoint_size(wt_ensemble *h, int64_t *bytes);
int wt_ensemble_checkpoint_save(wt_ensemble *h, void *blob, int64_t bytes);
int wt_ensemble_checkpoint_load(wt_ensemble *h, const void *blob, int64_t bytes);
int wt_checkpoint_check(const void *blob, int64_t bytes, int64_t *n_reactors, int *n_zones);
int wt_ensemble_copy(wt_ensemble *dst, wt_ensemble *src);
int wt_ensemble_mark(wt_ensemble *h);
int wt_ensemble_rewind(wt_ensemble *h);
int wt_ensemble_unmark(wt_ensemble *h);
/* Self-test of the kernel that performs a checkpoint's device-to-device copies (wtck::copy_table_kernel): `count`
 * arrays of bytes[i] >= 0 bytes, sources filled with a position-dependent pattern, destinations with another byte and
 * 64 guard bytes behind each; everything is compared on the host, guards included.  *mismatches must come back 0.
 * count = 0 launches nothing. */
int wt_selftest_copy_table(int device, const int64_t *bytes, int count, int *mismatches);

/* ---- reactor diagnostics (SURVEY.md section 8(f) NEXT-4): reductions over the zones of every reactor ----
 * out: host [WT_N_DIAG][N] doubles, rows
 *   0 total_chlorine_mg, 1 total_H_mol, 2 total_OH_mol, 3 charge_balance_mol, 4 thermal_energy_kJ
 *                                   IntegratedCSTR.validate_conservation (reactor.py:570-611)
 *   5 pH CV, 6 pH segregation index, 7 chlorine CV, 8 chlorine segregation index
 *                                   TransportModel.calculate_mixing_quality (transport.py:338-384, reactor.py:638-639)
 *   9 thermocline depth from the top [m], NaN where the reference returns None
 *                                   SpatialModel.identify_thermocline (spatial.py:352-379)
 *   10 + 8 p + {0 mean_value, 1 std_value, 2 max_value, 3 min_value, 4 range, 5 max_gradient, 6 mean_gradient,
 *   7 gradient_location}, p = 0 pH, 1 chlorine, 2 temperature
 *                                   SpatialModel.calculate_spatial_gradients (spatial.py:440-477)
 * evaluated on the current state (the derived H+ of the last step; call after wt_ensemble_step). */
#define WT_N_DIAG 34
int wt_ensemble_diagnostics(wt_ensemble *h, double *out);

/* Self-test of the kernel's cross-lane primitives (DPP row / wave shifts, segment
 * sums) against ds_bpermute for a given zone count; *mismatches must come back 0. */
int wt_selftest_shuffles(int device, int n_zones, int *mismatches);

/* Per-wavefront diagnostics of the LAST launch: {loop trips, trips with a Newton
 * evaluation, shader clocks, 100 MHz wall ticks, factorisation / Jacobian /
 * deferred-f block executions, spare} per wavefront.  The first call allocates the
 * buffer and switches recording on (out may be NULL); later calls copy
 * [n_waves][wt_wave_diag_slots()] int64 into `out` (8 slots; 16 in -DWT_STAMPS diagnostic builds,
 * which add the shader-clock shares of the kernel loop's sections). */
int wt_wave_diag_slots(void);
/* Developer trace of the LAST launch's work items under the queue schedule: {worker, group, first step | steps << 32,
 * start, end} in 100 MHz ticks, 5 int64 per item.  The first call allocates `capacity` items and switches tracing on. */
int wt_ensemble_item_trace(wt_ensemble *h, int64_t *out, int capacity, int *n_items);
int wt_ensemble_wave_diag(wt_ensemble *h, int64_t *out, int64_t capacity, int64_t *n_waves);

int64_t wt_ensemble_size(const wt_ensemble *h);
int wt_ensemble_zones(const wt_ensemble *h);

/* AqueousChemistry.calculate_pH (chemistry.py:271-330) batched: Newton-Raphson
 * on the charge balance, one system per element.  Host arrays of length n.
 * rc[i]: 0 converged, 1 "derivative too small" (RuntimeError), 2 no convergence. */
int wt_ph_solve(int device, int64_t n, const double *Kw, const double *Ka1, const double *Ka2,
                const double *CT_mol, const double *alk_mgL, const double *guess,
                double tol, int max_iter, double *pH_out, int32_t *iters, int32_t *rc);

#ifdef __cplusplus
}
#endif
#endif /* WTPHYS_H */
