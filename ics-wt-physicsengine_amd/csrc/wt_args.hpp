// wt_args.hpp -- the step kernel's argument block: StepArgs (filled by the host, wtphys.hip: make_args) with the
// argument structs of the sensor suite, the plant I/O, the eight per-reactor programs, the train, the wire and the tune program inside it, the words of the
// work queue's control block, which kernel instantiations carry which sections, and fresh(): how a section of a work
// item re-reads what it needs from the kernel-argument segment.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "wt_tables.hpp"
#include "wt_sensors.hpp"
#include "wt_svc.hpp"
#include "wt_ctl.hpp"
#include "wt_tun.hpp"
#include "wt_mpc.hpp"
#include "wt_inj.hpp"
#include "wt_lnk.hpp"
#include "wt_alm.hpp"
#include "wt_det.hpp"
#include "wt_rsp.hpp"
#include "wt_trd.hpp"
#include "wt_act.hpp"
#include "wt_dst.hpp"
#include "wt_scr.hpp"
#include "wt_trn.hpp"
#include "wt_wir.hpp"

namespace wt {

#ifdef WT_STAMPS
constexpr int WT_DIAG_SLOTS = 16;
#else
constexpr int WT_DIAG_SLOTS = 8;
#endif

struct StepArgs {
    int64_t N;        // reactors in the ensemble (row stride of par / bc)
    int64_t r0, r1;   // stream schedule: this launch advances reactors [r0, r1); queue schedule: [0, N)
    int n;            // zones per reactor
    int R;            // reactors per wavefront = 64 / n
    const double *par; // [WT_NP][N]
    double *bc;        // [WT_NB][N]  (rows 0, 4, 6 are rewritten by the command path when plant I/O is on)
    double *pH, *Cl, *T; // [N][n]
    double *time, *flow; // [N]
    double *dH, *dRho, *dK; // derived [N][n]
    uint32_t *status;    // [N]
    int32_t *stats;      // [N][5] or nullptr
    int64_t *wave_diag;  // [n_groups][WT_DIAG_SLOTS] or nullptr, accumulated over the work items of a launch:
                         //   trips, Newton trips, shader clocks, wall clock (100 MHz), factorize / num_jac / deferred-f block executions, items
    double *bad_T;       // [N] the temperature the reference's ValueError names (thermodynamics.py:151)
    // Placement: slot q of the wavefront-groups (group q / R, segment q % R) holds reactor perm[q].  Reactors never
    // interact, so which of them share a wavefront is free -- and a wavefront costs what its slowest reactor costs,
    // so reactors of similar solver cost are put together (wt_place.hpp re-bins them from `cost` between calls).
    const int32_t *perm;  // [N]
    int32_t *cost;        // [N] RHS evaluations since the last re-binning (the solver's nfev, summed over outer steps)
    double dt;
    int n_steps;      // outer steps this launch advances every reactor by
    int first_step;   // index of this launch's first step within the wt_ensemble_step call (PLC scan phase)
    int call_steps;   // outer steps of the whole wt_ensemble_step call
    int step_limit;   // give up an outer step after this many step attempts (0 = never, as the reference)
    // Work queue (nullptr: stream schedule -- workgroup b advances the wavefront-group r0 / R + b by n_steps).
    // q_ctrl: Q_AVAIL, Q_HEAD, Q_TAIL, Q_ERROR; q_slots[q_cap]: (ticket + 1) << 32 | group; q_next[group]: next step.
    int32_t *q_ctrl; unsigned long long *q_slots; int32_t *q_next;
    int q_cap, item_steps, n_groups;
    int64_t *trace; int trace_cap;   // optional item trace (tools/): worker, group, step0 | cnt << 32, start, end (100 MHz ticks)
    wts::SuiteArgs sens; // fused sensor suite + plant I/O (sens.on == 0: none)
    KTab kt;             // fp64 constants of the RHS sections (scalar loads)
    RTab rt;             // ... of the solver sections
    // Forcing and trajectory recording (wt_ensemble_step_scheduled / wt_ensemble_record), both handled in the cold
    // end-of-outer-step section of run_item.  x_on == 0: neither (the section is one scalar load and a branch).
    int x_on;
    const double *sched;   // [call_steps][NB][N]: row gs is the boundary of outer step gs of the call; nullptr: bc
    double *rec_pH, *rec_Cl, *rec_T;   // [rec_cap][N][n], nullptr: not recording in this call
    double *rec_time, *rec_flow;       // [rec_cap][N]
    uint32_t *rec_status;              // [rec_cap][N]
    int rec_every, rec_cap;
    int rec_phase, rec_slot0;  // outer steps taken since wt_ensemble_record before this call: % rec_every, / rec_every
    wtc::CtlArgs ctl;    // per-reactor PI programs run at PLC scans (wt_ensemble_control_*; ctl.on == 0: none)
    wti::InjArgs inj;    // per-reactor injection programs run at PLC scans (wt_ensemble_inject_*; inj.on == 0: none)
    wta::AlmArgs alm;    // per-reactor alarm and interlock programs run at PLC scans (wt_ensemble_alarm_*; alm.on == 0: none)
    wtv::ActArgs act;    // per-reactor actuator programs run at PLC scans (wt_ensemble_actuator_*; act.on == 0: none)
    wtd::DstArgs dst;    // per-reactor disturbance programs run after every outer step (wt_ensemble_disturb_*; dst.on == 0: none)
    wtsc::ScrArgs scr;   // per-reactor score programs run after every outer step (wt_ensemble_score_*; scr.on == 0: none)
    wtk::DetArgs det;    // per-reactor anomaly detector programs run at PLC scans (wt_ensemble_detect_*; det.on == 0: none)
    wtt::TrdArgs trd;    // per-reactor trend recorder programs run at PLC scans (wt_ensemble_trend_*; trd.on == 0: none)
    wtr::TrnArgs trn;    // the train program: stages feed their downstream after every outer step (wt_ensemble_train_*; trn.on == 0: none)
    wtw::WirArgs wir;    // the wire program: a train's signal cables, routed at the head of a PLC scan (wt_ensemble_wire_*; wir.on == 0: none)
    wtu::TunArgs tun;    // per-reactor relay autotune programs run at PLC scans before the PI programs (wt_ensemble_tune_*; tun.on == 0: none)
    wtin::InsArgs ins;   // the installation records of the sensor suite (wt_ensemble_install_*; ins.on == 0: the suite's own build)
    wtrp::RspArgs rsp;   // per-reactor response programs run at PLC scans between the tune program and the controllers (wt_ensemble_respond_*; rsp.on == 0: none)
    wtl::LnkArgs lnk;    // per-reactor link programs run at PLC scans before the injection programs, on readings and commands (wt_ensemble_link_*; lnk.on == 0: none)
    wtm::MpcArgs mpc;    // per-reactor model predictive controllers run at PLC scans between tune and PI programs (wt_ensemble_mpc_*; mpc.on == 0: none)
};
static_assert(sizeof(StepArgs) <= 4096, "the kernel-argument segment holds at most 4 KiB");
constexpr int NB = 10;     // rows of a boundary block (WT_NB)
// kernels that record and reload the schedule inside a work item (n <= 32); the others take one outer step per launch
__host__ __device__ constexpr bool x_in_item(int LV) { return LV <= 5; }
// kernels that carry the injection, alarm, actuator, disturbance, score, detector and trend recorder sections (wt_inj.hpp,
// wt_alm.hpp, wt_act.hpp, wt_dst.hpp, wt_scr.hpp, wt_det.hpp, wt_trd.hpp).  The n > 32 kernel has no register for them: every variant tried cost it 8 B of
// scratch and 4 VGPR spills, with or without a program, so it compiles the sections out and wt_ensemble_inject_set,
// _alarm_set, _actuator_set, _disturb_set, _score_set, _detect_set and _trend_set refuse ensembles of more than 32 zones.
// The train program's feed (wt_trn.hpp) shares the disturbance section; a train of two stages needs n <= 32 anyway,
// and so does the wire program on top of it (wt_wir.hpp).  The tune program (wt_tun.hpp) is in the same kernels only, and
// wt_ensemble_tune_set refuses more than 32 zones with the others' wording; so are the model predictive controllers
// (wt_mpc.hpp) and wt_ensemble_mpc_set, and the response programs (wt_rsp.hpp) and wt_ensemble_respond_set,
// and the link programs (wt_lnk.hpp) and wt_ensemble_link_set.
__host__ __device__ constexpr bool prog_in_item(int LV) { return LV <= 5; }
enum { Q_AVAIL = 0, Q_HEAD = 1, Q_TAIL = 2, Q_ERROR = 3, Q_TRACE = 4, Q_DONE = 5, Q_WORDS = 16 };

// The argument block has ~80 pointers; held in SGPRs across the solver loop they would crowd out the loop's own
// scalars (the compiler hoists kernel-argument loads to the top of the kernel and then spills them).  Each section
// of a work item therefore re-reads what it needs from the kernel-argument segment through a pointer the
// optimiser cannot see through, which ends the live ranges at the section's end.
typedef const __attribute__((address_space(4))) StepArgs *ArgPtr;
__device__ __forceinline__ ArgPtr fresh(ArgPtr p)
{
    asm volatile("" : "+s"(p));
    return p;
}

} // namespace wt
