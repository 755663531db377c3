// wtphys.hip -- host side of libwtphys.so: the C ABI declared in include/wtphys.h.
// Owns device memory behind an opaque handle, uploads the SoA constant / boundary
// blocks, launches the gfx950 kernels of wt_device.hpp on the handle's stream.
#include "wt_device.hpp"
#include "wt_diag.hpp"
#include "wt_place.hpp"
#include "wt_ckp.hpp"
#include "../../include/wtphys.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <string>
#include <vector>

#define WT_SNAPSHOT_PACK_MAX (256u * 1024u)   /* ensembles up to this image size download as one packed copy */

namespace {

thread_local std::string g_err;

int fail(int code, const std::string &msg)
{
    g_err = msg;
    return code;
}

#define HIP_TRY(expr)                                                                       \
    do {                                                                                    \
        hipError_t e_ = (expr);                                                             \
        if (e_ != hipSuccess)                                                               \
            return fail(WT_E_HIP, std::string(#expr) + ": " + hipGetErrorString(e_));       \
    } while (0)

int levels_for(int n)
{
    int l = 0;
    while ((1 << l) < n) ++l;
    return l < 1 ? 1 : l;
}

} // namespace

struct wt_mark;

struct wt_ensemble {
    int64_t N = 0;
    int n = 0, R = 0, device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    double *par = nullptr, *bc = nullptr;
    std::vector<double> par_sent;   // the constants as create uploaded them: what a checkpoint load or a copy compares
    double *pH = nullptr, *Cl = nullptr, *T = nullptr, *time = nullptr, *flow = nullptr;
    double *dH = nullptr, *dRho = nullptr, *dK = nullptr;
    uint32_t *status = nullptr;
    int32_t *stats = nullptr;
    int64_t *wave_diag = nullptr; // optional per-wavefront diagnostics (wt_ensemble_enable_wave_diag)
    double *bad_T = nullptr;      // [N] temperature named by the reference's ValueError
    // placement of reactors into wavefront-groups (wt_place.hpp): slot -> reactor, cost history, sort scratch
    int32_t *perm = nullptr, *cost = nullptr, *place_hist = nullptr;
    int placement = WT_PLACE_ADAPTIVE;
    int64_t cost_steps = 0;       // outer steps the cost history covers
    // device-side work queue of the default schedule (wt_queue.hpp): control words, FIFO slots, next step per group
    int32_t *q_ctrl = nullptr; unsigned long long *q_slots = nullptr; int32_t *q_next = nullptr;
    int q_cap = 0, q_workers = 0;
    int64_t n_groups = 0;
    int sched_mode = WT_SCHED_QUEUE;
    int64_t *trace = nullptr; int trace_cap = 0;   // developer item trace (wt_ensemble_item_trace)
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    bool have_bc = false, have_state = false;
    // The boundary block as the host last sent it (wt_ensemble_set_boundary, or the last row of a schedule), and whether
    // the device's block still is that block: then set_boundary of the same bytes has nothing to upload.  Whoever
    // writes bc on the device says so: disturb_op, train_op, and run_steps under plant I/O, a disturbance or a train
    // program.  bc_uploads counts the set_boundary calls that did upload.
    std::vector<double> bc_sent;
    bool bc_known = false;
    int64_t bc_uploads = 0;
    // Schedule.  WT_SCHED_QUEUE (default): one launch per wt_ensemble_step call, worker wavefronts take
    // (wavefront-group, next few outer steps) items from a device-side FIFO.  WT_SCHED_STREAMS (round-1
    // schedule, kept for comparison): n_sub contiguous reactor ranges on their own HIP streams, launches of
    // at most chunk_steps outer steps.  chunk_steps is also the PLC scan interval.
    // developer knobs (tools/), read from the environment once at creation: WT_Q_ITEM (outer steps per work item),
    // WT_PLACE_MIN (history before a re-deal), WT_Q_TICKETS (forces the launch split), WT_FULL_WAVES,
    // WT_DENSE_COUPLING (every solve takes the general path: the test that the fast paths give the same bits)
    // WT_CKP_MEMCPY (a checkpoint's device-to-device copies as one hipMemcpyAsync per array, not the table kernel)
    int knob_item = 0; int64_t knob_place_min = 0, knob_tickets = 0; int knob_dense = 0; int knob_memcpy = 0;
    // sticky record of a launch that did not advance every group (device word + pinned host mirror)
    int32_t *q_sticky = nullptr;   // device view of err_host (host-coherent pinned memory: the check kernel writes it in place)
    // one contiguous snapshot of a small ensemble: packed on the device, one copy into pinned memory
    void *snap_dev = nullptr, *snap_host = nullptr; size_t snap_bytes = 0;
    int32_t *err_host = nullptr;   // two words, each only ever set to 1: [0] a hand-off timed out, [1] a group was left behind
    int64_t redeals = 0;          // times the slots were re-dealt (bench.py reports it)
    int n_sub = 1, chunk_steps = WT_DEFAULT_CHUNK;
    int step_limit = 2000;    // attempts per outer step before a reactor is given up (reference: unlimited)
    hipStream_t sub_stream[WT_MAX_STREAMS] = {};
    hipEvent_t sub_done[WT_MAX_STREAMS] = {};
    hipEvent_t ev_fork = nullptr;
    double *diag_out = nullptr;
    // The kernel's argument structs of the optional parts, as every launch passes them (make_args adds what is per
    // call).  sens: fused sensor suite (wt_sensors.hpp, sens.on), plant I/O with its Modbus register images per reactor
    // (wt_plc.hpp, sens.plc_on: one PLC scan every chunk_steps outer steps), the command path into the boundary block.
    // The holding image lives in ctl.hr, which sens.cmd.hr repeats.  Then the per-reactor programs, [N] records each,
    // in WT_PROG_* order: k_programs below describes the host side of each; the service program's
    // records and switch are in sens, the tune program's in tun.  scr_steps: outer steps the step calls have taken
    // since score_set / score_reset (the index of the ensemble curve's next entry).
    wts::SuiteArgs sens = {};
    wtc::CtlArgs ctl = {};
    wti::InjArgs inj = {};
    wta::AlmArgs alm = {};
    wtv::ActArgs act = {};
    wtd::DstArgs dst = {};
    wtsc::ScrArgs scr = {};
    int64_t scr_steps = 0;
    wtk::DetArgs det = {};
    wtt::TrdArgs trd = {};
    // The train program (wt_trn.hpp; not one of k_programs: it changes the handle's shape).  trn_lk: host copy of trn.lk
    // (the disturbance conflict check reads it).  R0: reactors per wavefront as create chose them, what clear restores.
    wtr::TrnArgs trn = {};
    std::vector<int32_t> trn_lk;
    int R0 = 0;
    // The wire program on top of it (wt_wir.hpp): no switch of its own beyond wir.on, no host copy.
    wtw::WirArgs wir = {};
    // The tune program (wt_tun.hpp; WT_PROG_TUNE of k_programs): its records are plant I/O's arrays, its switch a PLIO scalar.
    wtu::TunArgs tun = {};
    // The installation records of the sensor suite (wt_ins.hpp; not one of k_programs): the suite's arrays and a SENS scalar.
    wtin::InsArgs ins = {};
    // The model predictive controllers (wt_mpc.hpp; not programs of k_programs either): plant I/O's arrays and a PLIO scalar.
    wtm::MpcArgs mpc = {};
    // The response programs (wt_rsp.hpp; not programs of k_programs either): plant I/O's arrays and a PLIO scalar.
    wtrp::RspArgs rsp = {};
    // The link programs (wt_lnk.hpp; not programs of k_programs either): plant I/O's arrays and PLIO scalars.
    wtl::LnkArgs lnk = {};
    // optional per-launch HIP-event timing (bench.py roofline accounting)
    bool time_launches = false;
    std::vector<hipEvent_t> lt_pool;   // start/stop pairs
    size_t lt_used = 0;
    // boundary schedule of wt_ensemble_step_scheduled ([n_steps][WT_NB][N], grown on demand); call_sched is set
    // only while such a call queues its launches
    double *sched = nullptr; size_t sched_bytes = 0; const double *call_sched = nullptr;
    // trajectory records of wt_ensemble_record
    struct Recording {
        double *pH = nullptr, *Cl = nullptr, *T = nullptr;   // [cap][N][n]
        double *time = nullptr, *flow = nullptr;             // [cap][N]
        uint32_t *status = nullptr;                          // [cap][N]
        int every = 1, cap = 0;
        int64_t steps = 0;                                   // outer steps since wt_ensemble_record
    } rec;
    wt_mark *mark = nullptr;      // the device-resident checkpoint of wt_ensemble_mark
};

namespace {

// recording is on and has free slots (afterwards the launches carry no record pointers at all)
bool recording_open(const wt_ensemble *h) { return h->rec.pH && h->rec.steps / h->rec.every < h->rec.cap; }

wt::StepArgs make_args(const wt_ensemble *h, double dt, int n_steps, int first_step, int call_steps, int scan_every)
{
    wt::StepArgs a;
    a.N = h->N; a.r0 = 0; a.r1 = h->N; a.n = h->n; a.R = h->R;
    a.par = h->par; a.bc = h->bc;
    a.pH = h->pH; a.Cl = h->Cl; a.T = h->T; a.time = h->time; a.flow = h->flow;
    a.dH = h->dH; a.dRho = h->dRho; a.dK = h->dK;
    a.status = h->status; a.stats = h->stats; a.wave_diag = h->wave_diag; a.bad_T = h->bad_T;
    a.perm = h->perm; a.cost = (h->placement == WT_PLACE_ADAPTIVE) ? h->cost : nullptr;
    a.dt = dt; a.n_steps = n_steps; a.first_step = first_step; a.call_steps = call_steps; a.step_limit = h->step_limit;
    a.q_ctrl = nullptr; a.q_slots = nullptr; a.q_next = nullptr; a.q_cap = 0; a.item_steps = n_steps; a.n_groups = (int)h->n_groups;
    a.trace = h->trace; a.trace_cap = h->trace_cap;
    a.kt = wt::default_ktab(); a.rt = wt::default_rtab();
    a.kt.dense_bias = h->knob_dense ? 1.0 : 0.0;
    a.sens = h->sens; a.ctl = h->ctl; a.inj = h->inj; a.alm = h->alm; a.act = h->act; a.dst = h->dst; a.scr = h->scr; a.det = h->det; a.trd = h->trd; a.trn = h->trn; a.wir = h->wir; a.tun = h->tun; a.ins = h->ins; a.mpc = h->mpc; a.rsp = h->rsp; a.lnk = h->lnk;
    // a full curve takes no more entries: the launches then carry no curve pointer at all
    const bool curve = h->scr.counts && h->scr_steps < h->scr.curve_cap;
    if (!curve) a.scr.counts = nullptr;
    a.scr.step0 = curve ? (int)h->scr_steps : 0;
    a.sens.scan_every = scan_every > 0 ? scan_every : 1;
    a.sched = h->call_sched;
    const bool rec = recording_open(h);
    a.rec_pH = rec ? h->rec.pH : nullptr; a.rec_Cl = h->rec.Cl; a.rec_T = h->rec.T;
    a.rec_time = h->rec.time; a.rec_flow = h->rec.flow; a.rec_status = h->rec.status;
    a.rec_every = h->rec.every; a.rec_cap = h->rec.cap;
    a.rec_phase = rec ? (int)(h->rec.steps % h->rec.every) : 0;
    a.rec_slot0 = rec ? (int)(h->rec.steps / h->rec.every) : 0;
    a.x_on = (a.sched || a.rec_pH) ? 1 : 0;
    return a;
}

template <class T> void free_and_null(T *&p) { if (p) (void)hipFree(p); p = nullptr; }

// The device arrays of one part of the handle (core, sensor suite, plant I/O, recording, a program): allocated
// together, all or none, and released together with the part's switch.  The sizes come from the handle alone: a call
// stores a new capacity there before it allocates, and release puts it back to 0, as a fresh handle has it.
struct ArrayGroup {
    const char *name;                                   // prefix of an allocation error
    int *on;                                            // the part's switch (nullptr: none)
    std::vector<std::pair<void **, size_t>> arrays;     // where each pointer lives, its bytes (0: not allocated)
    std::function<void()> zero;                         // zeroes the capacities the bytes come from (empty: none)
};

void release(const ArrayGroup &g)
{
    for (const auto &a : g.arrays) free_and_null(*a.first);
    if (g.on) *g.on = 0;
    if (g.zero) g.zero();
}

// allocates the group's arrays unless an earlier call did; on failure none is left behind
int allocate(const ArrayGroup &g)
{
    if (*g.arrays[0].first) return WT_OK;
    for (const auto &a : g.arrays) {
        const hipError_t e = a.second ? hipMalloc(a.first, a.second) : hipSuccess;
        if (e != hipSuccess) { release(g); return fail(WT_E_HIP, std::string(g.name) + ": " + hipGetErrorString(e)); }
    }
    return WT_OK;
}

ArrayGroup core_arrays(wt_ensemble *h)
{
    const size_t N = (size_t)h->N, zone = sizeof(double) * N * (size_t)h->n;
    return {"create", nullptr, {{(void **)&h->par, sizeof(double) * WT_NP * N}, {(void **)&h->bc, sizeof(double) * WT_NB * N},
                                {(void **)&h->pH, zone}, {(void **)&h->Cl, zone}, {(void **)&h->T, zone},
                                {(void **)&h->dH, zone}, {(void **)&h->dRho, zone}, {(void **)&h->dK, zone},
                                {(void **)&h->time, sizeof(double) * N}, {(void **)&h->flow, sizeof(double) * N},
                                {(void **)&h->status, sizeof(uint32_t) * N}, {(void **)&h->stats, sizeof(int32_t) * 5 * N},
                                {(void **)&h->bad_T, sizeof(double) * N}, {(void **)&h->perm, sizeof(int32_t) * N},
                                {(void **)&h->cost, sizeof(int32_t) * N},
                                {(void **)&h->place_hist, sizeof(int32_t) * wtpl::BINS * ((N + wtpl::CHUNK - 1) / wtpl::CHUNK)},
                                {(void **)&h->q_ctrl, sizeof(int32_t) * wt::Q_WORDS}}};
}

// the work queue's arrays that are sized by the group count: a train program changes it (reshape)
ArrayGroup queue_arrays(wt_ensemble *h)
{
    return {"queue", nullptr, {{(void **)&h->q_slots, sizeof(unsigned long long) * (size_t)h->q_cap},
                               {(void **)&h->q_next, sizeof(int32_t) * (size_t)h->n_groups}}};
}

// the history arrays only for hist_cap > 0; the service program's records (wt_svc.hpp) and the installation records
// (wt_ins.hpp) come and go with the suite
ArrayGroup sensor_arrays(wt_ensemble *h)
{
    wts::SuiteArgs &s = h->sens;
    const size_t N = (size_t)h->N, hist = (size_t)s.hist_cap * wts::NSENS * N;
    return {"sensors", &s.on, {{(void **)&s.fs, sizeof(float) * wts::NSENS * wts::NF * N},
                               {(void **)&s.ds, sizeof(double) * wts::NSENS * wts::ND * N},
                               {(void **)&s.is, sizeof(int32_t) * wts::NSENS * wts::NI * N},
                               {(void **)&s.full_scale, sizeof(float) * N},
                               {(void **)&s.ring_t, sizeof(double) * 2 * wts::RING * N},
                               {(void **)&s.ring_v, sizeof(float) * 2 * wts::RING * N},
                               {(void **)&s.ring_push, sizeof(int32_t) * 2 * N}, {(void **)&s.ring_cursor, sizeof(int32_t) * 2 * N},
                               {(void **)&s.out_value, sizeof(float) * wts::NSENS * N},
                               {(void **)&s.out_status, wts::NSENS * N}, {(void **)&s.out_fault, wts::NSENS * N},
                               {(void **)&s.t_enable, sizeof(double) * N},
                               {(void **)&s.svc_par, sizeof(double) * wtsv::PAR_DOUBLES * N},
                               {(void **)&s.svc_st, sizeof(double) * wtsv::ST_DOUBLES * N},
                               {(void **)&h->ins.par, sizeof(double) * wtin::REC_DOUBLES * N},
                               {(void **)&s.hist_value, sizeof(float) * hist}, {(void **)&s.hist_status, hist},
                               {(void **)&s.hist_fault, hist}, {(void **)&s.hist_pos, s.hist_cap > 0 ? sizeof(int32_t) * N : 0}},
            [h] { h->sens.hist_cap = 0; h->sens.svc_on = 0; h->ins.on = 0; }};
}

// the tune program's records (wt_tun.hpp), the model predictive controllers' arrays (wt_mpc.hpp), the response
// programs' records (wt_rsp.hpp) and the link programs' records and rings (wt_lnk.hpp) come and go with plant I/O
ArrayGroup plant_io_arrays(wt_ensemble *h)
{
    const size_t N = (size_t)h->N;
    return {"plc_enable", &h->sens.plc_on, {{(void **)&h->sens.pack.ir, sizeof(uint16_t) * wtp::IR_WORDS * N},
                                            {(void **)&h->ctl.hr, sizeof(uint16_t) * wtp::HR_WORDS * N},
                                            {(void **)&h->sens.pack.loop_time, sizeof(double) * N},
                                            {(void **)&h->sens.pack.update_ok, N},
                                            {(void **)&h->tun.par, sizeof(double) * wtu::PAR_DOUBLES * N},
                                            {(void **)&h->tun.st, sizeof(double) * wtu::ST_DOUBLES * N},
                                            {(void **)&h->mpc.par, sizeof(double) * wtm::PAR_DOUBLES * N},
                                            {(void **)&h->mpc.st, sizeof(double) * wtm::ST_DOUBLES * N},
                                            {(void **)&h->mpc.step, sizeof(double) * wtm::ROW_DOUBLES * N},
                                            {(void **)&h->mpc.gain, sizeof(double) * wtm::ROW_DOUBLES * N},
                                            {(void **)&h->mpc.pred, sizeof(double) * wtm::ROW_DOUBLES * N},
                                            {(void **)&h->rsp.par, sizeof(double) * wtrp::PAR_DOUBLES * N},
                                            {(void **)&h->rsp.st, sizeof(double) * wtrp::ST_DOUBLES * N},
                                            {(void **)&h->rsp.rst, sizeof(double) * wtrp::RST_DOUBLES * N},
                                            {(void **)&h->lnk.par, sizeof(double) * wtl::PAR_DOUBLES * N},
                                            {(void **)&h->lnk.st, sizeof(double) * wtl::ST_DOUBLES * N},
                                            {(void **)&h->lnk.ring, sizeof(double) * wtl::RING_ENTRIES * N},
                                            {(void **)&h->lnk.fring, sizeof(uint8_t) * wtl::RING_ENTRIES * N}},
            [h] { h->tun.on = 0; h->mpc.on = 0; h->rsp.on = 0; h->lnk.on = 0; }};
}

ArrayGroup record_arrays(wt_ensemble *h)
{
    wt_ensemble::Recording &r = h->rec;
    const size_t records = (size_t)r.cap * (size_t)h->N, zone = sizeof(double) * records * (size_t)h->n;
    return {"record", nullptr, {{(void **)&r.pH, zone}, {(void **)&r.Cl, zone}, {(void **)&r.T, zone},
                                {(void **)&r.time, sizeof(double) * records}, {(void **)&r.flow, sizeof(double) * records},
                                {(void **)&r.status, sizeof(uint32_t) * records}},
            [h] { h->rec = {}; }};
}

ArrayGroup control_arrays(wt_ensemble *h)
{
    const size_t N = (size_t)h->N;
    return {"control", &h->ctl.on, {{(void **)&h->ctl.par, sizeof(double) * wtc::PAR_DOUBLES * N},
                                    {(void **)&h->ctl.st, sizeof(double) * wtc::ST_DOUBLES * N}}};
}

ArrayGroup inject_arrays(wt_ensemble *h)
{
    const size_t N = (size_t)h->N;
    return {"inject", &h->inj.on, {{(void **)&h->inj.par, sizeof(double) * wti::PAR_DOUBLES * N},
                                   {(void **)&h->inj.st, sizeof(double) * wti::ST_DOUBLES * N}}};
}

ArrayGroup alarm_arrays(wt_ensemble *h)
{
    const size_t N = (size_t)h->N;
    return {"alarm", &h->alm.on, {{(void **)&h->alm.par, sizeof(double) * wta::PAR_DOUBLES * N},
                                  {(void **)&h->alm.st, sizeof(double) * wta::ST_DOUBLES * N},
                                  {(void **)&h->alm.rst, sizeof(double) * wta::RST_DOUBLES * N},
                                  {(void **)&h->alm.word, sizeof(uint16_t) * N}}};
}

ArrayGroup actuator_arrays(wt_ensemble *h)
{
    const size_t N = (size_t)h->N;
    return {"actuator", &h->act.on, {{(void **)&h->act.par, sizeof(double) * wtv::PAR_DOUBLES * N},
                                     {(void **)&h->act.st, sizeof(double) * wtv::ST_DOUBLES * N},
                                     {(void **)&h->act.q, sizeof(double) * wtv::Q_DOUBLES * N},
                                     {(void **)&h->act.tp, sizeof(double) * N}}};
}

// the history array only for hist_cap > 0
ArrayGroup disturb_arrays(wt_ensemble *h)
{
    const size_t N = (size_t)h->N;
    return {"disturb", &h->dst.on, {{(void **)&h->dst.par, sizeof(double) * wtd::PAR_DOUBLES * N},
                                    {(void **)&h->dst.st, sizeof(double) * wtd::ST_DOUBLES * N},
                                    {(void **)&h->dst.base, sizeof(double) * WT_NB * N},
                                    {(void **)&h->dst.tp, sizeof(double) * N},
                                    {(void **)&h->dst.hist, sizeof(double) * wtd::SLOTS * (size_t)h->dst.hist_cap * N}},
            [h] { h->dst.hist_cap = 0; }};
}

// the curve arrays only for curve_cap > 0, the fan only for bins > 0
ArrayGroup score_arrays(wt_ensemble *h)
{
    const int bins = h->scr.bins;
    const size_t N = (size_t)h->N, cells = (size_t)h->scr.curve_cap * wtsc::SLOTS;
    return {"score", &h->scr.on, {{(void **)&h->scr.par, sizeof(double) * wtsc::PAR_DOUBLES * N},
                                  {(void **)&h->scr.st, sizeof(double) * wtsc::ST_DOUBLES * N},
                                  {(void **)&h->scr.tp, sizeof(double) * N},
                                  {(void **)&h->scr.counts, sizeof(int32_t) * 3 * cells},
                                  {(void **)&h->scr.fan, bins > 0 ? sizeof(int32_t) * (size_t)(bins + 2) * cells : 0}},
            [h] { h->scr.curve_cap = h->scr.bins = 0; h->scr_steps = 0; }};
}

ArrayGroup detect_arrays(wt_ensemble *h)
{
    const size_t N = (size_t)h->N;
    return {"detect", &h->det.on, {{(void **)&h->det.par, sizeof(double) * wtk::PAR_DOUBLES * N},
                                   {(void **)&h->det.st, sizeof(double) * wtk::ST_DOUBLES * N},
                                   {(void **)&h->det.lab, sizeof(double) * wtk::NKR * N},
                                   {(void **)&h->det.tp, sizeof(double) * N}}};
}

ArrayGroup train_arrays(wt_ensemble *h)
{
    const size_t N = (size_t)h->N;
    wtr::JctArgs &j = h->trn.jct;   // the junction program's arrays come and go with the train's; tmp (last) is scratch
    return {"train", &h->trn.on, {{(void **)&h->trn.lk, sizeof(int32_t) * N},
                                  {(void **)&h->trn.st, sizeof(double) * wtr::NTRS * N},
                                  {(void **)&h->trn.base, sizeof(double) * wtr::FED_ROWS * N},
                                  {(void **)&j.src, sizeof(uint32_t) * N}, {(void **)&j.share, sizeof(double) * wtr::JCT_SLOTS * N},
                                  {(void **)&j.st, sizeof(double) * wtr::NJS * N}, {(void **)&j.base0, sizeof(double) * N},
                                  {(void **)&j.tmp, sizeof(double) * wtr::JCT_TMP * N}},
            [h] { h->trn.length = 0; h->trn.jct.on = 0; h->trn_lk.clear(); }};
}

// the pipe program's arrays (wt_trn.hpp); the ring is sized by pipe.slots, which the set call stores first
ArrayGroup pipe_arrays(wt_ensemble *h)
{
    wtr::PipeArgs &p = h->trn.pipe;
    const size_t N = (size_t)h->N;
    return {"pipe", &p.on, {{(void **)&p.delay, sizeof(int32_t) * N}, {(void **)&p.head, sizeof(int32_t) * N},
                            {(void **)&p.st, sizeof(double) * wtr::NPS * N},
                            {(void **)&p.ring, sizeof(double) * wtr::PIPE_Q * (size_t)p.slots * N}},
            [h] { h->trn.pipe.slots = 0; }};
}

// the wire program's arrays (wt_wir.hpp)
ArrayGroup wire_arrays(wt_ensemble *h)
{
    const size_t N = (size_t)h->N;
    return {"wire", &h->wir.on, {{(void **)&h->wir.src, sizeof(uint64_t) * N},
                                 {(void **)&h->wir.st, sizeof(double) * wtw::ST_DOUBLES * N}}};
}

ArrayGroup trend_arrays(wt_ensemble *h)
{
    const size_t N = (size_t)h->N;
    return {"trend", &h->trd.on, {{(void **)&h->trd.par, sizeof(double) * wtt::PAR_DOUBLES * N},
                                  {(void **)&h->trd.st, sizeof(double) * wtt::ST_DOUBLES * N},
                                  {(void **)&h->trd.store, sizeof(double2) * wtt::SLOTS * (size_t)h->trd.cap * N}},
            [h] { h->trd.cap = 0; }};
}

// Units (reactors, or trains under a train program) per wavefront, at most `most`.  A small ensemble is spread over all
// SIMDs rather than packed into full wavefronts: a wavefront costs what its slowest reactor costs, so fewer per
// wavefront is faster as long as every wavefront still finds a SIMD (about 4 per CU).  Results do not depend on it.
int units_per_wavefront(int device, int64_t units, int most)
{
    int cus = 256; hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) == hipSuccess && prop.multiProcessorCount > 0) cus = prop.multiProcessorCount;
    const int64_t slots = (int64_t)cus * 4;
    int64_t r = (units + slots - 1) / slots;
    if (const char *e = getenv("WT_FULL_WAVES")) if (atoi(e) != 0) r = most;      // tuning knob (tools/)
    if (r < 1) r = 1;
    return r < most ? (int)r : most;
}

bool row_mode(int n) { return n == 2 || n == 4 || n == 8 || n == 16; }

// default stream schedule: up to 4 ranges, but keep at least 64 wavefronts per range
int default_streams(int64_t n_reactors, int R)
{
    const int64_t waves = (n_reactors + R - 1) / R;
    const int ns = (int)(waves / 64);
    return ns < 1 ? 1 : (ns > 4 ? 4 : ns);
}

// the kernel instantiation for this zone count
template <class F> void with_step_kernel(const wt_ensemble *h, F &&f)
{
    const int n = h->n;
#if defined(WT_ONLY_LV3)   // scratch builds for kernel tuning: n = 8 only (the row-shift variant)
    (void)n;
    f(wt::step_kernel<3, true>, 64);
#elif defined(WT_ONLY_LV5)   // ... n in 17..32 only
    (void)n;
    f(wt::step_kernel<5, false>, 64);
#else
    const int lv = levels_for(n);
    if (row_mode(n)) { // n in {2,4,8,16}: every cross-lane move is a DPP row operation
        switch (lv) {
        case 1: f(wt::step_kernel<1, true>, 64); break;
        case 2: f(wt::step_kernel<2, true>, 64); break;
        case 3: f(wt::step_kernel<3, true>, 64); break;
        default: f(wt::step_kernel<4, true>, 64); break;
        }
    } else {
        switch (lv) {
        case 2: f(wt::step_kernel<2, false>, 64); break;
        case 3: f(wt::step_kernel<3, false>, 64); break;
        case 4: f(wt::step_kernel<4, false>, 64); break;
        case 5: f(wt::step_kernel<5, false>, 64); break;
        default: f(wt::step_kernel<6, false>, 64); break;
        }
    }
#endif
}

void launch_step_raw(const wt_ensemble *h, const wt::StepArgs &a, unsigned grid, hipStream_t stream)
{
    with_step_kernel(h, [&](auto kernel, int block) { hipLaunchKernelGGL(kernel, dim3(grid), dim3(block), 0, stream, a); });
}

// one kernel launch, bracketed by HIP events on its own stream when launch timing is on
void launch_step(wt_ensemble *h, const wt::StepArgs &a, unsigned grid, hipStream_t stream)
{
    bool timed = h->time_launches;
    if (timed && h->lt_used + 2 > h->lt_pool.size()) {
        for (int i = 0; i < 2 && timed; ++i) {
            hipEvent_t e;
            if (hipEventCreate(&e) != hipSuccess) timed = false; else h->lt_pool.push_back(e);
        }
        if (!timed) while (h->lt_pool.size() > h->lt_used) { (void)hipEventDestroy(h->lt_pool.back()); h->lt_pool.pop_back(); }
    }
    if (timed) (void)hipEventRecord(h->lt_pool[h->lt_used], stream);
    launch_step_raw(h, a, grid, stream);
    if (timed) { (void)hipEventRecord(h->lt_pool[h->lt_used + 1], stream); h->lt_used += 2; }
}

// Outer steps per work item of the queue schedule.  A group changes hands at item boundaries, which costs a few
// microseconds (state out and in, release / acquire), so not every step -- but often enough that the groups
// sharing the workers take turns at least half a dozen times; at most 32 steps.
int queue_item_steps(const wt_ensemble *h, int n_steps)
{
    int item = n_steps / 6;
    if (item > 32) item = 32;
    if (item < 1) item = 1;
    if (h->knob_item > 0) item = h->knob_item;
    return item;
}

// worker wavefronts of the queue schedule: as many as the device keeps resident (no more than there are groups)
int queue_workers(const wt_ensemble *h)
{
    int per_cu = 0, cus = 0;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, h->device) == hipSuccess) cus = prop.multiProcessorCount;
    with_step_kernel(h, [&](auto kernel, int block) {
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, block, 0) != hipSuccess) per_cu = 0;
    });
    if (cus <= 0) cus = 256;
    if (per_cu <= 0) per_cu = 4;
    const int64_t cap = (int64_t)cus * per_cu;
    return (int)(h->n_groups < cap ? h->n_groups : cap);
}

const char *k_incomplete = "a step launch did not advance every wavefront-group (work-queue hand-off timed out or a group was left behind); the state on the device is incomplete";

// Synchronises the handle's stream, then fails if a launch has set the sticky record (host-coherent memory, valid
// once the stream is synchronised): what was downloaded comes from an incomplete state.
int sync_checked(wt_ensemble *h)
{
    HIP_TRY(hipStreamSynchronize(h->stream));
    if (h->err_host[0] | h->err_host[1]) return fail(WT_E_HIP, k_incomplete);
    return WT_OK;
}

struct Copy { void *dst; const void *src; size_t bytes; };   // dst nullptr: not wanted

// Every download: the copies queued on the handle's stream, then sync_checked.
int download(wt_ensemble *h, const std::vector<Copy> &copies)
{
    for (const Copy &c : copies)
        if (c.dst && c.bytes) HIP_TRY(hipMemcpyAsync(c.dst, c.src, c.bytes, hipMemcpyDeviceToHost, h->stream));
    return sync_checked(h);
}

// [slots][fields][N] blocks of the C ABI <-> the device's [N][stride] records, slot s at s * fields of a record
void blocks_to_records(const double *block, int slots, int fields, int64_t N, double *rec, int stride)
{
    for (int s = 0; s < slots; ++s)
        for (int k = 0; k < fields; ++k)
            for (int64_t r = 0; r < N; ++r) rec[r * stride + s * fields + k] = block[((int64_t)s * fields + k) * N + r];
}

void records_to_blocks(const double *rec, int stride, int slots, int fields, int64_t N, double *block)
{
    for (int s = 0; s < slots; ++s)
        for (int k = 0; k < fields; ++k)
            for (int64_t r = 0; r < N; ++r) block[((int64_t)s * fields + k) * N + r] = rec[r * stride + s * fields + k];
}

struct Records { double *block; const double *rec; int stride, slots, fields; };   // block nullptr: not wanted

// Downloads [N][stride] records (one synchronisation for all) into [slots][fields][N] blocks.
int download_records(wt_ensemble *h, const std::vector<Records> &parts)
{
    const int64_t N = h->N;
    size_t total = 0;
    for (const Records &p : parts) total += p.block ? (size_t)(N * p.stride) : 0;
    std::vector<double> host(total);
    std::vector<Copy> copies;
    double *at = host.data();
    for (const Records &p : parts)
        if (p.block) { copies.push_back({at, p.rec, sizeof(double) * (size_t)(N * p.stride)}); at += N * p.stride; }
    if (int rc = download(h, copies)) return rc;
    at = host.data();
    for (const Records &p : parts)
        if (p.block) { records_to_blocks(at, p.stride, p.slots, p.fields, N, p.block); at += N * p.stride; }
    return WT_OK;
}

// The disturbance program's host operations (wtd::host_op_kernel) on the handle's stream, not synchronised.
int disturb_op(wt_ensemble *h, int op)
{
    h->bc_known = false;   // every op writes the targeted rows
    const wtd::HostOpArgs a{h->dst, h->bc, h->time, h->N, op};
    hipLaunchKernelGGL(wtd::host_op_kernel<wt::ExpK>, dim3((unsigned)((h->N + 255) / 256)), dim3(256), 0, h->stream, a);
    HIP_TRY(hipGetLastError());
    return WT_OK;
}

// The wire program's restart (wt_wir.hpp): n_routed = n_lost = 0 in every slot (set, and set_state with a program
// set); queued on the handle's stream.
int wire_restart(wt_ensemble *h)
{
    HIP_TRY(hipMemsetAsync(h->wir.st, 0, sizeof(double) * wtw::ST_DOUBLES * (size_t)h->N, h->stream));
    return WT_OK;
}

// The train program's host operations (wtr::host_op_kernel) on the handle's stream, not synchronised.
int train_op(wt_ensemble *h, int op)
{
    h->bc_known = false;   // a feed, a restore or a delivery writes the linked rows
    wtr::HostOpArgs a{h->trn, h->bc, h->pH, h->Cl, h->T, h->time, h->N, h->n, op};
    const dim3 grid((unsigned)((h->N + 255) / 256));
    if (h->trn.jct.on && (op == wtr::OP_FEED || op == wtr::OP_PIPE_FILL)) {   // every blend before any store
        a.op = wtr::OP_JCT_BLEND;
        hipLaunchKernelGGL(wtr::host_op_kernel<wt::JctK>, grid, dim3(256), 0, h->stream, a);
        HIP_TRY(hipGetLastError());
        a.op = op;
    }
    hipLaunchKernelGGL(wtr::host_op_kernel<wt::JctK>, grid, dim3(256), 0, h->stream, a);
    HIP_TRY(hipGetLastError());
    return WT_OK;
}

// -- the junction program (wt_trn.hpp) on top of a train program: what plant I/O asks of it (a disturbance slot never
// targets row 0 -- wt_program_check refuses it -- so a carried flow and the disturbance program cannot meet)
const char *k_junction_plant_io = "a carried flow cannot be combined with plant I/O (the scan's command path writes row 0 in the same outer step)";

// the junction words of a set program (empty: none is set)
int junction_words(wt_ensemble *h, std::vector<uint32_t> &w)
{
    w.clear();
    if (!h->trn.jct.on) return WT_OK;
    w.resize((size_t)h->N);
    return download(h, {{w.data(), h->trn.jct.src, sizeof(uint32_t) * w.size()}});
}

// The device work of wt_ensemble_set_boundary.  The block is "known" once its copy is queued and before the programs'
// ops run: under a disturbance or a train program they leave it unknown again, which is what the device then holds.
int upload_boundary(wt_ensemble *h, const double *bc)
{
    const size_t cells = (size_t)WT_NB * (size_t)h->N;
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipMemcpyAsync(h->bc, bc, sizeof(double) * cells, hipMemcpyHostToDevice, h->stream));
    h->bc_sent.assign(bc, bc + cells);
    h->bc_known = true;
    ++h->bc_uploads;
    if (h->dst.on) {   // a disturbance program: the new block is its base, the targeted rows are recomposed (no draw)
        HIP_TRY(hipMemcpyAsync(h->dst.base, h->bc, sizeof(double) * cells, hipMemcpyDeviceToDevice, h->stream));
        if (int rc = disturb_op(h, wtd::OP_COMPOSE)) return rc;
    }
    // a train program: rows 1..3 of the new block are its base, every link is fed from the current state (a link with
    // a pipe: the sample its line last delivered)
    if (h->trn.on) {
        HIP_TRY(hipMemcpyAsync(h->trn.base, bc + h->N, sizeof(double) * wtr::FED_ROWS * h->N, hipMemcpyHostToDevice, h->stream));
        // a junction program: row 0 is the base of its carriers
        if (h->trn.jct.on) HIP_TRY(hipMemcpyAsync(h->trn.jct.base0, bc, sizeof(double) * h->N, hipMemcpyHostToDevice, h->stream));
        if (int rc = train_op(h, wtr::OP_FEED)) return rc;
    }
    HIP_TRY(hipStreamSynchronize(h->stream));   // the caller's block is free on return
    h->have_bc = true;
    return WT_OK;
}

} // namespace

extern "C" {

int wt_abi_version(void) { return WT_ABI_VERSION; }
const char *wt_last_error(void) { return g_err.c_str(); }

int wt_device_count(int *count)
{
    if (!count) return fail(WT_E_ARG, "count is NULL");
    int c = 0;
    hipError_t e = hipGetDeviceCount(&c);
    if (e != hipSuccess) { *count = 0; return fail(WT_E_NOGPU, hipGetErrorString(e)); }
    *count = c;
    return WT_OK;
}

int wt_ensemble_create(int64_t n_reactors, int n_zones, int device, const double *par, wt_ensemble **out)
{
    if (!out || !par) return fail(WT_E_ARG, "NULL argument");
    *out = nullptr;
    if (n_reactors <= 0) return fail(WT_E_ARG, "n_reactors must be positive");
    if (n_zones < 2 || n_zones > WT_MAX_ZONES)
        return fail(WT_E_ARG, "Need at least 2 zones and at most 64, got " + std::to_string(n_zones));
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return fail(WT_E_NOGPU, "no HIP device available: libwtphys has no CPU path");
    if (device < 0 || device >= ndev) return fail(WT_E_ARG, "bad device index");
    HIP_TRY(hipSetDevice(device));
    wt_ensemble *h = new wt_ensemble();
    h->N = n_reactors; h->n = n_zones; h->device = device;
    h->R = h->R0 = units_per_wavefront(device, n_reactors, 64 / n_zones);
    const size_t N = (size_t)n_reactors, nz = (size_t)n_zones;
    auto cleanup = [&]() { wt_ensemble_destroy(h); };
    h->n_groups = (n_reactors + h->R - 1) / h->R;
    if (h->n_groups > 0x3fffffff) { cleanup(); return fail(WT_E_ARG, "too many reactors for one ensemble"); }
    h->q_cap = (int)(2 * h->n_groups + 64);
    if (int rc = allocate(core_arrays(h))) { cleanup(); return rc; }
    if (int rc = allocate(queue_arrays(h))) { cleanup(); return rc; }
    {   // small ensembles (the drop-in's N = 1 above all) are downloaded as one packed image through pinned memory
        const size_t image = sizeof(double) * (6 * N * nz + 2 * N) + sizeof(uint32_t) * (N + 1);
        if (image <= WT_SNAPSHOT_PACK_MAX) {
            h->snap_bytes = (image + 7) & ~(size_t)7;
            if (hipMalloc(&h->snap_dev, h->snap_bytes) != hipSuccess) { cleanup(); return fail(WT_E_HIP, "hipMalloc failed"); }
            if (hipHostMalloc(&h->snap_host, h->snap_bytes, hipHostMallocDefault) != hipSuccess) { cleanup(); return fail(WT_E_HIP, "hipHostMalloc failed"); }
        }
        if (hipHostMalloc((void **)&h->err_host, 2 * sizeof(int32_t), hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess) { cleanup(); return fail(WT_E_HIP, "hipHostMalloc failed"); }
        h->err_host[0] = h->err_host[1] = 0;
        if (hipHostGetDevicePointer((void **)&h->q_sticky, h->err_host, 0) != hipSuccess) { cleanup(); return fail(WT_E_HIP, "hipHostGetDevicePointer failed"); }
    }
    if (const char *e = getenv("WT_Q_ITEM")) h->knob_item = atoi(e);
    if (const char *e = getenv("WT_PLACE_MIN")) h->knob_place_min = atoll(e);
    if (const char *e = getenv("WT_Q_TICKETS")) h->knob_tickets = atoll(e);
    if (const char *e = getenv("WT_DENSE_COUPLING")) h->knob_dense = atoi(e) != 0;
    if (const char *e = getenv("WT_CKP_MEMCPY")) h->knob_memcpy = atoi(e) != 0;
    h->par_sent.assign(par, par + (size_t)WT_NP * N);
    h->sens.N = h->sens.cmd.N = h->N;
    h->sens.cmd.bc = h->bc;
    if (hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking) != hipSuccess) { cleanup(); return fail(WT_E_HIP, "hipStreamCreate failed"); }
    h->own_stream = true;
    if (hipEventCreate(&h->ev0) != hipSuccess || hipEventCreate(&h->ev1) != hipSuccess) { cleanup(); return fail(WT_E_HIP, "hipEventCreate failed"); }
    if (hipEventCreateWithFlags(&h->ev_fork, hipEventDisableTiming) != hipSuccess) { cleanup(); return fail(WT_E_HIP, "hipEventCreate failed"); }
    h->n_sub = default_streams(n_reactors, h->R);
    h->chunk_steps = WT_DEFAULT_CHUNK;
    h->sched_mode = WT_SCHED_QUEUE;
    h->q_workers = queue_workers(h);
    hipError_t e = hipMemcpyAsync(h->par, par, sizeof(double) * WT_NP * N, hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess) e = hipMemsetAsync(h->status, 0, sizeof(uint32_t) * N, h->stream);
    if (e == hipSuccess) e = hipMemsetAsync(h->stats, 0, sizeof(int32_t) * 5 * N, h->stream);
    if (e == hipSuccess) e = hipMemsetAsync(h->time, 0, sizeof(double) * N, h->stream);
    if (e == hipSuccess) e = hipMemsetAsync(h->flow, 0, sizeof(double) * N, h->stream);
    if (e == hipSuccess) e = hipMemsetAsync(h->bad_T, 0, sizeof(double) * N, h->stream);
    if (e == hipSuccess) e = hipMemsetAsync(h->cost, 0, sizeof(int32_t) * N, h->stream);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(wtpl::iota_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, h->stream, h->perm, (int64_t)N);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemsetAsync(h->q_ctrl, 0, sizeof(int32_t) * wt::Q_WORDS, h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess) { cleanup(); return fail(WT_E_HIP, std::string("upload: ") + hipGetErrorString(e)); }
    *out = h;
    return WT_OK;
}

int wt_ensemble_set_stream(wt_ensemble *h, void *hip_stream)
{
    if (!h) return fail(WT_E_ARG, "NULL handle");
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipStreamSynchronize(h->stream));
    if (h->own_stream && h->stream) (void)hipStreamDestroy(h->stream);
    h->stream = (hipStream_t)hip_stream;
    h->own_stream = false;
    return WT_OK;
}

int wt_ensemble_set_state(wt_ensemble *h, const double *pH, const double *Cl, const double *T, const double *time)
{
    if (!h || !pH || !Cl || !T) return fail(WT_E_ARG, "NULL argument");
    HIP_TRY(hipSetDevice(h->device));
    const size_t cnt = (size_t)h->N * h->n;
    HIP_TRY(hipMemcpyAsync(h->pH, pH, sizeof(double) * cnt, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipMemcpyAsync(h->Cl, Cl, sizeof(double) * cnt, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipMemcpyAsync(h->T, T, sizeof(double) * cnt, hipMemcpyHostToDevice, h->stream));
    if (time) HIP_TRY(hipMemcpyAsync(h->time, time, sizeof(double) * h->N, hipMemcpyHostToDevice, h->stream));
    // ReactorState.update_derived placeholders (reactor.py:137-147), filled where the state now lives
    wt::PlaceholderArgs pa{(int64_t)cnt, h->pH, h->dH, h->dRho, h->dK};
    hipLaunchKernelGGL(wt::derived_placeholder_kernel, dim3((unsigned)((cnt + 255) / 256)), dim3(256), 0, h->stream, pa);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemsetAsync(h->status, 0, sizeof(uint32_t) * h->N, h->stream));
    // a pipe program: a new state is a new plant -- every line full of it, the pipe state from the start
    if (h->trn.pipe.on) if (int rc = train_op(h, wtr::OP_PIPE_FILL)) return rc;
    if (h->trn.on) if (int rc = train_op(h, wtr::OP_FEED)) return rc;   // a train program: every link from the new state
    if (h->wir.on) if (int rc = wire_restart(h)) return rc;             // a wire program: its counters from the start
    HIP_TRY(hipStreamSynchronize(h->stream));   // the caller's buffers are free on return
    h->have_state = true;
    return WT_OK;
}

int wt_ensemble_set_boundary(wt_ensemble *h, const double *bc)
{
    if (!h || !bc) return fail(WT_E_ARG, "NULL argument");
    // the bytes the device already holds: nothing to do, no device call at all (the drop-in's step() sends its
    // boundary with every call)
    if (h->bc_known && std::memcmp(bc, h->bc_sent.data(), sizeof(double) * h->bc_sent.size()) == 0) return WT_OK;
    const int rc = upload_boundary(h, bc);
    if (rc != WT_OK) h->bc_known = false;
    return rc;
}

} // extern "C"

namespace {

// Steps [first, first + n_steps) of a call of `total` outer steps (first > 0 only where a forced / recorded call runs
// one outer step per launch, see run_steps): the launches of the schedule in force, queued on the handle's stream.
int queue_steps(wt_ensemble *h, double dt, int n_steps, int fused, int first, int total)
{
    // chunk_steps: PLC scan interval; under the stream schedule also the launch length
    const int chunk = fused ? (h->chunk_steps > 0 ? h->chunk_steps : total) : 1;
    if (h->wave_diag)
        HIP_TRY(hipMemsetAsync(h->wave_diag, 0, sizeof(int64_t) * wt::WT_DIAG_SLOTS * (size_t)h->n_groups, h->stream));
    // (the stream schedule feeds the cost history too; only the queue schedule re-deals)
    struct CountSteps { wt_ensemble *h; int n; ~CountSteps() { if (h->placement == WT_PLACE_ADAPTIVE && h->sched_mode != WT_SCHED_QUEUE) h->cost_steps += n; } } count_steps{h, n_steps};
    if (h->sched_mode == WT_SCHED_QUEUE) {
        // One launch of q_workers worker wavefronts (more than one only if the call is so long that the queue's
        // 32-bit tickets -- one per work item -- could run out: groups x items per launch stays below 2^30).
        const int W = h->q_workers > 0 ? h->q_workers : 1;
        const int item = queue_item_steps(h, n_steps);
        // Reactors of similar solver cost share a wavefront: once the cost history covers enough outer steps to tell
        // a reactor's regime from a burst, the slots are re-dealt in cost order (three small kernels, no sync).
        const int64_t min_steps = h->knob_place_min > 0 ? h->knob_place_min : WT_PLACE_MIN_STEPS;
        auto redeal = [&]() {
            if (h->placement != WT_PLACE_ADAPTIVE || h->cost_steps < min_steps) return;
            const int unit = h->trn.on ? h->trn.length : 1;      // a train program: whole trains are dealt
            const int blocks = (int)((h->N / unit + wtpl::CHUNK - 1) / wtpl::CHUNK);
            const wtpl::PlaceArgs pa{h->N, h->cost, (int)(h->cost_steps > 0x7fffffff ? 0x7fffffff : h->cost_steps), h->place_hist, h->perm, unit};
            hipLaunchKernelGGL(wtpl::place_count_kernel, dim3(blocks), dim3(wtpl::BINS), 0, h->stream, pa);
            hipLaunchKernelGGL(wtpl::place_scan_kernel, dim3(1), dim3(wtpl::BINS), 0, h->stream, pa, blocks);
            hipLaunchKernelGGL(wtpl::place_scatter_kernel, dim3(blocks), dim3(wtpl::BINS), 0, h->stream, pa);
            h->cost_steps = 0; h->redeals++;
        };
        const int64_t tickets = h->knob_tickets > 0 ? h->knob_tickets : (int64_t)1 << 30;
        int64_t per_launch = tickets / h->n_groups * item;
        if (per_launch < item) per_launch = item;
        if (h->n_groups <= W && h->knob_tickets <= 0) {
            // every group has a worker of its own: nothing to hand over, so no queue -- one plain launch in which
            // workgroup g advances group g by the whole call (the drop-in's N = 1 lives here: one kernel per step())
            redeal();
            const wt::StepArgs a = make_args(h, dt, n_steps, first, total, chunk);
            launch_step(h, a, (unsigned)h->n_groups, h->stream);
            if (h->placement == WT_PLACE_ADAPTIVE) h->cost_steps += n_steps;
            HIP_TRY(hipGetLastError());
            return WT_OK;
        }
        for (int64_t done = 0; done < n_steps; done += per_launch) {
            const int cnt = (int)((n_steps - done < per_launch) ? n_steps - done : per_launch);
            redeal();
            wt::StepArgs a = make_args(h, dt, cnt, first + (int)done, total, chunk);
            a.q_ctrl = h->q_ctrl; a.q_slots = h->q_slots; a.q_next = h->q_next; a.q_cap = h->q_cap; a.item_steps = item;
            wt::QueueResetArgs qr{h->q_ctrl, h->q_slots, h->q_next, (int)h->n_groups, h->q_cap};
            hipLaunchKernelGGL(wt::queue_reset_kernel, dim3((unsigned)((h->q_cap + 255) / 256)), dim3(256), 0, h->stream, qr);
            launch_step(h, a, (unsigned)W, h->stream);
            const wt::QueueCheckArgs qc{h->q_ctrl, h->q_next, (int)h->n_groups, cnt, h->q_sticky};
            hipLaunchKernelGGL(wt::queue_check_kernel, dim3((unsigned)((h->n_groups + 255) / 256)), dim3(256), 0, h->stream, qc);
            if (h->placement == WT_PLACE_ADAPTIVE) h->cost_steps += cnt;
        }
        HIP_TRY(hipGetLastError());
        return WT_OK;
    }
    const int S = h->n_sub;
    if (S <= 1) {
        for (int done = 0; done < n_steps; done += chunk) {
            const wt::StepArgs a = make_args(h, dt, (n_steps - done < chunk) ? n_steps - done : chunk, first + done, total, chunk);
            launch_step(h, a, (unsigned)h->n_groups, h->stream);
        }
        HIP_TRY(hipGetLastError());
        return WT_OK;
    }
    for (int s = 0; s < S; ++s) {   // streams of the ranges are created on first use
        if (!h->sub_stream[s]) {
            HIP_TRY(hipStreamCreateWithFlags(&h->sub_stream[s], hipStreamNonBlocking));
            HIP_TRY(hipEventCreateWithFlags(&h->sub_done[s], hipEventDisableTiming));
        }
    }
    // fork: every range's stream waits for what is already queued on the handle's stream
    HIP_TRY(hipEventRecord(h->ev_fork, h->stream));
    for (int s = 0; s < S; ++s) HIP_TRY(hipStreamWaitEvent(h->sub_stream[s], h->ev_fork, 0));
    const int64_t groups = h->n_groups;   // wavefront-sized groups of reactors
    for (int done = 0; done < n_steps; done += chunk) {
        wt::StepArgs a = make_args(h, dt, (n_steps - done < chunk) ? n_steps - done : chunk, first + done, total, chunk);
        for (int s = 0; s < S; ++s) {
            const int64_t g0 = groups * s / S, g1 = groups * (s + 1) / S;
            a.r0 = g0 * h->R; a.r1 = (g1 * h->R < h->N) ? g1 * h->R : h->N;
            if (a.r1 > a.r0) launch_step(h, a, (unsigned)(g1 - g0), h->sub_stream[s]);
        }
    }
    HIP_TRY(hipGetLastError());
    // join: later work on the handle's stream (copies, timers) sees every range finished
    for (int s = 0; s < S; ++s) {
        HIP_TRY(hipEventRecord(h->sub_done[s], h->sub_stream[s]));
        HIP_TRY(hipStreamWaitEvent(h->stream, h->sub_done[s], 0));
    }
    return WT_OK;
}

// A step call: the launches, trajectory records where the kernel does not write them itself, the record count.
int run_steps(wt_ensemble *h, double dt, int n_steps, int fused)
{
    const bool rec = recording_open(h);
    int rc = WT_OK;
    // the command path, a disturbance program and a train program write the boundary block inside the launches
    if (h->sens.plc_on | h->dst.on | h->trn.on) h->bc_known = false;
    if ((h->call_sched || rec) && !wt::x_in_item(levels_for(h->n))) {
        // the n > 32 kernel neither reloads the schedule nor records inside a work item: one outer step per launch
        // (each starts from its own schedule row), a record copied from the state in memory after the steps that want one
        for (int s = 0; s < n_steps && rc == WT_OK; ++s) {
            rc = queue_steps(h, dt, 1, fused, s, n_steps);
            const int64_t m = h->rec.steps + s + 1;
            if (rc == WT_OK && rec && m % h->rec.every == 0 && m / h->rec.every <= h->rec.cap) {
                const int64_t o = (m / h->rec.every - 1) * h->N;
                const wt::RecordCopyArgs ca{0, h->N, h->n, h->pH, h->Cl, h->T, h->time, h->flow, h->status,
                                            h->rec.pH + o * h->n, h->rec.Cl + o * h->n, h->rec.T + o * h->n,
                                            h->rec.time + o, h->rec.flow + o, h->rec.status + o};
                const int64_t cnt = h->N * h->n;
                hipLaunchKernelGGL(wt::record_copy_kernel, dim3((unsigned)((cnt + 255) / 256)), dim3(256), 0, h->stream, ca);
                HIP_TRY(hipGetLastError());
            }
        }
    } else {
        rc = queue_steps(h, dt, n_steps, fused, 0, n_steps);
    }
    if (rc == WT_OK && h->rec.pH) h->rec.steps += n_steps;
    if (rc == WT_OK && h->scr.on) h->scr_steps += n_steps;
    return rc;
}

// ---- the installation records of the sensor suite (wt_ins.hpp)

static_assert(WT_NINS == wtin::NINS && WT_INS_LINE_VOLUME_INLET == wtin::P_LINE_VOLUME_INLET &&
              WT_INS_LINE_FLOW_OUTLET == wtin::P_LINE_FLOW_OUTLET && WT_INS_FLOW_VELOCITY == wtin::P_FLOW_VELOCITY &&
              WT_INS_AIR_BUBBLE_FREQUENCY == wtin::P_AIR_BUBBLE_FREQUENCY && WT_INS_GROUNDING_QUALITY == wtin::P_GROUNDING_QUALITY &&
              WT_INS_PIPE_VIBRATION_G == wtin::P_PIPE_VIBRATION_G && WT_INS_AMBIENT_TEMPERATURE == wtin::P_AMBIENT_TEMPERATURE,
              "installation blocks of the C ABI");
static_assert(wts::RING == 100, "the ring bound of install_error is the reference's 100-entry buffer");

const char *const k_install_fields[wtin::NINS] = {"inlet_line_volume_mL", "inlet_line_flow_mL_min", "outlet_line_volume_mL",
                                                  "outlet_line_flow_mL_min", "flow_velocity", "air_bubble_frequency",
                                                  "grounding_quality", "pipe_vibration_g", "ambient_temperature"};
// create_realistic_sensor_suite's build (sensors/__init__.py:53-67)
constexpr double k_install_defaults[wtin::NINS] = {250.0, 500.0, 250.0, 500.0, 0.5, 0.0, 0.9, 0.1, 30.0};

// SampleLine.__post_init__ (base_sensor.py:167-171), in its order of operations
double line_delay(double volume_mL, double flow_mL_min)
{
    const double volume_L = volume_mL / 1000.0;
    const double flow_L_s = flow_mL_min / 1000.0 / 60.0;
    return flow_L_s > 0 ? volume_L / flow_L_s : 0.0;
}

// The first refusal of a [WT_NINS][N] block, reactor by reactor and at one reactor in the order of the header's list;
// empty when the block passes.
std::string install_error(int64_t N, const double *p)
{
    const auto at = [&](int k, int64_t r) { return p[(int64_t)k * N + r]; };
    const auto bad = [&](int k, int64_t r, const char *rule) {
        return std::string(k_install_fields[k]) + " " + rule + " (reactor " + std::to_string(r) + ")";
    };
    for (int64_t r = 0; r < N; ++r) {
        for (int k = 0; k < wtin::NINS; ++k)
            if (!std::isfinite(at(k, r))) return bad(k, r, "must be finite");
        for (int k = wtin::P_LINE_VOLUME_INLET; k <= wtin::P_LINE_FLOW_OUTLET; ++k)
            if (at(k, r) < 0.0) return bad(k, r, "must be >= 0");
        for (int line = 0; line < 2; ++line) {
            // SampleLine sizes its buffer max(100, int(delay) + 10) (base_sensor.py:174); the device's ring holds 100
            const double delay = line_delay(at(2 * line, r), at(2 * line + 1, r));
            if (!(delay < 91.0))
                return bad(2 * line, r, "and flow give a delay of 91 s or more: the reference's buffer grows beyond 100 entries "
                                        "(int(delay) + 10 > 100), the device's ring does not");
        }
        if (!(at(wtin::P_FLOW_VELOCITY, r) >= 0.0 && at(wtin::P_FLOW_VELOCITY, r) <= 5.0)) return bad(wtin::P_FLOW_VELOCITY, r, "must be in 0..5 m/s");
        if (at(wtin::P_AIR_BUBBLE_FREQUENCY, r) < 0.0) return bad(wtin::P_AIR_BUBBLE_FREQUENCY, r, "must be >= 0");
        if (!(at(wtin::P_GROUNDING_QUALITY, r) >= 0.0 && at(wtin::P_GROUNDING_QUALITY, r) <= 1.0))
            return bad(wtin::P_GROUNDING_QUALITY, r, "must be in 0..1");
        if (at(wtin::P_PIPE_VIBRATION_G, r) < 0.0) return bad(wtin::P_PIPE_VIBRATION_G, r, "must be >= 0");
    }
    return std::string();
}

// The device records of a checked [WT_NINS][N] block (nullptr: the defaults for every reactor).  Delays, the bubble
// probability and the threshold decisions are taken here, in fp64 on the doubles as given.
std::vector<double> install_records(int64_t N, const double *p)
{
    std::vector<double> rec((size_t)N * wtin::REC_DOUBLES, 0.0);
    for (int64_t r = 0; r < N; ++r) {
        double *q = rec.data() + r * wtin::REC_DOUBLES;
        double *c = q + wtin::R_PARAMS;
        for (int k = 0; k < wtin::NINS; ++k) c[k] = p ? p[(int64_t)k * N + r] : k_install_defaults[k];
        q[wtin::R_DELAY_INLET] = line_delay(c[wtin::P_LINE_VOLUME_INLET], c[wtin::P_LINE_FLOW_INLET]);
        q[wtin::R_DELAY_OUTLET] = line_delay(c[wtin::P_LINE_VOLUME_OUTLET], c[wtin::P_LINE_FLOW_OUTLET]);
        q[wtin::R_BUBBLE_P] = c[wtin::P_AIR_BUBBLE_FREQUENCY] / 60.0;                       // base_sensor.py:490
        const int flags = (c[wtin::P_FLOW_VELOCITY] < 0.1 ? wtin::F_STAGNANT : 0) | (c[wtin::P_AIR_BUBBLE_FREQUENCY] > 0 ? wtin::F_BUBBLES : 0) |
                          (c[wtin::P_GROUNDING_QUALITY] < 0.8 ? wtin::F_GROUND : 0) | (c[wtin::P_PIPE_VIBRATION_G] > 0.2 ? wtin::F_VIBRATION : 0);
        q[wtin::R_FLAGS] = (double)flags;
        q[wtin::R_GROUND_SCALE] = 2.0 - c[wtin::P_GROUNDING_QUALITY];                        // :496
        q[wtin::R_VIBRATION] = c[wtin::P_PIPE_VIBRATION_G];
        q[wtin::R_AMBIENT] = c[wtin::P_AMBIENT_TEMPERATURE];
    }
    return rec;
}

// The records on the device and both lines' cursors back to 0: a changed delay may move a line's target backwards, and
// a walk from the oldest entry is always right (Line::transport).  The stream is idle; synchronises.
int install_load(wt_ensemble *h, const double *params, int on)
{
    const std::vector<double> rec = install_records(h->N, params);
    HIP_TRY(hipMemcpyAsync((double *)h->ins.par, rec.data(), sizeof(double) * rec.size(), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipMemsetAsync(h->sens.ring_cursor, 0, sizeof(int32_t) * 2 * (size_t)h->N, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));   // the host vector is freed on return
    h->ins.on = on;
    return WT_OK;
}

} // namespace

extern "C" {

int wt_ensemble_step(wt_ensemble *h, double dt, int n_steps, int fused)
{
    if (!h) return fail(WT_E_ARG, "NULL handle");
    if (!h->have_state || !h->have_bc) return fail(WT_E_STATE, "set_state and set_boundary must precede step");
    if (!(dt > 0)) return fail(WT_E_ARG, "`max_step` must be positive."); // scipy validate_max_step (reactor.py:480)
    if (n_steps < 0) return fail(WT_E_ARG, "n_steps must be >= 0");
    if (n_steps == 0) return WT_OK;
    HIP_TRY(hipSetDevice(h->device));
    return run_steps(h, dt, n_steps, fused);
}

int wt_ensemble_step_scheduled(wt_ensemble *h, double dt, int n_steps, int fused, const double *bc_schedule)
{
    if (!h) return fail(WT_E_ARG, "NULL handle");
    if (!bc_schedule) return fail(WT_E_ARG, "bc_schedule is NULL");
    if (h->sens.plc_on) return fail(WT_E_STATE, "a boundary schedule cannot be combined with plant I/O (the command path owns the boundary)");
    if (h->dst.on) return fail(WT_E_STATE, "a boundary schedule cannot be combined with a disturbance program (its STEP and RAMP slots script events)");
    if (h->trn.on) return fail(WT_E_STATE, "a boundary schedule cannot be combined with a train program (the run itself sets the linked rows)");
    if (!h->have_state) return fail(WT_E_STATE, "set_state must precede step");
    if (!(dt > 0)) return fail(WT_E_ARG, "`max_step` must be positive."); // scipy validate_max_step (reactor.py:480)
    if (n_steps < 0) return fail(WT_E_ARG, "n_steps must be >= 0");
    if (n_steps == 0) return WT_OK;
    int64_t row = 0, bytes = 0;
    if (__builtin_mul_overflow((int64_t)WT_NB, h->N, &row) || __builtin_mul_overflow(row, (int64_t)n_steps, &bytes) ||
        __builtin_mul_overflow(bytes, (int64_t)sizeof(double), &bytes))
        return fail(WT_E_ARG, "boundary schedule size overflows int64");
    HIP_TRY(hipSetDevice(h->device));
    if ((size_t)bytes > h->sched_bytes) {    // grown here, never inside the launch path
        HIP_TRY(hipStreamSynchronize(h->stream));
        free_and_null(h->sched); h->sched_bytes = 0;
        HIP_TRY(hipMalloc((void **)&h->sched, (size_t)bytes));
        h->sched_bytes = (size_t)bytes;
    }
    // ordered after the launches of an earlier call that still read the buffer; the caller's array is free on return
    HIP_TRY(hipMemcpyAsync(h->sched, bc_schedule, (size_t)bytes, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    h->call_sched = h->sched;
    const int rc = run_steps(h, dt, n_steps, fused);
    h->call_sched = nullptr;
    if (rc != WT_OK) return rc;
    // the boundary block is the last row from now on (get_boundary, rhs, later plain step calls, and a set_boundary
    // of that row, which finds it there)
    h->bc_known = false;
    HIP_TRY(hipMemcpyAsync(h->bc, h->sched + (size_t)(n_steps - 1) * (size_t)row, sizeof(double) * (size_t)row,
                           hipMemcpyDeviceToDevice, h->stream));
    const double *last = bc_schedule + (size_t)(n_steps - 1) * (size_t)row;
    h->bc_sent.assign(last, last + row);
    h->bc_known = true;
    h->have_bc = true;
    return WT_OK;
}

int wt_ensemble_record(wt_ensemble *h, int every, int capacity)
{
    if (!h) return fail(WT_E_ARG, "NULL handle");
    if (every < 1) return fail(WT_E_ARG, "every must be >= 1");
    if (capacity < 0) return fail(WT_E_ARG, "capacity must be >= 0 (0 = recording off)");
    int64_t per = 0, zone = 0;
    if (__builtin_mul_overflow((int64_t)capacity, h->N, &per) || __builtin_mul_overflow(per, (int64_t)h->n, &zone) ||
        __builtin_mul_overflow(zone, (int64_t)sizeof(double), &zone) || __builtin_mul_overflow(per, (int64_t)sizeof(double), &per))
        return fail(WT_E_ARG, "record size overflows int64");
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipStreamSynchronize(h->stream));   // queued launches may still write the old records
    release(record_arrays(h));
    if (capacity == 0) return WT_OK;
    h->rec.every = every; h->rec.cap = capacity;
    return allocate(record_arrays(h));
}

int wt_ensemble_get_record(wt_ensemble *h, double *pH, double *Cl, double *T, double *time, double *flow,
                           uint32_t *status, int *n_records)
{
    if (!h) return fail(WT_E_ARG, "NULL handle");
    if (!h->rec.pH) return fail(WT_E_STATE, "recording is off (wt_ensemble_record)");
    HIP_TRY(hipSetDevice(h->device));
    const int64_t done = h->rec.steps / h->rec.every;
    const int64_t nr = done < h->rec.cap ? done : h->rec.cap;
    const size_t per = (size_t)nr * (size_t)h->N, zone = sizeof(double) * per * (size_t)h->n;
    if (n_records) *n_records = (int)nr;
    return download(h, {{pH, h->rec.pH, zone}, {Cl, h->rec.Cl, zone}, {T, h->rec.T, zone}, {time, h->rec.time, sizeof(double) * per},
                        {flow, h->rec.flow, sizeof(double) * per}, {status, h->rec.status, sizeof(uint32_t) * per}});
}

int wt_ensemble_launch_timing(wt_ensemble *h, int enable)
{
    if (!h) return fail(WT_E_ARG, "NULL handle");
    h->time_launches = enable != 0;
    h->lt_used = 0;
    // the first few event pairs exist before the timed region starts (event creation is not part of a launch)
    while (enable && h->lt_pool.size() < 16) {
        hipEvent_t e;
        if (hipEventCreate(&e) != hipSuccess) break;
        h->lt_pool.push_back(e);
    }
    return WT_OK;
}

int wt_ensemble_launch_stats(wt_ensemble *h, int64_t *n_launches, double *sum_ms, double *max_ms)
{
    if (!h || !n_launches || !sum_ms || !max_ms) return fail(WT_E_ARG, "NULL argument");
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipStreamSynchronize(h->stream));
    double sum = 0.0, mx = 0.0;
    for (size_t i = 0; i + 1 < h->lt_used; i += 2) {
        float ms = 0.f;
        HIP_TRY(hipEventSynchronize(h->lt_pool[i + 1]));
        HIP_TRY(hipEventElapsedTime(&ms, h->lt_pool[i], h->lt_pool[i + 1]));
        sum += ms; if (ms > mx) mx = ms;
    }
    *n_launches = (int64_t)(h->lt_used / 2); *sum_ms = sum; *max_ms = mx;
    h->lt_used = 0;
    return WT_OK;
}

int wt_ensemble_sensors_enable(wt_ensemble *h, uint64_t seed, int64_t reactor_base, const double *cfg_flow,
                               const double *cfg_chlorine, const double *cfg_temperature, int history_capacity)
{
    if (!h || !cfg_flow || !cfg_chlorine || !cfg_temperature) return fail(WT_E_ARG, "NULL argument");
    if (history_capacity < 0) return fail(WT_E_ARG, "history_capacity must be >= 0");
    if (h->sens.on) return fail(WT_E_STATE, "sensor suite already enabled");
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipStreamSynchronize(h->stream));
    const size_t N = (size_t)h->N, hist = (size_t)history_capacity * wts::NSENS * N;
    wts::SuiteArgs &s = h->sens;
    double *cfg = nullptr;
    HIP_TRY(hipMalloc((void **)&cfg, sizeof(double) * 3 * N));
    s.hist_cap = history_capacity;
    const ArrayGroup arrays = sensor_arrays(h);
    if (int rc = allocate(arrays)) { (void)hipFree(cfg); return rc; }
    if (history_capacity > 0) {
        // slots that are never written (a reactor whose step raised takes no reading) must not hold garbage
        (void)hipMemsetAsync(s.hist_value, 0, sizeof(float) * hist, h->stream);
        (void)hipMemsetAsync(s.hist_status, 0, hist, h->stream);
        (void)hipMemsetAsync(s.hist_fault, 0, hist, h->stream);
    }
    hipError_t e = hipMemcpy(cfg, cfg_flow, sizeof(double) * N, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(cfg + N, cfg_chlorine, sizeof(double) * N, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(cfg + 2 * N, cfg_temperature, sizeof(double) * N, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpyAsync((double *)s.t_enable, h->time, sizeof(double) * N, hipMemcpyDeviceToDevice, h->stream);
    if (e == hipSuccess) e = hipMemsetAsync(s.ring_t, 0, sizeof(double) * 2 * wts::RING * N, h->stream);
    if (e == hipSuccess) e = hipMemsetAsync(s.ring_v, 0, sizeof(float) * 2 * wts::RING * N, h->stream);
    // the service program's records, off: no slot enabled, no state (a checkpoint holds them whether or not one is set)
    if (e == hipSuccess) e = hipMemsetAsync((void *)s.svc_par, 0, sizeof(double) * wtsv::PAR_DOUBLES * N, h->stream);
    if (e == hipSuccess) e = hipMemsetAsync(s.svc_st, 0, sizeof(double) * wtsv::ST_DOUBLES * N, h->stream);
    // the installation records: the suite's own build for every reactor, off (the copy is from pageable memory: the
    // vector is free once the call returns)
    const std::vector<double> inst = install_records(h->N, nullptr);
    if (e == hipSuccess) e = hipMemcpy((double *)h->ins.par, inst.data(), sizeof(double) * inst.size(), hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        wts::SensorInitArgs a;
        a.N = h->N; a.cfg_flow = cfg; a.cfg_cl = cfg + N; a.cfg_temp = cfg + 2 * N;
        a.fs = s.fs; a.ds = s.ds; a.is = s.is; a.full_scale = s.full_scale;
        a.ring_push = s.ring_push; a.ring_cursor = s.ring_cursor;
        a.out_value = s.out_value; a.out_status = s.out_status; a.out_fault = s.out_fault; a.hist_pos = s.hist_pos;
        hipLaunchKernelGGL(wts::sensor_init_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, h->stream, a);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    (void)hipFree(cfg);
    if (e != hipSuccess) { release(arrays); return fail(WT_E_HIP, std::string("sensors_enable: ") + hipGetErrorString(e)); }
    s.seed_lo = (uint32_t)(seed & 0xffffffffu); s.seed_hi = (uint32_t)(seed >> 32); s.reactor_base = reactor_base;
    s.svc_on = 0;                                // a freshly enabled suite has no service program
    h->ins.on = 0;                               // and no installation
    s.on = 1;
    return WT_OK;
}

int wt_ensemble_sensors_get(wt_ensemble *h, float *values, uint8_t *status, uint8_t *fault)
{
    if (!h) return fail(WT_E_ARG, "NULL handle");
    if (!h->sens.on) return fail(WT_E_STATE, "sensor suite not enabled");
    HIP_TRY(hipSetDevice(h->device));
    const size_t cnt = (size_t)wts::NSENS * h->N;
    return download(h, {{values, h->sens.out_value, sizeof(float) * cnt}, {status, h->sens.out_status, cnt},
                        {fault, h->sens.out_fault, cnt}});
}

int wt_ensemble_sensors_history(wt_ensemble *h, float *values, uint8_t *status, uint8_t *fault, int32_t *n_filled)
{
    if (!h) return fail(WT_E_ARG, "NULL handle");
    if (!h->sens.on || h->sens.hist_cap <= 0) return fail(WT_E_STATE, "sensor history not enabled");
    HIP_TRY(hipSetDevice(h->device));
    const size_t cnt = (size_t)h->sens.hist_cap * wts::NSENS * h->N;
    return download(h, {{values, h->sens.hist_value, sizeof(float) * cnt}, {status, h->sens.hist_status, cnt},
                        {fault, h->sens.hist_fault, cnt}, {n_filled, h->sens.hist_pos, sizeof(int32_t) * h->N}});
}

int wt_ensemble_plc_enable(wt_ensemble *h)
{
    if (!h) return fail(WT_E_ARG, "NULL handle");
    if (!h->sens.on) return fail(WT_E_STATE, "the register image publishes sensor readings: enable the sensor suite first");
    if (h->sens.plc_on) return fail(WT_E_STATE, "plant I/O already enabled");
    HIP_TRY(hipSetDevice(h->device));
    const size_t N = (size_t)h->N;
    {
        std::vector<uint32_t> jw;
        if (int rc = junction_words(h, jw)) return rc;
        for (const uint32_t w : jw) if (w & wtr::JCT_CARRY) return fail(WT_E_STATE, k_junction_plant_io);
    }
    const ArrayGroup arrays = plant_io_arrays(h);
    if (int rc = allocate(arrays)) return rc;
    wtp::PackArgs &p = h->sens.pack;
    // ModbusSequentialDataBlock(0, [0] * size): every register starts at 0 (slave.py:134-137); sim_time = 0.0
    hipError_t e = hipMemsetAsync(p.ir, 0, sizeof(uint16_t) * wtp::IR_WORDS * N, h->stream);
    if (e == hipSuccess) e = hipMemsetAsync(h->ctl.hr, 0, sizeof(uint16_t) * wtp::HR_WORDS * N, h->stream);
    if (e == hipSuccess) e = hipMemsetAsync(p.loop_time, 0, sizeof(double) * N, h->stream);
    if (e == hipSuccess) e = hipMemsetAsync(p.update_ok, 1, N, h->stream);
    // the tune program's records, off: no loop enabled, no state (a checkpoint holds them whether or not one is set)
    if (e == hipSuccess) e = hipMemsetAsync((void *)h->tun.par, 0, sizeof(double) * wtu::PAR_DOUBLES * N, h->stream);
    if (e == hipSuccess) e = hipMemsetAsync(h->tun.st, 0, sizeof(double) * wtu::ST_DOUBLES * N, h->stream);
    // the model predictive controllers' arrays likewise
    if (e == hipSuccess) e = hipMemsetAsync((void *)h->mpc.par, 0, sizeof(double) * wtm::PAR_DOUBLES * N, h->stream);
    if (e == hipSuccess) e = hipMemsetAsync(h->mpc.st, 0, sizeof(double) * wtm::ST_DOUBLES * N, h->stream);
    if (e == hipSuccess) e = hipMemsetAsync((void *)h->mpc.step, 0, sizeof(double) * wtm::ROW_DOUBLES * N, h->stream);
    if (e == hipSuccess) e = hipMemsetAsync((void *)h->mpc.gain, 0, sizeof(double) * wtm::ROW_DOUBLES * N, h->stream);
    if (e == hipSuccess) e = hipMemsetAsync(h->mpc.pred, 0, sizeof(double) * wtm::ROW_DOUBLES * N, h->stream);
    // and the response programs' records: every slot off
    if (e == hipSuccess) e = hipMemsetAsync((void *)h->rsp.par, 0, sizeof(double) * wtrp::PAR_DOUBLES * N, h->stream);
    if (e == hipSuccess) e = hipMemsetAsync(h->rsp.st, 0, sizeof(double) * wtrp::ST_DOUBLES * N, h->stream);
    if (e == hipSuccess) e = hipMemsetAsync(h->rsp.rst, 0, sizeof(double) * wtrp::RST_DOUBLES * N, h->stream);
    // and the link programs' records and rings: every slot off
    if (e == hipSuccess) e = hipMemsetAsync((void *)h->lnk.par, 0, sizeof(double) * wtl::PAR_DOUBLES * N, h->stream);
    if (e == hipSuccess) e = hipMemsetAsync(h->lnk.st, 0, sizeof(double) * wtl::ST_DOUBLES * N, h->stream);
    if (e == hipSuccess) e = hipMemsetAsync(h->lnk.ring, 0, sizeof(double) * wtl::RING_ENTRIES * N, h->stream);
    if (e == hipSuccess) e = hipMemsetAsync(h->lnk.fring, 0, sizeof(uint8_t) * wtl::RING_ENTRIES * N, h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess) { release(arrays); return fail(WT_E_HIP, std::string("plc_enable: ") + hipGetErrorString(e)); }
    h->sens.cmd.hr = h->ctl.hr;
    h->tun.on = 0;                               // freshly enabled plant I/O has no tune program
    h->mpc.on = 0;                               // and no model predictive controller
    h->rsp.on = 0;                               // and no response program
    h->lnk.on = 0; h->lnk.seed_lo = h->lnk.seed_hi = 0;   // and no link program
    h->sens.plc_on = 1;
    return WT_OK;
}

int wt_ensemble_plc_write_holding(wt_ensemble *h, const uint16_t *words, int64_t first_reactor, int64_t count)
{
    if (!h || !words) return fail(WT_E_ARG, "NULL argument");
    if (!h->sens.plc_on) return fail(WT_E_STATE, "plant I/O not enabled");
    if (first_reactor < 0 || count < 0 || first_reactor + count > h->N) return fail(WT_E_ARG, "reactor range outside the ensemble");
    if (count == 0) return WT_OK;
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipMemcpyAsync(h->ctl.hr + first_reactor * wtp::HR_WORDS, words, sizeof(uint16_t) * wtp::HR_WORDS * (size_t)count,
                           hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));   // the caller's buffer is free on return
    return WT_OK;
}

int wt_ensemble_plc_read_inputs(wt_ensemble *h, uint16_t *words, uint8_t *update_ok)
{
    if (!h) return fail(WT_E_ARG, "NULL handle");
    if (!h->sens.plc_on) return fail(WT_E_STATE, "plant I/O not enabled");
    HIP_TRY(hipSetDevice(h->device));
    return download(h, {{words, h->sens.pack.ir, sizeof(uint16_t) * wtp::IR_WORDS * (size_t)h->N},
                        {update_ok, h->sens.pack.update_ok, (size_t)h->N}});
}

int wt_ensemble_plc_device(wt_ensemble *h, void **input_image, void **holding_image)
{
    if (!h) return fail(WT_E_ARG, "NULL handle");
    if (!h->sens.plc_on) return fail(WT_E_STATE, "plant I/O not enabled");
    if (input_image) *input_image = h->sens.pack.ir;
    if (holding_image) *holding_image = h->ctl.hr;
    return WT_OK;
}

} // extern "C"

namespace {

// ---- The per-reactor programs: one description each, one lifecycle for all ----

static_assert(WT_CTL_LOOPS == wtc::LOOPS && WT_NC == wtc::NC && WT_NCS == wtc::NCS, "control blocks of the C ABI");

static_assert(WT_INJ_SLOTS == wti::SLOTS && WT_NI == wti::NI && WT_NIS == wti::NIS, "injection blocks of the C ABI");
static_assert(WT_INJ_N_TARGETS == wti::N_TARGETS && WT_INJ_CMD_ACID == wti::CMD_ACID && WT_INJ_CMD_CHLORINE == wti::CMD_CHLORINE &&
              WT_INJ_CMD_INLET == wti::CMD_INLET && WT_INJ_FAULT == wti::M_FAULT && WT_INJ_FAULT + 1 == wti::N_MODES,
              "injection targets and modes of the C ABI");

static_assert(WT_ALM_SLOTS == wta::SLOTS && WT_NA == wta::NA && WT_NAS == wta::NAS && WT_NAR == wta::NAR, "alarm blocks of the C ABI");
static_assert(WT_ALM_HIGH == wta::K_HIGH && WT_ALM_LOW == wta::K_LOW && WT_ALM_FIELD == wta::SRC_FIELD &&
              WT_ALM_ALARM == wta::ON_BAD_ALARM && WT_ALM_TRIP_ACID == wta::ACT_TRIP_ACID &&
              WT_ALM_TRIP_CHLORINE == wta::ACT_TRIP_CHLORINE && WT_ALM_TRIP_CHLORINE + 1 == wta::N_ACTIONS,
              "alarm kinds, sources and actions of the C ABI");
static_assert(WT_A_TRIP_VALUE == wta::A_TRIP_VALUE && WT_AS_N_BAD == wta::AS_N_BAD && WT_AR_N_OVR_CHLORINE == wta::AR_N_OVR_CHLORINE,
              "alarm rows of the C ABI");

static_assert(WT_ACT_CHANNELS == wtv::CH && WT_NV == wtv::NV && WT_NVS == wtv::NVS && WT_ACT_MAX_DELAY == wtv::MAX_DELAY,
              "actuator blocks of the C ABI");
static_assert(WT_ACT_ACID == wtv::CH_ACID && WT_ACT_CHLORINE == wtv::CH_CHLORINE && WT_ACT_INLET == wtv::CH_INLET &&
              WT_ACT_INLET + 7 == WT_INJ_CMD_INLET && WT_ACT_STUCK == wtv::F_STUCK && WT_ACT_FAIL_TO == wtv::F_FAIL_TO &&
              WT_ACT_FAIL_TO + 1 == wtv::N_FAULTS, "actuator channels and faults of the C ABI");
static_assert(WT_V_FAIL_VALUE == wtv::V_FAIL_VALUE && WT_VS_N_FAULT == wtv::VS_N_FAULT, "actuator rows of the C ABI");

static_assert(WT_DST_SLOTS == wtd::SLOTS && WT_ND == wtd::ND && WT_NDS == wtd::NDS && WT_NB == wtd::NB,
              "disturbance blocks of the C ABI");
static_assert(WT_DST_OU == wtd::K_OU && WT_DST_OU + 1 == wtd::N_KINDS && WT_D_C == wtd::D_C && WT_DS_N_DRAW == wtd::DS_N_DRAW,
              "disturbance kinds and rows of the C ABI");

static_assert(WT_SCR_SLOTS == wtsc::SLOTS && WT_NSP == wtsc::NSP && WT_NSS == wtsc::NSS && WT_SCR_MAX_BINS == wtsc::MAX_BINS,
              "score blocks of the C ABI");
static_assert(WT_SCR_BAND + 1 == wtsc::N_KINDS && WT_SQ_TEMPERATURE + 1 == wtsc::N_QUANTITIES && WT_SR_MEAN + 1 == wtsc::N_REDUCES &&
              WT_SP_T_END == wtsc::P_T_END && WT_SS_RUN_MAX == wtsc::S_RUN_MAX, "score kinds and rows of the C ABI");

static_assert(WT_DET_SLOTS == wtk::SLOTS && WT_NK == wtk::NK && WT_NKS == wtk::NKS && WT_NKR == wtk::NKR, "detector blocks of the C ABI");
static_assert(WT_DET_CUSUM == wtk::D_CUSUM && WT_DET_EWMA == wtk::D_EWMA && WT_DET_FLATLINE == wtk::D_FLATLINE &&
              WT_DET_FLATLINE + 1 == wtk::N_KINDS && WT_DET_FIELD == wtk::SRC_FIELD && WT_DET_SENSOR == wtk::REF_SENSOR &&
              WT_DET_TRACK == wtk::REF_TRACK && WT_DET_TRACK + 1 == wtk::N_REFS && WT_DET_ALARM == wtk::ON_BAD_ALARM,
              "detector kinds, sources, references and policies of the C ABI");
static_assert(WT_K_REF_ARG == wtk::K_REF_ARG && WT_K_ON_BAD == wtk::K_ON_BAD && WT_KS_X_PREV == wtk::KS_X_PREV &&
              WT_KS_T_DETECT == wtk::KS_T_DETECT && WT_KS_N_FN == wtk::KS_N_FN && WT_KR_LABEL_END == wtk::KR_LABEL_END,
              "detector rows of the C ABI");
static_assert(wtk::NK % 2 == 0 && wtk::NKS % 2 == 0 && wtk::NKR == 2, "the detector's records are read in 16-byte pairs");

static_assert(WT_TRD_SLOTS == wtt::SLOTS && WT_NT == wtt::NT && WT_NTS == wtt::NTS, "trend blocks of the C ABI");
static_assert(WT_TRD_IMAGE_VALUE == wtt::G_IMAGE_VALUE && WT_TRD_FIELD_FAULT == wtt::G_FIELD_FAULT && WT_TRD_COMMAND == wtt::G_COMMAND &&
              WT_TRD_CONTROL == wtt::G_CONTROL && WT_TRD_INJECT == wtt::G_INJECT && WT_TRD_ALARM == wtt::G_ALARM &&
              WT_TRD_ALARM_WORD == wtt::G_ALARM_WORD && WT_TRD_ACTUATOR == wtt::G_ACTUATOR && WT_TRD_DETECT == wtt::G_DETECT &&
              WT_TRD_DETECT + 1 == wtt::N_TAGS, "trend tags of the C ABI");
static_assert(WT_T_T_END == wtt::T_T_END && WT_TS_LAST == wtt::TS_LAST, "trend rows of the C ABI");
static_assert(wtt::NT % 2 == 0 && wtt::NTS % 2 == 0, "the recorder's records are read in 16-byte pairs");
static_assert(wtt::index_range(wtt::G_IMAGE_VALUE) == WT_N_SENSORS && wtt::index_range(wtt::G_CONTROL) == WT_CTL_LOOPS * WT_NCS &&
              wtt::index_range(wtt::G_INJECT) == WT_INJ_SLOTS * WT_NIS && wtt::index_range(wtt::G_ALARM) == WT_ALM_SLOTS * WT_NAS &&
              wtt::index_range(wtt::G_ACTUATOR) == WT_ACT_CHANNELS * WT_NVS && wtt::index_range(wtt::G_DETECT) == WT_DET_SLOTS * WT_NKS,
              "a trend index names an entry of the block the program's get call returns");
// COMMAND channels in WT_INJ_CMD_* order
static_assert(WT_INJ_CMD_ACID + 1 == WT_INJ_CMD_CHLORINE && WT_INJ_CMD_CHLORINE + 1 == WT_INJ_CMD_INLET, "acid, chlorine, inlet");

static_assert(WT_SVC_SLOTS == wtsv::SLOTS && WT_NSV == wtsv::NSV && WT_NSVS == wtsv::NSVS && WT_NSH == wtsv::NSH &&
              WT_SV_ENABLE == wtsv::V_ENABLE && WT_SV_REF2 == wtsv::V_REF2 && WT_SVS_N_DONE == wtsv::VS_N_DONE &&
              WT_SVS_T_SEEN == wtsv::VS_T_SEEN && WT_SVC_CALIBRATE == wtsv::A_CALIBRATE &&
              WT_SVC_REPLACE_REAGENT == wtsv::A_REPLACE_REAGENT && WT_SVC_ON_STATUS == wtsv::TR_ON_STATUS &&
              WT_SVC_REF_TRIM == wtsv::REF_TRIM && WT_SH_FAULT == wtsv::H_FAULT && WT_N_SENSORS == wts::NSENS,
              "service blocks of the C ABI");

static_assert(WT_TUN_LOOPS == wtu::LOOPS && WT_TUN_LOOPS == WT_CTL_LOOPS && WT_NU == wtu::NU && WT_NUS == wtu::NUS &&
              WT_TUN_ENABLE == wtu::U_ENABLE && WT_TUN_AMPLITUDE == wtu::U_AMPLITUDE && WT_TUN_COMMISSION == wtu::U_COMMISSION &&
              WT_TUNS_PHASE == wtu::US_PHASE && WT_TUNS_N_CYCLES == wtu::US_N_CYCLES && WT_TUNS_KU == wtu::US_KU &&
              WT_TUNS_COMMISSIONED == wtu::US_COMMISSIONED && WT_TUN_DONE == wtu::PH_DONE && WT_TUN_FAILED == wtu::PH_FAILED &&
              WT_TUN_MAX_CYCLES == wtu::MAX_CYCLES, "tune blocks of the C ABI");

// -- parameter rules: the checks of one slot's row vector c[fields] (slot: its index in the block); nullptr when it passes

using Rule = const char *(*)(int slot, const double *c);

bool whole_in(double x, double lo, double hi) { return x == std::floor(x) && x >= lo && x <= hi; }

const char *control_rule(int, const double *c)
{
    for (int k = 0; k < wtc::NC; ++k)
        if (!std::isfinite(c[k])) return "control parameters must be finite";
    if (c[wtc::C_ENABLE] != 0.0 && c[wtc::C_ENABLE] != 1.0) return "enable must be 0 or 1";
    if (!whole_in(c[wtc::C_SENSOR], 0, WT_N_SENSORS - 1)) return "sensor must be an integer in 0..6";
    if (c[wtc::C_DIRECTION] != 1.0 && c[wtc::C_DIRECTION] != -1.0) return "direction must be +1 or -1";
    if (!(c[wtc::C_KP] >= 0) || !(c[wtc::C_KI] >= 0)) return "kp and ki must be >= 0";
    if (!(c[wtc::C_OUT_MIN] <= c[wtc::C_OUT_MAX])) return "out_min must not exceed out_max";
    return nullptr;
}

const char *inject_rule(int, const double *c)
{
    for (int k = 0; k < wti::NI; ++k)
        if (!std::isfinite(c[k]) && !(k == wti::I_T_END && c[k] == INFINITY))
            return "injection parameters must be finite (end may be +inf)";
    const double mode = c[wti::I_MODE], target = c[wti::I_TARGET];
    if (!whole_in(mode, 0, wti::N_MODES - 1)) return "mode must be an integer in 0..7";
    if (!whole_in(target, 0, wti::N_TARGETS - 1)) return "target must be an integer in 0..9";
    if (c[wti::I_T_START] > c[wti::I_T_END]) return "start must not exceed end";
    if (mode == wti::M_FAULT) {
        if (target >= wti::CMD_ACID) return "a FAULT slot must target a sensor";
        if (!whole_in(c[wti::I_A], 1, 6)) return "a FAULT slot's fault code (a) must be an integer in 1..6";
    }
    return nullptr;
}

const char *alarm_rule(int, const double *c)
{
    for (int k = 0; k < wta::NA; ++k)
        if (!std::isfinite(c[k])) return "alarm parameters must be finite";
    if (!whole_in(c[wta::A_KIND], 0, 2)) return "kind must be 0 (off), 1 (high) or 2 (low)";
    if (!whole_in(c[wta::A_SENSOR], 0, WT_N_SENSORS - 1)) return "sensor must be an integer in 0..6";
    if (!whole_in(c[wta::A_SOURCE], 0, 1)) return "source must be 0 (image) or 1 (field)";
    if (c[wta::A_DEADBAND] < 0) return "deadband must be >= 0";
    if (c[wta::A_ON_DELAY] < 0) return "on_delay must be >= 0";
    if (!whole_in(c[wta::A_LATCH], 0, 1)) return "latch must be 0 or 1";
    if (!whole_in(c[wta::A_ON_BAD], 0, 1)) return "on_bad must be 0 (hold) or 1 (alarm)";
    if (!whole_in(c[wta::A_ACTION], 0, 2)) return "action must be 0 (none), 1 (trip_acid) or 2 (trip_chlorine)";
    const double tv = c[wta::A_TRIP_VALUE];
    if (c[wta::A_ACTION] == wta::ACT_TRIP_ACID && !(tv >= 0 && tv <= 2.0)) return "a trip_acid slot's trip_value must be in [0, 2]";
    if (c[wta::A_ACTION] == wta::ACT_TRIP_CHLORINE && !(tv >= 0 && tv <= 1.0)) return "a trip_chlorine slot's trip_value must be in [0, 1]";
    return nullptr;
}

const char *actuator_finite(int, const double *c)
{
    for (int v = 0; v < wtv::NV; ++v)
        if (!std::isfinite(c[v]) && !((v == wtv::V_RATE || v == wtv::V_T_REPAIR) && c[v] == INFINITY))
            return "actuator parameters must be finite (rate and t_repair may be +inf)";
    return nullptr;
}

const char *actuator_rule(int k, const double *c)
{
    if (!whole_in(c[wtv::V_ENABLE], 0, 1)) return "enable must be 0 or 1";
    if (!(c[wtv::V_TAU] >= 0)) return "tau must be >= 0";
    if (!(c[wtv::V_RATE] > 0)) return "rate must be > 0";
    if (!(c[wtv::V_BACKLASH] >= 0)) return "backlash must be >= 0";
    if (!whole_in(c[wtv::V_DELAY], 0, wtv::MAX_DELAY)) return "delay must be an integer in 0..8";
    if (!whole_in(c[wtv::V_FAULT], 0, 2)) return "fault must be 0 (none), 1 (stuck) or 2 (fail_to)";
    if (!(c[wtv::V_T_REPAIR] >= c[wtv::V_T_FAULT])) return "t_repair must be >= t_fault";
    if (c[wtv::V_FAULT] == wtv::F_FAIL_TO) {
        const double fv = c[wtv::V_FAIL_VALUE];
        if (k == wtv::CH_INLET && !(fv > wtv::INLET_MIN && fv <= wtv::limit_of(k)))
            return "an inlet fail_to fail_value must be in (0.1, 20]";
        if (k != wtv::CH_INLET && !(fv >= 0 && fv <= wtv::limit_of(k)))
            return "a fail_to fail_value must be in [0, limit]: 2 for acid, 1 for chlorine";
    }
    return nullptr;
}

const char *disturb_finite(int, const double *c)
{
    for (int v = 0; v < wtd::ND; ++v)
        if (!std::isfinite(c[v]) && !(v == wtd::D_T_END && c[v] == INFINITY))
            return "disturbance parameters must be finite (t_end may be +inf)";
    return nullptr;
}

const char *disturb_rule(int, const double *c)
{
    const double kind = c[wtd::D_KIND], row = c[wtd::D_ROW];
    if (!whole_in(kind, 0, wtd::N_KINDS - 1)) return "kind must be an integer in 0..4 (off, step, ramp, sine, ou)";
    if (!whole_in(row, 0, wtd::NB - 1)) return "row must be a boundary row: 1, 2, 3, 5, 7, 8 or 9";
    if (!wtd::row_allowed((int)row))
        return "rows 0, 4 and 6 (inlet, acid and chlorine flow) belong to the command path or the master";
    if (!(c[wtd::D_T_END] >= c[wtd::D_T_START])) return "t_end must be >= t_start";
    if (kind == wtd::K_SINE && !(c[wtd::D_B] > 0)) return "a sine needs b (the period) > 0";
    if (kind == wtd::K_OU && !(c[wtd::D_A] >= 0)) return "an OU slot needs a (sigma) >= 0";
    if (kind == wtd::K_OU && !(c[wtd::D_B] > 0)) return "an OU slot needs b (tau) > 0";
    return nullptr;
}

const char *score_rule(int, const double *c)
{
    if (!whole_in(c[wtsc::P_KIND], 0, wtsc::N_KINDS - 1)) return "kind must be 0 (off) or 1 (band)";
    if (!whole_in(c[wtsc::P_QUANTITY], 0, wtsc::N_QUANTITIES - 1)) return "quantity must be 0 (pH), 1 (chlorine) or 2 (temperature)";
    if (!whole_in(c[wtsc::P_REDUCE], 0, wtsc::N_REDUCES - 1)) return "reduce must be an integer in 0..3 (zone, min, max, mean)";
    if (!whole_in(c[wtsc::P_ZONE], -1, 31)) return "zone must be an integer in -1..31 (-1: the last zone, the outlet)";
    if (std::isnan(c[wtsc::P_LO]) || std::isnan(c[wtsc::P_HI])) return "lo and hi must not be NaN (-inf and +inf leave a side open)";
    if (!(c[wtsc::P_LO] <= c[wtsc::P_HI])) return "lo must be <= hi";
    if (!(c[wtsc::P_T_END] >= c[wtsc::P_T_START])) return "t_end must be >= t_start, neither NaN";
    return nullptr;
}

const char *detect_rule(int, const double *c)
{
    for (int k = 0; k < wtk::NK; ++k)
        if (!std::isfinite(c[k]) && !(k == wtk::K_T_ARM && c[k] == -INFINITY))
            return "detector parameters must be finite (t_arm may be -inf)";
    const double kind = c[wtk::K_KIND], ref = c[wtk::K_REF], slack = c[wtk::K_SLACK];
    if (!whole_in(kind, 0, wtk::N_KINDS - 1)) return "kind must be 0 (off), 1 (cusum), 2 (ewma) or 3 (flatline)";
    if (kind == wtk::D_OFF) return nullptr;                // the other rows of an OFF slot are not read
    if (!whole_in(c[wtk::K_SENSOR], 0, WT_N_SENSORS - 1)) return "sensor must be an integer in 0..6";
    if (!whole_in(c[wtk::K_SOURCE], 0, 1)) return "source must be 0 (image) or 1 (field)";
    if (!whole_in(ref, 0, wtk::N_REFS - 1)) return "ref must be 0 (const), 1 (sensor) or 2 (track)";
    if (ref == wtk::REF_SENSOR) {
        if (!whole_in(c[wtk::K_REF_ARG], 0, WT_N_SENSORS - 1)) return "a SENSOR reference's ref_arg must be a sensor index in 0..6";
        if (!whole_in(c[wtk::K_REF_SOURCE], 0, 1)) return "ref_source must be 0 (image) or 1 (field)";
    }
    if (ref == wtk::REF_TRACK && !(c[wtk::K_REF_ARG] > 0)) return "a TRACK reference's ref_arg (tau) must be > 0";
    if (!(c[wtk::K_SIGMA] > 0)) return "sigma must be > 0";
    if (kind == wtk::D_CUSUM && !(slack >= 0)) return "a CUSUM slot's slack (k) must be >= 0";
    if (kind == wtk::D_EWMA && !(slack > 0 && slack <= 1)) return "an EWMA slot's slack (lambda) must be in (0, 1]";
    if (kind == wtk::D_FLATLINE && !(slack >= 0)) return "a FLATLINE slot's slack (eps) must be >= 0";
    if (!(c[wtk::K_LIMIT] > 0)) return "limit must be > 0";
    if (!whole_in(c[wtk::K_ON_BAD], 0, 1)) return "on_bad must be 0 (hold) or 1 (alarm)";
    return nullptr;
}

const char *trend_rule(int, const double *c)
{
    const double tag = c[wtt::T_TAG];
    if (!whole_in(tag, 0, wtt::N_TAGS - 1)) return "tag must be an integer in 0..11 (0: off)";
    if (tag == wtt::G_OFF) return nullptr;                 // the other rows of an OFF slot are not read
    if (!whole_in(c[wtt::T_INDEX], 0, wtt::index_range((int)tag) - 1)) return "index must be an integer within the tag's range";
    if (!whole_in(c[wtt::T_EVERY], 1, 9007199254740991.0)) return "every must be an integer >= 1";   // whole numbers below 2^53
    if (std::isnan(c[wtt::T_DEADBAND])) return "deadband must not be NaN (negative: every candidate is recorded)";
    if (std::isnan(c[wtt::T_T_START]) || std::isnan(c[wtt::T_T_END])) return "t_start and t_end must not be NaN";
    if (!(c[wtt::T_T_END] >= c[wtt::T_T_START])) return "t_end must be >= t_start";
    return nullptr;
}

const char *k_service_no_suite = "the sensor suite is not enabled (wt_ensemble_sensors_enable)";

// what the reference would raise for, and the codes: an action on a sensor with a reference mode
// (wt_ensemble_sensors_service checks its arguments with it too)
const char *service_action_error(double sensor, double action, double ref_mode)
{
    if (!whole_in(sensor, 0, WT_N_SENSORS - 1)) return "sensor must be an integer in 0..6";
    if (!whole_in(action, 0, wtsv::N_ACTIONS - 1)) return "action must be an integer in 0..6";
    if (!whole_in(ref_mode, 0, wtsv::N_REF_MODES - 1)) return "ref_mode must be 0 (constant), 1 (sample) or 2 (trim)";
    const int a = (int)action;
    if (a >= wtsv::A_TWO_POINT && a <= wtsv::A_PEPSIN_CLEAN && sensor > 1.0)
        return "two-point calibration and cleaning are for the pH sensors (0, 1)";
    if (a == wtsv::A_REPLACE_MEMBRANE && sensor != 2.0) return "only the amperometric chlorine sensor (2) has a membrane to replace";
    if (a == wtsv::A_REPLACE_REAGENT && sensor != 3.0) return "only the DPD chlorine sensor (3) has a reagent to replace";
    if (a == wtsv::A_TWO_POINT && ref_mode != (double)wtsv::REF_CONSTANT)
        return "a two-point calibration takes its buffers as constants (ref_mode 0)";
    return nullptr;
}

const char *service_rule(int, const double *c)
{
    if (!whole_in(c[WT_SV_ENABLE], 0, 1)) return "enable must be 0 or 1";
    if (c[WT_SV_ENABLE] == 0.0) return nullptr;            // the other rows of a slot that is off are not read
    if (!whole_in(c[WT_SV_SENSOR], 0, WT_N_SENSORS - 1)) return "sensor must be an integer in 0..6";
    if (!whole_in(c[WT_SV_ACTION], 0, wtsv::N_ACTIONS - 1)) return "action must be an integer in 0..6";
    if (!whole_in(c[WT_SV_TRIGGER], 0, wtsv::N_TRIGGERS - 1)) return "trigger must be 0 (at_time) or 1 (on_status)";
    if (const char *msg = service_action_error(c[WT_SV_SENSOR], c[WT_SV_ACTION], c[WT_SV_REF_MODE])) return msg;
    for (const int f : {WT_SV_T_FIRST, WT_SV_PERIOD, WT_SV_DELAY})
        if (!(std::isfinite(c[f]) && c[f] >= 0.0)) return "t_first, period and delay must be finite and >= 0";
    if (c[WT_SV_PERIOD] != 0.0 && c[WT_SV_PERIOD] < wtsv::MIN_PERIOD) return "period must be 0 (once) or at least 0.001 s";
    if (!whole_in(c[WT_SV_COUNT], 0, 9007199254740991.0)) return "count must be a whole number >= 0 (0: no cap)";
    if (!whole_in(c[WT_SV_STATUS], 0, 11)) return "status must be an integer in 0..11 (a SensorStatus code)";
    if (!(std::isfinite(c[WT_SV_REF]) && std::isfinite(c[WT_SV_REF2]))) return "ref and ref2 must be finite";
    return nullptr;
}

// validate_flow_rate's maxima (__main__.py:57-63, :236-242) by loop: chlorine, acid
constexpr double k_command_limit[WT_TUN_LOOPS] = {1.0, 2.0};

const char *tune_rule(int loop, const double *c)
{
    if (!whole_in(c[WT_TUN_ENABLE], 0, 1)) return "enable must be 0 or 1";
    if (c[WT_TUN_ENABLE] == 0.0) return nullptr;           // the other rows of a loop that is off are not read
    if (!whole_in(c[WT_TUN_SENSOR], 0, WT_N_SENSORS - 1)) return "sensor must be an integer in 0..6";
    if (c[WT_TUN_DIRECTION] != 1.0 && c[WT_TUN_DIRECTION] != -1.0) return "direction must be +1 or -1";
    if (!(std::isfinite(c[WT_TUN_SETPOINT]) && std::isfinite(c[WT_TUN_BIAS]))) return "setpoint and bias must be finite";
    const double d = c[WT_TUN_AMPLITUDE], b = c[WT_TUN_BIAS];
    if (!(std::isfinite(d) && d > 0.0)) return "amplitude must be finite and > 0";
    if (!(b - d >= 0.0 && b + d <= k_command_limit[loop]))
        return "bias - amplitude must be >= 0 and bias + amplitude at most the loop's command limit (1.0 chlorine, 2.0 acid)";
    if (!(std::isfinite(c[WT_TUN_HYSTERESIS]) && c[WT_TUN_HYSTERESIS] >= 0.0)) return "hysteresis must be finite and >= 0";
    if (!std::isfinite(c[WT_TUN_T_START])) return "t_start must be finite";
    if (!(c[WT_TUN_T_MAX] > 0.0)) return "t_max must be > 0 (+inf: no time-out)";
    if (!whole_in(c[WT_TUN_SETTLE], 0, 9007199254740991.0)) return "settle must be a whole number >= 0";
    if (!whole_in(c[WT_TUN_CYCLES], 1, WT_TUN_MAX_CYCLES)) return "cycles must be an integer in 1..4096";
    for (const int f : {WT_TUN_KP_FACTOR, WT_TUN_TI_FACTOR})
        if (!(std::isfinite(c[f]) && c[f] >= 0.0)) return "kp_factor and ti_factor must be finite and >= 0";
    if (!whole_in(c[WT_TUN_COMMISSION], 0, 1)) return "commission must be 0 or 1";
    return nullptr;
}

// Walks a [slots][fields][N] block slot by slot, reactor by reactor, and hands each row vector to `rule`: the first
// message, so the first failing rule of the first bad reactor of the first bad slot is the one named.
const char *block_error(const double *p, int slots, int fields, int64_t N, Rule rule)
{
    std::vector<double> c((size_t)fields);
    for (int s = 0; s < slots; ++s)
        for (int64_t r = 0; r < N; ++r) {
            for (int k = 0; k < fields; ++k) c[(size_t)k] = p[((int64_t)s * fields + k) * N + r];
            if (const char *msg = rule(s, c.data())) return msg;
        }
    return nullptr;
}

// -- restart functions: the program's state at its set-time values (set, and reset where the program has one).  The
// arrays exist; the work is queued on the handle's stream, and a restart that uploads from host vectors synchronises
// before it returns them.

int upload(wt_ensemble *h, double *dst, const std::vector<double> &src)
{
    HIP_TRY(hipMemcpyAsync(dst, src.data(), sizeof(double) * src.size(), hipMemcpyHostToDevice, h->stream));
    return WT_OK;
}

// the reactors' loop time now (the download also waits for queued launches, which may still use the old records)
int loop_time(wt_ensemble *h, std::vector<double> &lt)
{
    lt.resize((size_t)h->N);
    return download(h, {{lt.data(), h->sens.pack.loop_time, sizeof(double) * lt.size()}});
}

int inject_restart(wt_ensemble *h)
{
    std::vector<double> st((size_t)h->N * wti::ST_DOUBLES);
    for (size_t i = 0; i < st.size(); i += wti::NIS) {
        double *q = st.data() + i;
        q[wti::IS_N_APPLIED] = 0.0; q[wti::IS_T_FIRST] = q[wti::IS_T_LAST] = q[wti::IS_HELD] = NAN;
    }
    if (int rc = upload(h, h->inj.st, st)) return rc;
    HIP_TRY(hipStreamSynchronize(h->stream));   // the host vector is freed on return
    return WT_OK;
}

int alarm_restart(wt_ensemble *h)
{
    const int64_t N = h->N;
    std::vector<double> st((size_t)N * wta::ST_DOUBLES, 0.0), rst((size_t)N * wta::RST_DOUBLES, 0.0), lt;
    for (size_t i = 0; i < st.size(); i += wta::NAS) {
        double *q = st.data() + i;
        q[wta::AS_PENDING] = q[wta::AS_T_FIRST] = q[wta::AS_T_LAST] = NAN;
    }
    if (int rc = loop_time(h, lt)) return rc;
    for (int64_t r = 0; r < N; ++r) {
        double *q = rst.data() + r * wta::RST_DOUBLES;
        q[wta::AR_T_PREV] = lt[(size_t)r]; q[wta::AR_FIRST_OUT] = -1.0; q[wta::AR_OVR_ACID] = q[wta::AR_OVR_CHLORINE] = NAN;
    }
    if (int rc = upload(h, h->alm.st, st)) return rc;
    if (int rc = upload(h, h->alm.rst, rst)) return rc;
    HIP_TRY(hipMemsetAsync(h->alm.word, 0, sizeof(uint16_t) * (size_t)N, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));   // the host vectors are freed on return
    return WT_OK;
}

// every element at its boundary row in force, the queue filled with it, t_prev the loop time
int actuator_restart(wt_ensemble *h)
{
    const int64_t N = h->N;
    std::vector<double> st((size_t)N * wtv::ST_DOUBLES, 0.0), q((size_t)N * wtv::Q_DOUBLES), lt((size_t)N), bc((size_t)N * wt::NB);
    // (the download also waits for queued launches, which may still read or write the old records)
    if (int rc = download(h, {{lt.data(), h->sens.pack.loop_time, sizeof(double) * lt.size()}, {bc.data(), h->bc, sizeof(double) * bc.size()}}))
        return rc;
    for (int64_t r = 0; r < N; ++r)
        for (int k = 0; k < wtv::CH; ++k) {
            const double row = bc[(size_t)(wtv::row_of(k) * N + r)];
            double *s = st.data() + r * wtv::ST_DOUBLES + k * wtv::NVS;
            s[wtv::VS_POSITION] = s[wtv::VS_APPLIED] = s[wtv::VS_PLAY] = s[wtv::VS_DEMAND] = row;
            for (int i = 0; i < wtv::MAX_DELAY; ++i) q[(size_t)(r * wtv::Q_DOUBLES + k * wtv::MAX_DELAY + i)] = row;
        }
    if (int rc = upload(h, h->act.st, st)) return rc;
    if (int rc = upload(h, h->act.q, q)) return rc;
    if (int rc = upload(h, h->act.tp, lt)) return rc;
    HIP_TRY(hipStreamSynchronize(h->stream));   // the host vectors are freed on return
    return WT_OK;
}

// x = 0, counts 0, an empty history, base = the boundary in force, t_prev = ReactorState.time, then one evaluation
int disturb_restart(wt_ensemble *h)
{
    const size_t N = (size_t)h->N;
    HIP_TRY(hipMemsetAsync(h->dst.st, 0, sizeof(double) * wtd::ST_DOUBLES * N, h->stream));
    if (h->dst.hist) HIP_TRY(hipMemsetAsync(h->dst.hist, 0, sizeof(double) * wtd::SLOTS * (size_t)h->dst.hist_cap * N, h->stream));   // entries not filled: 0
    HIP_TRY(hipMemcpyAsync(h->dst.base, h->bc, sizeof(double) * WT_NB * N, hipMemcpyDeviceToDevice, h->stream));
    HIP_TRY(hipMemcpyAsync(h->dst.tp, h->time, sizeof(double) * N, hipMemcpyDeviceToDevice, h->stream));
    return disturb_op(h, wtd::OP_SET);
}

// the accumulators and the curve at their set-time values, t_prev = ReactorState.time, j = 0
int score_restart(wt_ensemble *h)
{
    const size_t cells = (size_t)h->scr.curve_cap * wtsc::SLOTS;
    const wtsc::HostOpArgs a{h->scr.st, h->scr.tp, h->time, h->N};
    hipLaunchKernelGGL(wtsc::host_op_kernel, dim3((unsigned)((h->N + 255) / 256)), dim3(256), 0, h->stream, a);
    HIP_TRY(hipGetLastError());
    if (h->scr.counts) HIP_TRY(hipMemsetAsync(h->scr.counts, 0, sizeof(int32_t) * 3 * cells, h->stream));
    if (h->scr.fan) HIP_TRY(hipMemsetAsync(h->scr.fan, 0, sizeof(int32_t) * (size_t)(h->scr.bins + 2) * cells, h->stream));
    h->scr_steps = 0;
    return WT_OK;
}

// slot state and t_prev at their set-time values, t_prev = the reactors' loop time now
int detect_restart(wt_ensemble *h)
{
    std::vector<double> st((size_t)h->N * wtk::ST_DOUBLES, 0.0), lt;
    for (size_t i = 0; i < st.size(); i += wtk::NKS) {
        double *q = st.data() + i;
        q[wtk::KS_BASELINE] = q[wtk::KS_X_PREV] = q[wtk::KS_T_FIRST] = q[wtk::KS_T_DETECT] = NAN;
    }
    if (int rc = loop_time(h, lt)) return rc;
    if (int rc = upload(h, h->det.st, st)) return rc;
    if (int rc = upload(h, h->det.tp, lt)) return rc;
    HIP_TRY(hipStreamSynchronize(h->stream));   // the host vectors are freed on return
    return WT_OK;
}

// slot state at its set-time values (0, 0, 0, NaN) and an all-NaN store
int trend_restart(wt_ensemble *h)
{
    std::vector<double> st((size_t)h->N * wtt::ST_DOUBLES, 0.0);
    for (size_t i = 0; i < st.size(); i += wtt::NTS) st[i + wtt::TS_LAST] = NAN;
    HIP_TRY(hipStreamSynchronize(h->stream));   // queued launches may still write the old records
    if (int rc = upload(h, h->trd.st, st)) return rc;
    // every byte 0xff: a NaN in both halves of every sample
    HIP_TRY(hipMemsetAsync(h->trd.store, 0xff, sizeof(double2) * wtt::SLOTS * (size_t)h->trd.cap * (size_t)h->N, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));   // the host vector is freed on return
    return WT_OK;
}

// the slot state at its set-time values: 0, NaN, t_first from the parameter records in force, NaN
int service_restart(wt_ensemble *h)
{
    std::vector<double> par((size_t)h->N * wtsv::PAR_DOUBLES), st((size_t)h->N * wtsv::ST_DOUBLES);
    // (the download also waits for queued launches, which may still write the old state)
    if (int rc = download(h, {{par.data(), h->sens.svc_par, sizeof(double) * par.size()}})) return rc;
    for (size_t r = 0; r < (size_t)h->N; ++r)
        for (int k = 0; k < wtsv::SLOTS; ++k) {
            double *q = st.data() + r * wtsv::ST_DOUBLES + k * wtsv::NSVS;
            q[wtsv::VS_N_DONE] = 0.0; q[wtsv::VS_T_LAST] = NAN; q[wtsv::VS_T_SEEN] = NAN;
            q[wtsv::VS_T_DUE] = par[r * wtsv::PAR_DOUBLES + k * wtsv::NSV + wtsv::V_T_FIRST];
        }
    if (int rc = upload(h, h->sens.svc_st, st)) return rc;
    HIP_TRY(hipStreamSynchronize(h->stream));   // the host vector is freed on return
    return WT_OK;
}

// every loop waiting: the state all 0
int tune_restart(wt_ensemble *h)
{
    HIP_TRY(hipStreamSynchronize(h->stream));   // queued launches may still write the records
    HIP_TRY(hipMemsetAsync(h->tun.st, 0, sizeof(double) * wtu::ST_DOUBLES * (size_t)h->N, h->stream));
    return WT_OK;
}

// The service and the tune program own no arrays: their records are the sensor suite's and plant I/O's, which
// allocate, release and checkpoint them (sensor_arrays, plant_io_arrays).  For k_programs these two only name the
// switch and the records, parameters first; the descriptor says `borrowed`, and nothing allocates or releases them.
ArrayGroup service_records(wt_ensemble *h)
{
    return {"service", &h->sens.svc_on, {{(void **)&h->sens.svc_par, 0}, {(void **)&h->sens.svc_st, 0}}};
}

ArrayGroup tune_records(wt_ensemble *h)
{
    return {"tune", &h->tun.on, {{(void **)&h->tun.par, 0}, {(void **)&h->tun.st, 0}}};
}

// -- the descriptors, indexed by WT_PROG_*

enum Needs { NEEDS_PLANT_IO, NEEDS_SENSORS, NEEDS_STATE, NEEDS_STATE_AND_BOUNDARY };

struct Program {
    const char *not_set;                  // refusal of get, reset and the other read calls while no program is set
    Needs needs; const char *needs_text;  // what a set call needs first, and its refusal
    const char *zones;                    // refusal above 32 zones (nullptr: every kernel carries the program)
    int slots, fields;                    // the parameter block is [slots][fields][N], a record slots * fields doubles
    Rule first_pass, rule;                // first_pass (nullptr: none) runs over the whole block before rule does
    ArrayGroup (*arrays)(wt_ensemble *);  // switch and arrays; the parameter records are the group's first array
    int (*restart)(wt_ensemble *);        // nullptr: control_load builds the state, loop by loop
    bool borrowed;                        // the arrays are another part's: set does not allocate, stop only clears the switch
};

const Program k_programs[] = {
    {"control is off (wt_ensemble_control_enable)", NEEDS_PLANT_IO, "control writes the holding image: enable plant I/O first",
     nullptr, wtc::LOOPS, wtc::NC, nullptr, control_rule, control_arrays, nullptr},
    {"no injection program is set (wt_ensemble_inject_set)", NEEDS_PLANT_IO, "injection acts on the plant I/O images: enable plant I/O first",
     "injection programs run in the kernels for up to 32 zones", wti::SLOTS, wti::NI, nullptr, inject_rule, inject_arrays, inject_restart},
    {"no alarm program is set (wt_ensemble_alarm_set)", NEEDS_PLANT_IO, "alarms act on the plant I/O scan: enable plant I/O first",
     "alarm programs run in the kernels for up to 32 zones", wta::SLOTS, wta::NA, nullptr, alarm_rule, alarm_arrays, alarm_restart},
    {"no actuator program is set (wt_ensemble_actuator_set)", NEEDS_PLANT_IO, "actuators act on the plant I/O scan: enable plant I/O first",
     "actuator programs run in the kernels for up to 32 zones", wtv::CH, wtv::NV, actuator_finite, actuator_rule, actuator_arrays, actuator_restart},
    {"no disturbance program is set (wt_ensemble_disturb_set)", NEEDS_STATE_AND_BOUNDARY, "set_state and set_boundary must precede disturb_set",
     "disturbance programs run in the kernels for up to 32 zones", wtd::SLOTS, wtd::ND, disturb_finite, disturb_rule, disturb_arrays, disturb_restart},
    {"no score program is set (wt_ensemble_score_set)", NEEDS_STATE, "set_state must precede score_set",
     "score programs run in the kernels for up to 32 zones", wtsc::SLOTS, wtsc::NSP, nullptr, score_rule, score_arrays, score_restart},
    {"no detector program is set (wt_ensemble_detect_set)", NEEDS_PLANT_IO, "detectors read the plant I/O scan: enable plant I/O first",
     "detector programs run in the kernels for up to 32 zones", wtk::SLOTS, wtk::NK, nullptr, detect_rule, detect_arrays, detect_restart},
    {"no trend program is set (wt_ensemble_trend_set)", NEEDS_PLANT_IO, "trends read the plant I/O scan: enable plant I/O first",
     "trend programs run in the kernels for up to 32 zones", wtt::SLOTS, wtt::NT, nullptr, trend_rule, trend_arrays, trend_restart},
    {"no service program is set (wt_ensemble_service_set)", NEEDS_SENSORS, k_service_no_suite,
     "service programs run in the kernels for up to 32 zones", WT_SVC_SLOTS, WT_NSV, nullptr, service_rule, service_records, service_restart, true},
    {"no tune program is set (wt_ensemble_tune_set)", NEEDS_PLANT_IO, "tuners act on the plant I/O scan: enable plant I/O first",
     "tune programs run in the kernels for up to 32 zones", WT_TUN_LOOPS, WT_NU, nullptr, tune_rule, tune_records, tune_restart, true},
};
constexpr int N_PROGRAMS = (int)(sizeof k_programs / sizeof *k_programs);
static_assert(WT_PROG_CONTROL == 0 && WT_PROG_INJECT == 1 && WT_PROG_ALARM == 2 && WT_PROG_ACTUATOR == 3 && WT_PROG_DISTURB == 4 &&
              WT_PROG_SCORE == 5 && WT_PROG_DETECT == 6 && WT_PROG_TREND == 7 && WT_PROG_SERVICE == 8 && WT_PROG_TUNE == 9 &&
              N_PROGRAMS == 10, "k_programs is indexed by WT_PROG_*");
// wt_ensemble_info: one code per program up to the trend program, then the rest; service and tune have codes among the rest
static_assert(WT_INFO_PROGRAM + WT_PROG_SERVICE == WT_INFO_TRAIN && WT_INFO_SERVICE == 22 && WT_INFO_TUNE == 23, "wt_ensemble_info codes");

// -- the lifecycle

// The preconditions of a set call, in this order: the arguments, what the program needs first, the zone limit.  The
// parameter block itself goes through wt_program_check.
int check_program_set(const wt_ensemble *h, int program, const double *params)
{
    const Program &p = k_programs[program];
    if (!h || !params) return fail(WT_E_ARG, "NULL argument");
    const bool met = p.needs == NEEDS_PLANT_IO ? h->sens.plc_on != 0 : p.needs == NEEDS_SENSORS ? h->sens.on != 0
                   : h->have_state && (p.needs == NEEDS_STATE || h->have_bc);
    if (!met) return fail(WT_E_STATE, p.needs_text);
    if (p.zones && !wt::prog_in_item(levels_for(h->n))) return fail(WT_E_STATE, p.zones);
    return WT_OK;
}

// program off: its arrays released and its capacities 0, or, where the arrays are another part's, the switch alone
void switch_off(const Program &p, const ArrayGroup &g)
{
    if (p.borrowed) *g.on = 0; else release(g);
}

// The rest of a set call once the call is accepted and its sizes and settings are in the handle: the arrays (those of
// a running program are used again), the parameter records, the restart function, the switch.  A failure leaves the
// program off, with neither arrays nor capacities.
int load_program(wt_ensemble *h, int program, const double *params)
{
    const Program &p = k_programs[program];
    const ArrayGroup g = p.arrays(h);
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipStreamSynchronize(h->stream));   // queued launches may still read or write the old records
    if (int rc = p.borrowed ? WT_OK : allocate(g)) return rc;
    std::vector<double> par((size_t)h->N * p.slots * p.fields);
    blocks_to_records(params, p.slots, p.fields, h->N, par.data(), p.slots * p.fields);
    int rc = upload(h, (double *)*g.arrays[0].first, par);
    if (rc == WT_OK) rc = p.restart(h);
    if (rc == WT_OK) rc = sync_checked(h);      // the host vector is freed on return
    if (rc != WT_OK) { switch_off(p, g); return rc; }
    *g.on = 1;
    return WT_OK;
}

// The start of get, reset and every other call that needs a program set: the handle, the refusal, the device.
int program_ready(wt_ensemble *h, int program)
{
    if (!h) return fail(WT_E_ARG, "NULL handle");
    if (!*k_programs[program].arrays(h).on) return fail(WT_E_STATE, k_programs[program].not_set);
    HIP_TRY(hipSetDevice(h->device));
    return WT_OK;
}

int get_program(wt_ensemble *h, int program, const std::vector<Records> &records)
{
    if (int rc = program_ready(h, program)) return rc;
    return download_records(h, records);
}

int reset_program(wt_ensemble *h, int program)
{
    if (int rc = program_ready(h, program)) return rc;
    if (int rc = k_programs[program].restart(h)) return rc;
    return sync_checked(h);
}

// clear, and a set that replaces a program whose capacities may change
int stop_program(wt_ensemble *h, int program)
{
    if (!h) return fail(WT_E_ARG, "NULL handle");
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipStreamSynchronize(h->stream));   // queued launches may still use the records
    switch_off(k_programs[program], k_programs[program].arrays(h));
    return WT_OK;
}

// Enable (retune == false) or retune the PI programs.  A loop starts -- integral 0, output and holding words the
// float32 of the clamped bias, metrics 0 -- where enable switches it on; retune keeps the state of the other loops.
int control_load(wt_ensemble *h, const double *params, bool retune)
{
    if (!h) return fail(WT_E_ARG, "NULL handle");
    if (!params) return fail(WT_E_ARG, "params is NULL");
    if (int rc = check_program_set(h, WT_PROG_CONTROL, params)) return rc;
    if (retune && !h->ctl.on) return fail(WT_E_STATE, k_programs[WT_PROG_CONTROL].not_set);
    if (int rc = wt_program_check(WT_PROG_CONTROL, params, h->N)) return rc;
    HIP_TRY(hipSetDevice(h->device));
    const int64_t N = h->N;
    const size_t par_bytes = sizeof(double) * wtc::PAR_DOUBLES * (size_t)N, st_bytes = sizeof(double) * wtc::ST_DOUBLES * (size_t)N;
    std::vector<double> par((size_t)N * wtc::PAR_DOUBLES), old((size_t)N * wtc::PAR_DOUBLES, 0.0);
    std::vector<double> st((size_t)N * wtc::ST_DOUBLES, 0.0), lt((size_t)N);
    std::vector<uint16_t> hr((size_t)N * wtp::HR_WORDS);
    HIP_TRY(hipStreamSynchronize(h->stream));   // queued launches may still read or write the old records
    if (int rc = allocate(control_arrays(h))) return rc;
    if (int rc = download(h, {{hr.data(), h->ctl.hr, sizeof(uint16_t) * hr.size()},
                              {retune ? st.data() : nullptr, h->ctl.st, st_bytes}, {retune ? old.data() : nullptr, h->ctl.par, par_bytes},
                              {retune ? nullptr : lt.data(), h->sens.pack.loop_time, sizeof(double) * (size_t)N}}))
        return rc;
    blocks_to_records(params, wtc::LOOPS, wtc::NC, N, par.data(), wtc::PAR_DOUBLES);
    for (int64_t r = 0; r < N; ++r) {
        double *s = st.data() + r * wtc::ST_DOUBLES;
        if (!retune) s[wtc::T_PREV] = lt[(size_t)r];
        for (int l = 0; l < wtc::LOOPS; ++l) {
            const double *c = par.data() + r * wtc::PAR_DOUBLES + l * wtc::NC;
            const bool was_on = retune && old[(size_t)(r * wtc::PAR_DOUBLES + l * wtc::NC + wtc::C_ENABLE)] == 1.0;
            if (c[wtc::C_ENABLE] != 1.0 || was_on) continue;
            const double y = std::fmin(std::fmax(c[wtc::C_BIAS], c[wtc::C_OUT_MIN]), c[wtc::C_OUT_MAX]);
            double *q = s + l * wtc::NCS;
            for (int k = 0; k < wtc::NCS; ++k) q[k] = 0.0;
            q[wtc::CS_OUTPUT] = y;
            const float f = (float)y;   // round to nearest even, as the device's store
            uint32_t b; std::memcpy(&b, &f, sizeof b);
            uint16_t *w = hr.data() + r * wtp::HR_WORDS + wtc::loop_word(l);
            w[0] = (uint16_t)(b >> 16); w[1] = (uint16_t)(b & 0xffffu);
        }
    }
    HIP_TRY(hipMemcpyAsync((double *)h->ctl.par, par.data(), par_bytes, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipMemcpyAsync(h->ctl.st, st.data(), st_bytes, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipMemcpyAsync(h->ctl.hr, hr.data(), sizeof(uint16_t) * hr.size(), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));   // the host vectors are freed on return
    h->ctl.on = 1;
    return WT_OK;
}

// ovr_*, first_out and the word of reactor r from its slot records and state (after a reset)
uint16_t alarm_settle(const double *par, const double *st, double *rst)
{
    double ovr[2] = {NAN, NAN};
    unsigned word = 0;
    bool any = false;
    for (int s = 0; s < wta::SLOTS; ++s) {
        const double *p = par + s * wta::NA, *q = st + s * wta::NAS;
        if (q[wta::AS_ACTIVE] != 0.0) {
            any = true;
            word |= 1u << s;
            const double act = p[wta::A_ACTION];
            if (act == wta::ACT_TRIP_ACID && std::isnan(ovr[0])) ovr[0] = p[wta::A_TRIP_VALUE];
            if (act == wta::ACT_TRIP_CHLORINE && std::isnan(ovr[1])) ovr[1] = p[wta::A_TRIP_VALUE];
        }
        if (q[wta::AS_COND] != 0.0) word |= 1u << (4 + s);
    }
    if (!any) rst[wta::AR_FIRST_OUT] = -1.0;
    rst[wta::AR_OVR_ACID] = ovr[0]; rst[wta::AR_OVR_CHLORINE] = ovr[1];
    if (!std::isnan(ovr[0])) word |= wta::W_ACID;
    if (!std::isnan(ovr[1])) word |= wta::W_CHLORINE;
    word |= (unsigned)((int)rst[wta::AR_FIRST_OUT] + 1) << wta::W_FIRST_OUT_SHIFT;
    return (uint16_t)word;
}

// -- the train program (wt_trn.hpp): not one of k_programs, because setting it changes the handle's shape

const char *k_train_not_set = "no train program is set (wt_ensemble_train_set)";
const char *k_train_conflict = "a disturbance slot targets an inlet row (1, 2 or 3) that the train program feeds into that reactor";

// some non-OFF slot of a [WT_DST_SLOTS][WT_ND][N] disturbance block targets a row that lk (wtr::TrnArgs::lk) feeds
bool train_conflict(const int32_t *lk, const double *blk, int64_t N)
{
    for (int s = 0; s < wtd::SLOTS; ++s)
        for (int64_t r = 0; r < N; ++r) {
            const double row = blk[((int64_t)s * wtd::ND + wtd::D_ROW) * N + r];
            if (blk[((int64_t)s * wtd::ND + wtd::D_KIND) * N + r] != (double)wtd::K_OFF && row >= 1.0 && row <= 3.0 &&
                ((lk[r] >> ((int)row - 1)) & 1))
                return true;
        }
    return false;
}

// The handle's shape for R reactors per wavefront: the group count and what is sized by it -- the queue's arrays, the
// stream ranges of the default schedule, the workers.  The developer buffers of the old shape (wave diagnostics, item
// trace) are released; their next call allocates them again.  The stream is idle.  A failure leaves the old shape.
int reshape(wt_ensemble *h, int R)
{
    free_and_null(h->wave_diag); free_and_null(h->trace); h->trace_cap = 0;
    if (R == h->R) return WT_OK;
    const int64_t groups = (h->N + R - 1) / R;
    if (groups > 0x3fffffff) return fail(WT_E_ARG, "too many reactors for one ensemble");
    unsigned long long *slots = h->q_slots; int32_t *next = h->q_next;
    const int old_R = h->R, old_cap = h->q_cap; const int64_t old_groups = h->n_groups;
    h->q_slots = nullptr; h->q_next = nullptr;
    h->R = R; h->n_groups = groups; h->q_cap = (int)(2 * groups + 64);
    if (int rc = allocate(queue_arrays(h))) {
        h->q_slots = slots; h->q_next = next; h->R = old_R; h->n_groups = old_groups; h->q_cap = old_cap;
        return rc;
    }
    (void)hipFree(slots); (void)hipFree(next);
    if (h->sched_mode == WT_SCHED_QUEUE) h->n_sub = default_streams(h->N, h->R);
    h->q_workers = queue_workers(h);
    return WT_OK;
}

// n_fed = 0, t_last = NaN, base = rows 1..3 of the boundary in force, reactor r in slot r with an empty cost history
// (whole trains in consecutive slots), then every link fed from the current state
int train_restart(wt_ensemble *h)
{
    const size_t N = (size_t)h->N;
    std::vector<double> st(N * wtr::NTRS, 0.0);
    for (size_t r = 0; r < N; ++r) st[r * wtr::NTRS + wtr::S_T_LAST] = NAN;
    if (int rc = upload(h, h->trn.st, st)) return rc;
    HIP_TRY(hipMemcpyAsync((void *)h->trn.lk, h->trn_lk.data(), sizeof(int32_t) * N, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipMemcpyAsync(h->trn.base, h->bc + N, sizeof(double) * wtr::FED_ROWS * N, hipMemcpyDeviceToDevice, h->stream));
    hipLaunchKernelGGL(wtpl::iota_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, h->stream, h->perm, h->N);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemsetAsync(h->cost, 0, sizeof(int32_t) * N, h->stream));
    h->cost_steps = 0;
    // the junction program's arrays, off: no slot used, no state (a checkpoint holds them whether or not one is set)
    HIP_TRY(hipMemsetAsync((void *)h->trn.jct.src, 0, sizeof(uint32_t) * N, h->stream));
    HIP_TRY(hipMemsetAsync((void *)h->trn.jct.share, 0, sizeof(double) * wtr::JCT_SLOTS * N, h->stream));
    HIP_TRY(hipMemsetAsync(h->trn.jct.st, 0, sizeof(double) * wtr::NJS * N, h->stream));
    HIP_TRY(hipMemsetAsync(h->trn.jct.base0, 0, sizeof(double) * N, h->stream));
    if (int rc = train_op(h, wtr::OP_FEED)) return rc;
    return sync_checked(h);                     // the host vector is freed on return
}

// -- the pipe program (wt_trn.hpp) on top of a train program
const char *k_pipe_not_set = "no pipe program is set (wt_ensemble_pipe_set)";

// the first refusal of a delay array, reactor by reactor; linked(r): reactor r has an upstream that feeds it
template <class Linked> const char *pipe_error(int64_t N, const double *delay, Linked linked)
{
    for (int64_t r = 0; r < N; ++r) {
        if (!whole_in(delay[r], 0, WT_PIPE_MAX_DELAY)) return "delay must be a whole number in 0..4095 (outer steps)";
        if (delay[r] != 0.0 && !linked(r)) return "a stage that is not linked has no pipe: its delay must be 0";
    }
    return nullptr;
}

// the stream is idle: the lines go, the linked rows stay as they are
void pipe_release(wt_ensemble *h) { release(pipe_arrays(h)); }

// -- the junction program (wt_trn.hpp) on top of a train program
static_assert(WT_JCT_SLOTS == wtr::JCT_SLOTS && WT_NJ == wtr::NJ && WT_NJS == wtr::NJS && WT_J_STAGE == wtr::J_STAGE &&
              WT_J_SHARE == wtr::J_SHARE && WT_JS_N_BLEND == wtr::JS_N_BLEND && WT_JS_N_HELD == wtr::JS_N_HELD &&
              WT_JS_Q_LAST == wtr::JS_Q_LAST, "junction blocks of the C ABI");
const char *k_junction_not_set = "no junction program is set (wt_ensemble_junction_set)";
const char *k_junction_pipes = "junctions must be set before the pipes (a line holds what its junction delivered)";

// The first refusal of a [WT_JCT_SLOTS][WT_NJ][N] block and its carry[N] for trains of `length` stages: reactor by
// reactor, and at one reactor rule by rule in the header's order.  linked(r): the train program links reactor r.
template <class Linked> const char *junction_error(int length, int64_t N, const double *p, const double *carry, Linked linked)
{
    const auto at = [&](int k, int f, int64_t r) { return p[((int64_t)k * WT_NJ + f) * N + r]; };
    for (int64_t r = 0; r < N; ++r) {
        bool used = false;
        for (int k = 0; k < WT_JCT_SLOTS; ++k)
            if (!whole_in(at(k, WT_J_STAGE, r), -1, length - 1))
                return "a source's stage must be -1 (the slot is unused) or a whole number in 0..length - 1 (a stage of the same train)";
        for (int k = 0; k < WT_JCT_SLOTS; ++k) {
            used = used || at(k, WT_J_STAGE, r) >= 0.0;
            if (at(k, WT_J_STAGE, r) == (double)(r % length)) return "a junction cannot be its own source";
        }
        for (int k = 0; k < WT_JCT_SLOTS; ++k)
            for (int i = 0; i < k; ++i)
                if (at(k, WT_J_STAGE, r) >= 0.0 && at(k, WT_J_STAGE, r) == at(i, WT_J_STAGE, r))
                    return "a stage can be a source of a junction once only";
        for (int k = 0; k < WT_JCT_SLOTS; ++k)
            if (at(k, WT_J_STAGE, r) >= 0.0 && !(std::isfinite(at(k, WT_J_SHARE, r)) && at(k, WT_J_SHARE, r) > 0.0 && at(k, WT_J_SHARE, r) <= 1.0))
                return "a source's share must be finite and in (0, 1]";
        if (used && !linked(r)) return "a junction needs a linked reactor (the train program's link; a first stage has none)";
        if (!(carry[r] == 0.0 || carry[r] == 1.0)) return "carry must be 0 or 1";
        if (carry[r] == 1.0 && !used) return "carry needs a junction: a reactor without a used slot carries no flow";
    }
    return nullptr;
}

// -- the wire program (wt_wir.hpp) on top of a train program
static_assert(WT_NSENS == wts::NSENS && WT_NW == wtw::NW && WT_NWS == wtw::NWS && WT_W_STAGE == wtw::W_STAGE &&
              WT_W_SENSOR == wtw::W_SENSOR && WT_WS_N_ROUTED == wtw::WS_N_ROUTED && WT_WS_N_LOST == wtw::WS_N_LOST,
              "wire blocks of the C ABI");
const char *k_wire_not_set = "no wire program is set (wt_ensemble_wire_set)";

// The first refusal of a [WT_NSENS][WT_NW][N] block for trains of `length` stages: reactor by reactor, and at one
// reactor rule by rule over its seven slots -- finite, stage, sensor -- so that which slot holds which fault does not
// decide the message.
const char *wire_error(int length, int64_t N, const double *p)
{
    const auto at = [&](int i, int k, int64_t r) { return p[((int64_t)i * WT_NW + k) * N + r]; };
    for (int64_t r = 0; r < N; ++r) {
        for (int i = 0; i < WT_NSENS; ++i)
            if (!std::isfinite(at(i, WT_W_STAGE, r)) || !std::isfinite(at(i, WT_W_SENSOR, r))) return "wire parameters must be finite";
        for (int i = 0; i < WT_NSENS; ++i)
            if (!whole_in(at(i, WT_W_STAGE, r), -1, length - 1))
                return "stage must be -1 (the reactor's own instrument) or a whole number in 0..length - 1 (a stage of the same train)";
        for (int i = 0; i < WT_NSENS; ++i)
            if (!whole_in(at(i, WT_W_SENSOR, r), 0, WT_NSENS - 1)) return "a wire's sensor must be a whole number in 0..6";
    }
    return nullptr;
}

// the stream is idle: the cables go, every slot is the reactor's own instrument again
void wire_release(wt_ensemble *h) { release(wire_arrays(h)); }

// before a disturbance program's arrays go (clear, a set over a program): the targeted rows back to the base
int disturb_restore(wt_ensemble *h)
{
    HIP_TRY(hipSetDevice(h->device));
    if (!h->dst.on) return WT_OK;
    if (int rc = disturb_op(h, wtd::OP_RESTORE)) return rc;
    return sync_checked(h);
}

// ---- checkpoint, copy and rewind: one table of the handle's parts, which save, load, copy, mark,
// rewind and destroy all walk.  A part is its ArrayGroup function, how many of the group's trailing arrays are scratch,
// and its host scalars, field by field.  No pointer is a scalar: after a load the pointers are the destination's own
// allocations, and the aliases (sens.cmd.hr) are derived again by restore().

enum ScalarKind { S_I32, S_U32, S_I64, S_BOOL, S_F64 };

// a host field of a part; shape: a switch or a capacity that sizes arrays (two handles with equal shape scalars have
// arrays of equal sizes, which is what the rewind's fast path needs)
struct Scalar { ScalarKind kind; void *p; bool shape; };

int64_t scalar_get(const Scalar &s)
{
    switch (s.kind) {
    case S_I32: return *(const int32_t *)s.p;
    case S_U32: return *(const uint32_t *)s.p;
    case S_BOOL: return *(const bool *)s.p ? 1 : 0;
    default: { int64_t v; std::memcpy(&v, s.p, sizeof v); return v; }      // S_I64; S_F64: the double's bits
    }
}

void scalar_put(const Scalar &s, int64_t v)
{
    switch (s.kind) {
    case S_I32: *(int32_t *)s.p = (int32_t)v; break;
    case S_U32: *(uint32_t *)s.p = (uint32_t)v; break;
    case S_BOOL: *(bool *)s.p = v != 0; break;
    default: std::memcpy(s.p, &v, sizeof v); break;
    }
}

using Scalars = std::vector<Scalar>;

struct Part {
    const char *tag;                                    // four characters, the part's mark in a blob
    ArrayGroup (*arrays)(wt_ensemble *);
    int scratch;                                        // trailing arrays of the group that no checkpoint holds
    void (*scalars)(wt_ensemble *, Scalars &);          // nullptr: none
    bool (*present)(const wt_ensemble *);               // nullptr: the group's switch, or always without one
};

void switch_only(int *on, Scalars &s) { s.push_back({S_I32, on, true}); }

const Part k_parts[] = {
    // place_hist and q_ctrl are scratch; perm, cost and cost_steps travel, so a restored run re-deals when the original would
    {"CORE", core_arrays, 2, [](wt_ensemble *h, Scalars &s) {
         s.insert(s.end(), {{S_BOOL, &h->have_state, false}, {S_BOOL, &h->have_bc, false}, {S_I32, &h->placement, false},
                            {S_I64, &h->cost_steps, false}, {S_I32, &h->sched_mode, false}, {S_I32, &h->n_sub, false},
                            {S_I32, &h->chunk_steps, false}, {S_I32, &h->step_limit, false}}); }, nullptr},
    {"QUEU", queue_arrays, 2, nullptr, nullptr},
    {"SENS", sensor_arrays, 0, [](wt_ensemble *h, Scalars &s) {
         s.insert(s.end(), {{S_I32, &h->sens.on, true}, {S_I32, &h->sens.hist_cap, true}, {S_U32, &h->sens.seed_lo, false},
                            {S_U32, &h->sens.seed_hi, false}, {S_I64, &h->sens.reactor_base, false},
                            {S_I32, &h->sens.svc_on, false}, {S_I32, &h->ins.on, false}}); }, nullptr},   // (the service program's arrays and the installation records are the suite's)
    {"PLIO", plant_io_arrays, 0, [](wt_ensemble *h, Scalars &s) {
         s.insert(s.end(), {{S_I32, &h->sens.plc_on, true}, {S_I32, &h->tun.on, false}, {S_I32, &h->mpc.on, false}, {S_I32, &h->rsp.on, false},
                            {S_I32, &h->lnk.on, false}, {S_U32, &h->lnk.seed_lo, false}, {S_U32, &h->lnk.seed_hi, false}}); }, nullptr},   // (the tune program's, the model predictive controllers', the response programs' and the link programs' arrays are plant I/O's)
    {"RECD", record_arrays, 0, [](wt_ensemble *h, Scalars &s) {
         s.insert(s.end(), {{S_I32, &h->rec.every, false}, {S_I32, &h->rec.cap, true}, {S_I64, &h->rec.steps, false}}); },
     [](const wt_ensemble *h) { return h->rec.cap > 0; }},
    {"CTRL", control_arrays, 0, [](wt_ensemble *h, Scalars &s) { switch_only(&h->ctl.on, s); }, nullptr},
    {"INJC", inject_arrays, 0, [](wt_ensemble *h, Scalars &s) { switch_only(&h->inj.on, s); }, nullptr},
    {"ALRM", alarm_arrays, 0, [](wt_ensemble *h, Scalars &s) { switch_only(&h->alm.on, s); }, nullptr},
    {"ACTU", actuator_arrays, 0, [](wt_ensemble *h, Scalars &s) { switch_only(&h->act.on, s); }, nullptr},
    {"DSTB", disturb_arrays, 0, [](wt_ensemble *h, Scalars &s) {
         s.insert(s.end(), {{S_I32, &h->dst.on, true}, {S_I32, &h->dst.hist_cap, true}, {S_U32, &h->dst.seed_lo, false},
                            {S_U32, &h->dst.seed_hi, false}, {S_I64, &h->dst.reactor_base, false}}); }, nullptr},
    {"SCOR", score_arrays, 0, [](wt_ensemble *h, Scalars &s) {
         s.insert(s.end(), {{S_I32, &h->scr.on, true}, {S_I32, &h->scr.curve_cap, true}, {S_I32, &h->scr.bins, true},
                            {S_I64, &h->scr_steps, false}});
         for (int k = 0; k < wtsc::SLOTS; ++k)
             s.insert(s.end(), {{S_F64, &h->scr.fan_lo[k], false}, {S_F64, &h->scr.fan_hi[k], false}, {S_F64, &h->scr.fan_scale[k], false}}); },
     nullptr},
    {"DETC", detect_arrays, 0, [](wt_ensemble *h, Scalars &s) { switch_only(&h->det.on, s); }, nullptr},
    {"TRAN", train_arrays, 1, [](wt_ensemble *h, Scalars &s) {   // (the junction program's arrays are the train's)
         s.insert(s.end(), {{S_I32, &h->trn.on, true}, {S_I32, &h->trn.length, true}, {S_I32, &h->trn.jct.on, false}}); }, nullptr},
    {"PIPE", pipe_arrays, 0, [](wt_ensemble *h, Scalars &s) {
         s.insert(s.end(), {{S_I32, &h->trn.pipe.on, true}, {S_I32, &h->trn.pipe.slots, true}}); }, nullptr},
    {"WIRE", wire_arrays, 0, [](wt_ensemble *h, Scalars &s) { switch_only(&h->wir.on, s); }, nullptr},
    {"TRND", trend_arrays, 0, [](wt_ensemble *h, Scalars &s) {
         s.insert(s.end(), {{S_I32, &h->trd.on, true}, {S_I64, &h->trd.cap, true}, {S_I32, &h->trd.wrap, false}}); }, nullptr},
};
constexpr int N_PARTS = (int)(sizeof k_parts / sizeof *k_parts);
constexpr int PART_CORE = 0, PART_QUEUE = 1, PART_TRAIN = 12;   // core's first array is par, the train's first array lk
static_assert(N_PARTS == 16, "every *_arrays function of this file has one entry in k_parts (tests/test_checkpoint_cpu.py counts them)");

// a part of a handle as a checkpoint sees it: its scalars, whether it is on, and then its payload arrays
struct PartView { Scalars scalars; bool on; std::vector<std::pair<void **, size_t>> payload; };

PartView view(const Part &p, wt_ensemble *h)
{
    PartView v;
    if (p.scalars) p.scalars(h, v.scalars);
    const ArrayGroup g = p.arrays(h);
    v.on = p.present ? p.present(h) : (g.on ? *g.on != 0 : true);
    if (v.on) v.payload.assign(g.arrays.begin(), g.arrays.end() - p.scratch);
    return v;
}

uint32_t tag_word(const char *t) { uint32_t w; std::memcpy(&w, t, 4); return w; }
size_t pad8(size_t b) { return (b + 7) & ~(size_t)7; }

// The layout fingerprint: the table as a blob shows it -- tags, scalar kinds, array counts -- and the byte count of every
// payload array of a handle of one reactor with two zones and every capacity 1, which is the element size times the
// record constant (*_DOUBLES, SLOTS, NSENS, RING, ...) that sizes the array.
uint64_t layout_fingerprint()
{
    static const uint64_t value = [] {
        wt_ensemble u;
        u.N = 1; u.n = 2;
        uint64_t f = wtck::fnv1a_u64(WT_CKP_FORMAT, wtck::FNV_BASIS);
        for (const Part &p : k_parts) {
            Scalars sc;
            if (p.scalars) p.scalars(&u, sc);
            for (const Scalar &s : sc) if (s.shape) scalar_put(s, 1);
        }
        for (const Part &p : k_parts) {
            const PartView v = view(p, &u);
            f = wtck::fnv1a_u64(tag_word(p.tag), f);
            f = wtck::fnv1a_u64(v.scalars.size(), f);
            for (const Scalar &s : v.scalars) f = wtck::fnv1a_u64((uint64_t)s.kind * 2 + s.shape, f);
            f = wtck::fnv1a_u64(v.payload.size(), f);
            for (const auto &a : v.payload) f = wtck::fnv1a_u64(a.second, f);
        }
        return f;
    }();
    return value;
}

std::vector<int64_t> scalars_of(wt_ensemble *h)
{
    std::vector<int64_t> out;
    for (const Part &p : k_parts) {
        Scalars sc;
        if (p.scalars) p.scalars(h, sc);
        for (const Scalar &s : sc) out.push_back(scalar_get(s));
    }
    return out;
}

void apply_scalars(wt_ensemble *h, const std::vector<int64_t> &values)
{
    size_t i = 0;
    for (const Part &p : k_parts) {
        Scalars sc;
        if (p.scalars) p.scalars(h, sc);
        for (const Scalar &s : sc) scalar_put(s, values[i++]);
    }
}

// the switches and capacities of `values` are the handle's
bool same_shape(wt_ensemble *h, const std::vector<int64_t> &values)
{
    size_t i = 0;
    for (const Part &p : k_parts) {
        Scalars sc;
        if (p.scalars) p.scalars(h, sc);
        for (const Scalar &s : sc) { if (s.shape && scalar_get(s) != values[i]) return false; ++i; }
    }
    return true;
}

int64_t checkpoint_bytes(wt_ensemble *h)
{
    size_t total = WT_CKP_HEADER_BYTES;
    for (const Part &p : k_parts) {
        const PartView v = view(p, h);
        total += 16 + 8 * v.scalars.size();
        for (const auto &a : v.payload) total += 8 + pad8(a.second);
    }
    return (int64_t)total;
}

// Where a checkpoint's payload comes from: a blob on the host, another handle's arrays, or a mark's device memory.
struct Source {
    std::vector<int64_t> scalars;                                       // every part's, in table order
    std::vector<std::vector<std::pair<const void *, size_t>>> arrays;   // per part its payload arrays (none: the part is off)
    std::vector<int32_t> trn_lk;
    bool device = false;                                                // the arrays are device memory of the handle's device
};

Source source_of(wt_ensemble *h)
{
    Source s;
    s.scalars = scalars_of(h);
    for (const Part &p : k_parts) {
        const PartView v = view(p, h);
        s.arrays.emplace_back();
        for (const auto &a : v.payload) s.arrays.back().push_back({*a.first, a.second});
    }
    s.trn_lk = h->trn_lk;
    s.device = true;
    return s;
}

// A refusal of the configuration a blob declares: the rules the set calls enforce, on a host-only handle.
const char *config_error(wt_ensemble *u)
{
    for (const Part &p : k_parts) {
        Scalars sc;
        if (p.scalars) p.scalars(u, sc);
        for (const Scalar &s : sc) {
            const int64_t v = scalar_get(s);
            if (s.shape && (v < 0 || v > 0x7fffffff)) return "range";
            if (s.kind == S_BOOL && v != 0 && v != 1) return "range";
        }
    }
    const bool programs = u->ctl.on | u->inj.on | u->alm.on | u->act.on | u->det.on | u->trd.on;
    const bool zoned = u->inj.on | u->alm.on | u->act.on | u->dst.on | u->scr.on | u->det.on | u->trd.on;
    const auto flag = [](int v) { return v == 0 || v == 1; };
    if (!flag(u->sens.on) || !flag(u->sens.plc_on) || !flag(u->ctl.on) || !flag(u->inj.on) || !flag(u->alm.on) || !flag(u->act.on) ||
        !flag(u->dst.on) || !flag(u->scr.on) || !flag(u->det.on) || !flag(u->trn.on) || !flag(u->trn.pipe.on) || !flag(u->trn.jct.on) || !flag(u->wir.on) ||
        !flag(u->sens.svc_on) || !flag(u->ins.on) || !flag(u->tun.on) || !flag(u->mpc.on) || !flag(u->rsp.on) || !flag(u->lnk.on) || !flag(u->trd.on) || !flag(u->trd.wrap))
        return "range";
    if (u->placement != WT_PLACE_IDENTITY && u->placement != WT_PLACE_ADAPTIVE) return "range";
    if (u->sched_mode != WT_SCHED_STREAMS && u->sched_mode != WT_SCHED_QUEUE) return "range";
    if (u->n_sub < 1 || u->n_sub > WT_MAX_STREAMS || u->chunk_steps < 0 || u->step_limit < 0 || u->cost_steps < 0) return "range";
    if (u->rec.every < 1 || u->rec.steps < 0 || u->scr_steps < 0) return "range";
    if ((u->sens.plc_on && !u->sens.on) || (programs && !u->sens.plc_on) || (zoned && !wt::prog_in_item(levels_for(u->n)))) return "range";
    if (!u->sens.on && u->sens.hist_cap) return "range";
    if (!u->dst.on && u->dst.hist_cap) return "range";
    if ((!u->scr.on && (u->scr.curve_cap | u->scr.bins)) || u->scr.bins > wtsc::MAX_BINS || (!u->scr.curve_cap && u->scr.bins)) return "range";
    if (u->trd.on ? u->trd.cap < 1 : u->trd.cap != 0) return "range";
    if (u->trn.on ? (u->trn.length < 2 || u->trn.length > 64 / u->n || u->N % u->trn.length != 0) : u->trn.length != 0) return "range";
    if (u->trn.pipe.on ? (!u->trn.on || u->trn.pipe.slots < 1 || u->trn.pipe.slots > WT_PIPE_MAX_DELAY + 1) : u->trn.pipe.slots != 0) return "range";
    if (u->wir.on && (!u->trn.on || !u->sens.plc_on)) return "range";
    if (u->trn.jct.on && !u->trn.on) return "range";
    if (u->sens.svc_on && (!u->sens.on || !wt::prog_in_item(levels_for(u->n)))) return "range";
    if (u->ins.on && !u->sens.on) return "range";
    if (u->tun.on && (!u->sens.plc_on || !wt::prog_in_item(levels_for(u->n)))) return "range";
    if (u->mpc.on && (!u->sens.plc_on || !wt::prog_in_item(levels_for(u->n)))) return "range";
    if (u->rsp.on && (!u->sens.plc_on || !wt::prog_in_item(levels_for(u->n)))) return "range";
    if (u->lnk.on && (!u->sens.plc_on || !wt::prog_in_item(levels_for(u->n)))) return "range";
    return nullptr;
}

// Validates a blob on the host, every check of wt_checkpoint_check in its order, and describes it as a Source.  `into`:
// the handle a load is for, whose N and n the blob's must be (checked where N and n are, before the arrays).
int parse_blob(const void *blob, int64_t bytes, int64_t *N_out, int *n_out, Source *out, const wt_ensemble *into = nullptr)
{
    static_assert(sizeof(wt_checkpoint_header) == WT_CKP_HEADER_BYTES, "the header is 64 bytes without padding");
    if (!blob) return fail(WT_E_ARG, "checkpoint: NULL argument");
    if (bytes < WT_CKP_HEADER_BYTES) return fail(WT_E_ARG, "checkpoint: shorter than its header");
    wt_checkpoint_header hd;
    std::memcpy(&hd, blob, sizeof hd);
    if (std::memcmp(hd.magic, WT_CKP_MAGIC, 4) != 0) return fail(WT_E_ARG, "checkpoint: bad magic");
    if (hd.format != WT_CKP_FORMAT) return fail(WT_E_ARG, "checkpoint: unknown format version");
    if (hd.bytes != bytes) return fail(WT_E_ARG, "checkpoint: the header's byte count is not the blob's length");
    if (hd.layout != layout_fingerprint() || hd.abi != WT_ABI_VERSION || hd.n_parts != N_PARTS)
        return fail(WT_E_ARG, "checkpoint: the layout fingerprint is not this library's");
    const unsigned char *b = (const unsigned char *)blob;
    if (hd.checksum != wtck::fnv1a(b + WT_CKP_HEADER_BYTES, (size_t)bytes - WT_CKP_HEADER_BYTES))
        return fail(WT_E_ARG, "checkpoint: checksum mismatch");
    if (hd.n_reactors <= 0) return fail(WT_E_ARG, "checkpoint: n_reactors must be positive");
    if (hd.n_zones < 2 || hd.n_zones > WT_MAX_ZONES) return fail(WT_E_ARG, "checkpoint: n_zones must be in 2..64");
    if (into && (hd.n_reactors != into->N || (int)hd.n_zones != into->n))
        return fail(WT_E_ARG, "checkpoint_load: the checkpoint's n_reactors or n_zones differ from the handle's");
    const char *k_arrays = "checkpoint: a part's arrays do not match the capacities it declares";
    wt_ensemble u;                          // host only: holds the blob's scalars, sizes its arrays
    u.N = hd.n_reactors; u.n = (int)hd.n_zones;
    Source src;
    size_t at = WT_CKP_HEADER_BYTES;
    const size_t end = (size_t)bytes;
    const auto word = [&](size_t o) { uint32_t w; std::memcpy(&w, b + o, 4); return w; };
    for (const Part &p : k_parts) {         // the structure first: tags, counts, lengths that stay inside the blob
        Scalars sc;
        if (p.scalars) p.scalars(&u, sc);
        if (end - at < 8 || word(at) != tag_word(p.tag) || word(at + 4) != sc.size()) return fail(WT_E_ARG, k_arrays);
        at += 8;
        if (end - at < 8 * sc.size() + 8) return fail(WT_E_ARG, k_arrays);
        for (const Scalar &s : sc) {
            int64_t v; std::memcpy(&v, b + at, 8); at += 8;
            src.scalars.push_back(v);
            scalar_put(s, v);
        }
        const uint32_t count = word(at);
        if (word(at + 4) != 0) return fail(WT_E_ARG, k_arrays);
        at += 8;
        src.arrays.emplace_back();
        for (uint32_t i = 0; i < count; ++i) {
            int64_t len;
            if (end - at < 8) return fail(WT_E_ARG, k_arrays);
            std::memcpy(&len, b + at, 8); at += 8;
            if (len < 0 || (uint64_t)len > end - at || pad8((size_t)len) > end - at) return fail(WT_E_ARG, k_arrays);
            src.arrays.back().push_back({b + at, (size_t)len});
            at += pad8((size_t)len);
        }
    }
    if (at != end) return fail(WT_E_ARG, k_arrays);
    if (config_error(&u)) return fail(WT_E_ARG, "checkpoint: a part's switches or capacities are out of range");
    for (int i = 0; i < N_PARTS; ++i) {     // then every array's byte count against the capacities now in `u`
        const PartView v = view(k_parts[i], &u);
        if (v.payload.size() != src.arrays[(size_t)i].size()) return fail(WT_E_ARG, k_arrays);
        for (size_t k = 0; k < v.payload.size(); ++k)
            if (v.payload[k].second != src.arrays[(size_t)i][k].second) return fail(WT_E_ARG, k_arrays);
    }
    if (u.trn.on) {
        const int32_t *lk = (const int32_t *)src.arrays[PART_TRAIN][0].first;
        src.trn_lk.assign(lk, lk + u.N);
    }
    if (N_out) *N_out = hd.n_reactors;
    if (n_out) *n_out = (int)hd.n_zones;
    if (out) *out = std::move(src);
    return WT_OK;
}

// Device-to-device copies on `stream`: the table kernel, as many launches as 128-entry tables are needed, or (memcpy)
// one hipMemcpyAsync per array.  Zero-byte copies are skipped here.
int device_copies(const std::vector<Copy> &copies, hipStream_t stream, bool memcpy_each)
{
    if (memcpy_each) {
        for (const Copy &c : copies)
            if (c.bytes) HIP_TRY(hipMemcpyAsync(c.dst, c.src, c.bytes, hipMemcpyDeviceToDevice, stream));
        return WT_OK;
    }
    wtck::CopyTable t;
    t.count = 0; t.chunks = 0;
    const auto flush = [&]() {
        if (t.count == 0) return;
        t.first[t.count] = t.chunks;
        const int grid = t.chunks < 4096 ? t.chunks : 4096;
        hipLaunchKernelGGL(wtck::copy_table_kernel, dim3((unsigned)grid), dim3(wtck::THREADS), 0, stream, t);
        t.count = 0; t.chunks = 0;
    };
    for (const Copy &c : copies) {
        if (!c.bytes) continue;
        const size_t chunks = (c.bytes + wtck::CHUNK - 1) / wtck::CHUNK;
        if (chunks > 0x3fffffffu) return fail(WT_E_ARG, "checkpoint: an array is too large for one copy");
        if (t.count == wtck::MAX_ENTRIES || (size_t)t.chunks + chunks > 0x3fffffffu) flush();
        t.src[t.count] = c.src; t.dst[t.count] = c.dst; t.bytes[t.count] = (int64_t)c.bytes; t.first[t.count] = t.chunks;
        t.chunks += (int)chunks; ++t.count;
    }
    flush();
    HIP_TRY(hipGetLastError());
    return WT_OK;
}

// wave diagnostics, item trace and launch timing off: what a checkpoint does not hold
void instrumentation_off(wt_ensemble *h)
{
    free_and_null(h->wave_diag); free_and_null(h->trace); h->trace_cap = 0;
    h->time_launches = false; h->lt_used = 0;
}

// every optional part off, as a fresh handle has them (the stream is idle)
void release_optional(wt_ensemble *h)
{
    for (int i = 0; i < N_PARTS; ++i)
        if (i != PART_CORE && i != PART_QUEUE) release(k_parts[i].arrays(h));
}

// The handle takes the source's configuration and payload.  Where its switches and capacities already are the
// source's, nothing is released or allocated and the copies are queued on its stream with no synchronisation (the
// rewind's fast path).  Otherwise the stream is synchronised, every optional part is released, the source's scalars are
// stored, the shape is rebuilt by reshape() under the handle's own packing rule, and the groups are allocated anew.  A
// HIP failure on that path leaves a handle without programs that needs set_state and set_boundary again.
int restore(wt_ensemble *h, const Source &src)
{
    HIP_TRY(hipSetDevice(h->device));
    if (!same_shape(h, src.scalars)) {
        HIP_TRY(hipStreamSynchronize(h->stream));
        release_optional(h);
        apply_scalars(h, src.scalars);
        const int length = h->trn.on ? h->trn.length : 0;
        int rc = reshape(h, length ? length * units_per_wavefront(h->device, h->N / length, 64 / h->n / length) : h->R0);
        for (int i = 0; i < N_PARTS && rc == WT_OK; ++i)
            if (view(k_parts[i], h).on) rc = allocate(k_parts[i].arrays(h));
        if (rc != WT_OK) {
            const std::string msg = g_err;
            release_optional(h);
            (void)reshape(h, h->R0);
            h->have_state = h->have_bc = false;
            return fail(rc, msg);
        }
    } else {
        apply_scalars(h, src.scalars);
    }
    std::vector<Copy> copies;
    for (int i = 0; i < N_PARTS; ++i) {
        const PartView v = view(k_parts[i], h);
        if (v.payload.size() != src.arrays[(size_t)i].size()) return fail(WT_E_ARG, "checkpoint: internal error: part count");
        for (size_t k = 0; k < v.payload.size(); ++k) {
            if (v.payload[k].second != src.arrays[(size_t)i][k].second) return fail(WT_E_ARG, "checkpoint: internal error: array size");
            copies.push_back({*v.payload[k].first, src.arrays[(size_t)i][k].first, v.payload[k].second});
        }
    }
    if (src.device) {
        if (int rc = device_copies(copies, h->stream, h->knob_memcpy != 0)) return rc;
    } else {
        for (const Copy &c : copies)
            if (c.bytes) HIP_TRY(hipMemcpyAsync(c.dst, c.src, c.bytes, hipMemcpyHostToDevice, h->stream));
    }
    // what is derived from the arrays and the shape, by the rules of the calls that set them
    h->sens.cmd.hr = h->ctl.hr;
    h->trn_lk = src.trn_lk;
    if (h->sched_mode == WT_SCHED_QUEUE) h->n_sub = default_streams(h->N, h->R);
    h->bc_known = false;                    // one extra upload, never a wrong skip
    return WT_OK;
}

} // namespace

// the device-resident checkpoint of wt_ensemble_mark: one allocation, the payload arrays at 256-byte offsets
struct wt_mark {
    void *buf = nullptr;
    Source src;
};

namespace {

void drop_mark(wt_ensemble *h)
{
    if (!h->mark) return;
    if (h->mark->buf) (void)hipFree(h->mark->buf);
    delete h->mark;
    h->mark = nullptr;
}

// the two handles hold the same reactor constants
bool same_constants(const wt_ensemble *a, const void *par, size_t bytes)
{
    return bytes == sizeof(double) * a->par_sent.size() && std::memcmp(a->par_sent.data(), par, bytes) == 0;
}

} // namespace

extern "C" {

int wt_ensemble_destroy(wt_ensemble *h)
{
    if (!h) return WT_OK;
    (void)hipSetDevice(h->device);
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    drop_mark(h);
    for (const Part &p : k_parts) release(p.arrays(h));
    free_and_null(h->trace); free_and_null(h->wave_diag); free_and_null(h->snap_dev); free_and_null(h->sched);
    free_and_null(h->diag_out);
    for (int s = 0; s < WT_MAX_STREAMS; ++s) {
        if (h->sub_stream[s]) { (void)hipStreamSynchronize(h->sub_stream[s]); (void)hipStreamDestroy(h->sub_stream[s]); }
        if (h->sub_done[s]) (void)hipEventDestroy(h->sub_done[s]);
    }
    if (h->snap_host) (void)hipHostFree(h->snap_host);
    if (h->err_host) (void)hipHostFree(h->err_host);
    for (hipEvent_t e : h->lt_pool) (void)hipEventDestroy(e);
    if (h->ev_fork) (void)hipEventDestroy(h->ev_fork);
    if (h->ev0) (void)hipEventDestroy(h->ev0);
    if (h->ev1) (void)hipEventDestroy(h->ev1);
    if (h->own_stream && h->stream) (void)hipStreamDestroy(h->stream);
    delete h;
    return WT_OK;
}

int wt_program_check(int program, const double *params, int64_t n_reactors)
{
    if (!params) return fail(WT_E_ARG, "params is NULL");
    if (n_reactors < 1) return fail(WT_E_ARG, "n_reactors must be >= 1");
    if (program < 0 || program >= N_PROGRAMS) return fail(WT_E_ARG, "unknown program");
    const Program &p = k_programs[program];
    const char *msg = p.first_pass ? block_error(params, p.slots, p.fields, n_reactors, p.first_pass) : nullptr;
    if (!msg) msg = block_error(params, p.slots, p.fields, n_reactors, p.rule);
    return msg ? fail(WT_E_ARG, msg) : WT_OK;
}

int wt_ensemble_control_enable(wt_ensemble *h, const double *params) { return control_load(h, params, false); }
int wt_ensemble_control_retune(wt_ensemble *h, const double *params) { return control_load(h, params, true); }

int wt_ensemble_control_get(wt_ensemble *h, double *state)
{
    if (!h || !state) return fail(WT_E_ARG, "NULL argument");
    return get_program(h, WT_PROG_CONTROL, {{state, h->ctl.st, wtc::ST_DOUBLES, wtc::LOOPS, wtc::NCS}});
}

int wt_ensemble_control_disable(wt_ensemble *h) { return stop_program(h, WT_PROG_CONTROL); }

int wt_ensemble_inject_set(wt_ensemble *h, const double *params)
{
    if (int rc = check_program_set(h, WT_PROG_INJECT, params)) return rc;
    if (int rc = wt_program_check(WT_PROG_INJECT, params, h->N)) return rc;
    return load_program(h, WT_PROG_INJECT, params);
}

int wt_ensemble_inject_get(wt_ensemble *h, double *state)
{
    if (!h || !state) return fail(WT_E_ARG, "NULL argument");
    return get_program(h, WT_PROG_INJECT, {{state, h->inj.st, wti::ST_DOUBLES, wti::SLOTS, wti::NIS}});
}

int wt_ensemble_inject_clear(wt_ensemble *h) { return stop_program(h, WT_PROG_INJECT); }

int wt_ensemble_alarm_set(wt_ensemble *h, const double *params)
{
    if (int rc = check_program_set(h, WT_PROG_ALARM, params)) return rc;
    if (int rc = wt_program_check(WT_PROG_ALARM, params, h->N)) return rc;
    return load_program(h, WT_PROG_ALARM, params);
}

int wt_ensemble_alarm_get(wt_ensemble *h, double *slot_state, double *reactor_state)
{
    if (!h) return fail(WT_E_ARG, "NULL handle");
    return get_program(h, WT_PROG_ALARM, {{slot_state, h->alm.st, wta::ST_DOUBLES, wta::SLOTS, wta::NAS},
                                          {reactor_state, h->alm.rst, wta::RST_DOUBLES, 1, wta::NAR}});
}

int wt_ensemble_alarm_reset(wt_ensemble *h, const uint8_t *mask)
{
    if (int rc = program_ready(h, WT_PROG_ALARM)) return rc;
    const int64_t N = h->N;
    std::vector<double> par((size_t)N * wta::PAR_DOUBLES), st((size_t)N * wta::ST_DOUBLES), rst((size_t)N * wta::RST_DOUBLES);
    std::vector<uint16_t> word((size_t)N);
    if (int rc = download(h, {{par.data(), h->alm.par, sizeof(double) * par.size()}, {st.data(), h->alm.st, sizeof(double) * st.size()},
                              {rst.data(), h->alm.rst, sizeof(double) * rst.size()}, {word.data(), h->alm.word, sizeof(uint16_t) * word.size()}}))
        return rc;
    for (int64_t r = 0; r < N; ++r) {
        if (mask && !mask[r]) continue;
        const double *p = par.data() + r * wta::PAR_DOUBLES;
        double *q = st.data() + r * wta::ST_DOUBLES;
        for (int s = 0; s < wta::SLOTS; ++s) {
            double *qs = q + s * wta::NAS;
            if (p[s * wta::NA + wta::A_LATCH] == 1.0 && qs[wta::AS_ACTIVE] == 1.0 && qs[wta::AS_COND] == 0.0) {
                qs[wta::AS_ACTIVE] = 0.0; qs[wta::AS_PENDING] = NAN;
            }
        }
        word[(size_t)r] = alarm_settle(p, q, rst.data() + r * wta::RST_DOUBLES);
    }
    if (int rc = upload(h, h->alm.st, st)) return rc;
    if (int rc = upload(h, h->alm.rst, rst)) return rc;
    HIP_TRY(hipMemcpyAsync(h->alm.word, word.data(), sizeof(uint16_t) * word.size(), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    return WT_OK;
}

int wt_ensemble_alarm_words(wt_ensemble *h, uint16_t *words)
{
    if (!h || !words) return fail(WT_E_ARG, "NULL argument");
    if (int rc = program_ready(h, WT_PROG_ALARM)) return rc;
    return download(h, {{words, h->alm.word, sizeof(uint16_t) * (size_t)h->N}});
}

int wt_ensemble_alarm_device(wt_ensemble *h, void **word)
{
    if (!h || !word) return fail(WT_E_ARG, "NULL argument");
    if (int rc = program_ready(h, WT_PROG_ALARM)) return rc;
    *word = h->alm.word;
    return WT_OK;
}

int wt_ensemble_alarm_clear(wt_ensemble *h) { return stop_program(h, WT_PROG_ALARM); }

int wt_ensemble_actuator_set(wt_ensemble *h, const double *params)
{
    if (int rc = check_program_set(h, WT_PROG_ACTUATOR, params)) return rc;
    if (int rc = wt_program_check(WT_PROG_ACTUATOR, params, h->N)) return rc;
    return load_program(h, WT_PROG_ACTUATOR, params);
}

int wt_ensemble_actuator_get(wt_ensemble *h, double *state, double *queue, double *t_prev)
{
    if (!h) return fail(WT_E_ARG, "NULL handle");
    return get_program(h, WT_PROG_ACTUATOR, {{state, h->act.st, wtv::ST_DOUBLES, wtv::CH, wtv::NVS},
                                             {queue, h->act.q, wtv::Q_DOUBLES, wtv::CH, wtv::MAX_DELAY}, {t_prev, h->act.tp, 1, 1, 1}});
}

int wt_ensemble_actuator_clear(wt_ensemble *h) { return stop_program(h, WT_PROG_ACTUATOR); }

int wt_ensemble_disturb_set(wt_ensemble *h, const double *params, uint64_t seed, int64_t reactor_base, int history_capacity)
{
    if (int rc = check_program_set(h, WT_PROG_DISTURB, params)) return rc;
    if (history_capacity < 0) return fail(WT_E_ARG, "history_capacity must be >= 0 (0 = no history)");
    int64_t hist = 0;
    if (__builtin_mul_overflow((int64_t)history_capacity * wtd::SLOTS, h->N, &hist) ||
        __builtin_mul_overflow(hist, (int64_t)sizeof(double), &hist))
        return fail(WT_E_ARG, "history size overflows int64");
    if (int rc = wt_program_check(WT_PROG_DISTURB, params, h->N)) return rc;
    if (h->trn.on && train_conflict(h->trn_lk.data(), params, h->N)) return fail(WT_E_STATE, k_train_conflict);
    if (int rc = disturb_restore(h)) return rc;
    if (int rc = stop_program(h, WT_PROG_DISTURB)) return rc;   // set replaces any program (and its capacity)
    h->dst.hist_cap = history_capacity;
    h->dst.seed_lo = (uint32_t)(seed & 0xffffffffu); h->dst.seed_hi = (uint32_t)(seed >> 32); h->dst.reactor_base = reactor_base;
    return load_program(h, WT_PROG_DISTURB, params);
}

int wt_ensemble_disturb_get(wt_ensemble *h, double *slot_state, double *base, double *t_prev)
{
    if (!h) return fail(WT_E_ARG, "NULL handle");
    if (int rc = get_program(h, WT_PROG_DISTURB, {{slot_state, h->dst.st, wtd::ST_DOUBLES, wtd::SLOTS, wtd::NDS}, {t_prev, h->dst.tp, 1, 1, 1}}))
        return rc;
    return download(h, {{base, h->dst.base, sizeof(double) * WT_NB * (size_t)h->N}});
}

int wt_ensemble_disturb_history(wt_ensemble *h, double *offsets, int32_t *n_filled)
{
    if (int rc = program_ready(h, WT_PROG_DISTURB)) return rc;
    const int64_t N = h->N;
    const int cap = h->dst.hist_cap;
    std::vector<double> st((size_t)N * wtd::NDS);   // slot 0's state: n_eval
    if (int rc = download_records(h, {{st.data(), h->dst.st, wtd::ST_DOUBLES, 1, wtd::NDS},
                                      {cap > 0 ? offsets : nullptr, h->dst.hist, wtd::SLOTS * cap, cap, wtd::SLOTS}}))
        return rc;
    if (n_filled)
        for (int64_t r = 0; r < N; ++r) {
            const double e = st[(size_t)(wtd::DS_N_EVAL * N + r)];
            n_filled[r] = (int32_t)(e < cap ? e : cap);
        }
    return WT_OK;
}

int wt_ensemble_disturb_clear(wt_ensemble *h)
{
    if (!h) return fail(WT_E_ARG, "NULL handle");
    if (int rc = disturb_restore(h)) return rc;
    return stop_program(h, WT_PROG_DISTURB);
}

int wt_train_check(int length, int n_zones, int64_t n_reactors, const double *params)
{
    if (n_reactors < 1) return fail(WT_E_ARG, "n_reactors must be >= 1");
    if (n_zones < 2 || n_zones > WT_MAX_ZONES) return fail(WT_E_ARG, "n_zones must be in 2..64");
    if (length < 2 || length > 64 / n_zones)
        return fail(WT_E_ARG, "length must be at least 2 and at most 64 / n_zones (the stages of a train share a wavefront)");
    if (n_reactors % length != 0) return fail(WT_E_ARG, "n_reactors must be a multiple of length (an ensemble holds whole trains)");
    if (!params) return WT_OK;                  // every stage after the first linked, rows 7
    for (int64_t r = 0; r < n_reactors; ++r) {
        const double link = params[WT_TR_LINK * n_reactors + r], rows = params[WT_TR_ROWS * n_reactors + r];
        if (!(link == 0.0 || link == 1.0)) return fail(WT_E_ARG, "link must be 0 or 1");
        if (link != 0.0 && r % length == 0) return fail(WT_E_ARG, "the first stage of a train has no upstream: its link must be 0");
        if (!whole_in(rows, 0, 7)) return fail(WT_E_ARG, "rows must be an integer in 0..7 (1 pH, 2 chlorine, 4 temperature)");
    }
    return WT_OK;
}

int wt_ensemble_train_set(wt_ensemble *h, int length, const double *params)
{
    if (!h) return fail(WT_E_ARG, "NULL handle");
    if (!h->have_state || !h->have_bc) return fail(WT_E_STATE, "set_state and set_boundary must precede train_set");
    if (int rc = wt_train_check(length, h->n, h->N, params)) return rc;
    const int64_t N = h->N;
    std::vector<int32_t> lk((size_t)N);
    for (int64_t r = 0; r < N; ++r) {
        const bool linked = params ? params[WT_TR_LINK * N + r] == 1.0 : r % length != 0;
        lk[(size_t)r] = linked ? (wtr::LINKED | (params ? (int)params[WT_TR_ROWS * N + r] : 7)) : 0;
    }
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipStreamSynchronize(h->stream));   // queued launches may still use the records and the old shape
    if (h->dst.on) {                            // the other direction: wt_ensemble_disturb_set with a train program set
        std::vector<double> rec((size_t)N * wtd::PAR_DOUBLES), blk(rec.size());
        if (int rc = download(h, {{rec.data(), h->dst.par, sizeof(double) * rec.size()}})) return rc;
        records_to_blocks(rec.data(), wtd::PAR_DOUBLES, wtd::SLOTS, wtd::ND, N, blk.data());
        if (train_conflict(lk.data(), blk.data(), N)) return fail(WT_E_STATE, k_train_conflict);
    }
    if (h->trn.on) {                            // set replaces a program: its rows go back to its base first
        if (int rc = train_op(h, wtr::OP_RESTORE)) return rc;
        if (int rc = sync_checked(h)) return rc;
        pipe_release(h);                        // and its pipes, wires and junctions go with it
        wire_release(h);
        h->trn.jct.on = 0;
    }
    // whole trains per wavefront: the small-ensemble rule of wt_ensemble_create, counted in trains
    const int k = units_per_wavefront(h->device, N / length, 64 / h->n / length);
    if (int rc = reshape(h, length * k)) return rc;
    const ArrayGroup g = train_arrays(h);
    int rc = allocate(g);
    if (rc == WT_OK) {
        h->trn.length = length; h->trn_lk = lk;
        rc = train_restart(h);
    }
    if (rc != WT_OK) { release(g); (void)reshape(h, h->R0); return rc; }
    h->trn.on = 1;
    return WT_OK;
}

int wt_ensemble_train_get(wt_ensemble *h, int *length, int *per_wavefront, double *state)
{
    if (!h) return fail(WT_E_ARG, "NULL handle");
    if (!h->trn.on) return fail(WT_E_STATE, k_train_not_set);
    HIP_TRY(hipSetDevice(h->device));
    if (length) *length = h->trn.length;
    if (per_wavefront) *per_wavefront = h->R;
    return download_records(h, {{state, h->trn.st, wtr::NTRS, 1, wtr::NTRS}});
}

int wt_ensemble_train_params(wt_ensemble *h, double *params)
{
    if (!h || !params) return fail(WT_E_ARG, "NULL argument");
    if (!h->trn.on) return fail(WT_E_STATE, k_train_not_set);
    const int64_t N = h->N;
    for (int64_t r = 0; r < N; ++r) {
        const int32_t lk = h->trn_lk[(size_t)r];
        params[WT_TR_LINK * N + r] = (lk & wtr::LINKED) ? 1.0 : 0.0;
        params[WT_TR_ROWS * N + r] = (double)(lk & 7);
    }
    return WT_OK;
}

int wt_ensemble_train_clear(wt_ensemble *h)
{
    if (!h) return fail(WT_E_ARG, "NULL handle");
    if (!h->trn.on) return WT_OK;
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipStreamSynchronize(h->stream));   // queued launches may still use the records and the shape
    if (int rc = train_op(h, wtr::OP_RESTORE)) return rc;
    if (int rc = sync_checked(h)) return rc;
    pipe_release(h);
    wire_release(h);
    release(train_arrays(h));
    return reshape(h, h->R0);
}

int wt_pipe_check(int64_t n_reactors, const double *train_params, const double *delay)
{
    if (n_reactors < 1) return fail(WT_E_ARG, "n_reactors must be >= 1");
    if (!train_params || !delay) return fail(WT_E_ARG, "NULL argument");
    const char *msg = pipe_error(n_reactors, delay, [&](int64_t r) { return train_params[WT_TR_LINK * n_reactors + r] == 1.0; });
    return msg ? fail(WT_E_ARG, msg) : WT_OK;
}

int wt_ensemble_pipe_set(wt_ensemble *h, const double *delay)
{
    if (!h) return fail(WT_E_ARG, "NULL handle");
    if (!h->trn.on) return fail(WT_E_STATE, k_train_not_set);
    if (!delay) return fail(WT_E_ARG, "delay is NULL");
    const int64_t N = h->N;
    if (const char *msg = pipe_error(N, delay, [&](int64_t r) { return h->trn_lk[(size_t)r] != 0; })) return fail(WT_E_ARG, msg);
    std::vector<int32_t> d((size_t)N);
    int most = 0;
    for (int64_t r = 0; r < N; ++r) { d[(size_t)r] = (int32_t)delay[r]; most = std::max(most, (int)d[(size_t)r]); }
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipStreamSynchronize(h->stream));   // queued launches may still use the old lines
    pipe_release(h);                            // set replaces any program
    h->trn.pipe.slots = most + 1;
    int rc = allocate(pipe_arrays(h));
    if (rc == WT_OK) {
        h->trn.pipe.on = 1;                     // (the re-delivery below reads the lines)
        hipError_t e = hipMemcpyAsync((void *)h->trn.pipe.delay, d.data(), sizeof(int32_t) * (size_t)N, hipMemcpyHostToDevice, h->stream);
        if (e != hipSuccess) rc = fail(WT_E_HIP, hipGetErrorString(e));
        if (rc == WT_OK) rc = train_op(h, wtr::OP_PIPE_FILL);   // every line full of the upstream's outlet as it is now
        if (rc == WT_OK) rc = train_op(h, wtr::OP_FEED);        // and every link delivered from it
        if (rc == WT_OK) rc = sync_checked(h);  // the host vector is freed on return
    }
    if (rc != WT_OK) { (void)hipStreamSynchronize(h->stream); pipe_release(h); return rc; }
    return WT_OK;
}

int wt_ensemble_pipe_get(wt_ensemble *h, int *slots, double *delay, double *state, double *lines)
{
    if (!h) return fail(WT_E_ARG, "NULL handle");
    if (!h->trn.pipe.on) return fail(WT_E_STATE, k_pipe_not_set);
    HIP_TRY(hipSetDevice(h->device));
    const wtr::PipeArgs &p = h->trn.pipe;
    const size_t N = (size_t)h->N;
    if (slots) *slots = p.slots;
    if (int rc = download_records(h, {{state, p.st, wtr::NPS, 1, wtr::NPS}})) return rc;
    if (!delay && !lines) return WT_OK;
    std::vector<int32_t> d(N), head(N);
    std::vector<double> ring(lines ? (size_t)wtr::PIPE_Q * (size_t)p.slots * N : 0);
    if (int rc = download(h, {{d.data(), p.delay, sizeof(int32_t) * N}, {head.data(), p.head, sizeof(int32_t) * N},
                              {lines ? ring.data() : nullptr, p.ring, sizeof(double) * ring.size()}}))
        return rc;
    if (delay) for (size_t r = 0; r < N; ++r) delay[r] = (double)d[r];
    if (lines)   // [slots - 1][4][N]: the samples in flight, oldest first -- the D slots after head, in ring order
        for (int i = 0; i + 1 < p.slots; ++i)
            for (int q = 0; q < wtr::PIPE_Q; ++q)
                for (size_t r = 0; r < N; ++r) {
                    const int D = d[r];
                    lines[((size_t)i * wtr::PIPE_Q + q) * N + r] =
                        i < D ? ring[((size_t)((head[r] + 1 + i) % (D + 1)) * wtr::PIPE_Q + q) * N + r] : NAN;
                }
    return WT_OK;
}

int wt_ensemble_pipe_clear(wt_ensemble *h)
{
    if (!h) return fail(WT_E_ARG, "NULL handle");
    if (!h->trn.pipe.on) return WT_OK;
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipStreamSynchronize(h->stream));   // queued launches may still use the lines
    pipe_release(h);
    return WT_OK;
}

int wt_junction_check(int length, int64_t n_reactors, const double *train_params, const double *params, const double *carry)
{
    if (n_reactors < 1) return fail(WT_E_ARG, "n_reactors must be >= 1");
    if (length < 2 || length > 32) return fail(WT_E_ARG, "length must be in 2..32 (the length of the train program)");
    if (!train_params || !params || !carry) return fail(WT_E_ARG, "NULL argument");
    const char *msg = junction_error(length, n_reactors, params, carry,
                                     [&](int64_t r) { return train_params[WT_TR_LINK * n_reactors + r] == 1.0; });
    return msg ? fail(WT_E_ARG, msg) : WT_OK;
}

int wt_ensemble_junction_set(wt_ensemble *h, const double *params, const double *carry)
{
    if (!h) return fail(WT_E_ARG, "NULL handle");
    if (!h->trn.on) return fail(WT_E_STATE, k_train_not_set);
    if (h->trn.pipe.on) return fail(WT_E_STATE, k_junction_pipes);
    if (!params || !carry) return fail(WT_E_ARG, "NULL argument");
    const int64_t N = h->N;
    const int length = h->trn.length;
    if (const char *msg = junction_error(length, N, params, carry, [&](int64_t r) { return h->trn_lk[(size_t)r] != 0; }))
        return fail(WT_E_ARG, msg);
    std::vector<uint32_t> src((size_t)N, 0);
    std::vector<double> share((size_t)N * wtr::JCT_SLOTS, 0.0), st((size_t)N * wtr::NJS, 0.0);
    bool carries = false;
    for (int64_t r = 0; r < N; ++r) {
        for (int k = 0; k < WT_JCT_SLOTS; ++k) {
            const double g = params[((int64_t)k * WT_NJ + WT_J_STAGE) * N + r];
            if (g >= 0.0) {
                src[(size_t)r] |= wtr::jct_slot_word(k, (int)g);
                share[(size_t)(k * N + r)] = params[((int64_t)k * WT_NJ + WT_J_SHARE) * N + r];
            }
        }
        if (carry[r] == 1.0) { src[(size_t)r] |= wtr::JCT_CARRY; carries = true; }
        st[(size_t)r * wtr::NJS + wtr::JS_Q_LAST] = NAN;
    }
    if (carries && h->sens.plc_on) return fail(WT_E_STATE, k_junction_plant_io);
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipStreamSynchronize(h->stream));   // queued launches may still use the old records
    if (h->trn.jct.on) {                        // set replaces a program: its rows and carried flows go back to the bases first
        if (int rc = train_op(h, wtr::OP_RESTORE)) return rc;
        if (int rc = sync_checked(h)) return rc;
        h->trn.jct.on = 0;
    }
    const size_t n = (size_t)N;
    HIP_TRY(hipMemcpyAsync((void *)h->trn.jct.src, src.data(), sizeof(uint32_t) * n, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipMemcpyAsync((void *)h->trn.jct.share, share.data(), sizeof(double) * share.size(), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipMemcpyAsync(h->trn.jct.st, st.data(), sizeof(double) * st.size(), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipMemcpyAsync(h->trn.jct.base0, h->bc, sizeof(double) * n, hipMemcpyDeviceToDevice, h->stream));
    h->trn.jct.on = 1;
    int rc = train_op(h, wtr::OP_RESTORE);      // the rows a plain link fed go back too: a junction with Qs = 0 keeps its base
    if (rc == WT_OK) rc = train_op(h, wtr::OP_FEED);
    if (rc == WT_OK) rc = sync_checked(h);      // the host vectors are freed on return
    if (rc != WT_OK) { (void)hipStreamSynchronize(h->stream); h->trn.jct.on = 0; return rc; }
    return WT_OK;
}

int wt_ensemble_junction_get(wt_ensemble *h, double *state)
{
    if (!h) return fail(WT_E_ARG, "NULL handle");
    if (!h->trn.jct.on) return fail(WT_E_STATE, k_junction_not_set);
    HIP_TRY(hipSetDevice(h->device));
    return download_records(h, {{state, h->trn.jct.st, wtr::NJS, 1, wtr::NJS}});
}

int wt_ensemble_junction_params(wt_ensemble *h, double *params, double *carry)
{
    if (!h || !params || !carry) return fail(WT_E_ARG, "NULL argument");
    if (!h->trn.jct.on) return fail(WT_E_STATE, k_junction_not_set);
    HIP_TRY(hipSetDevice(h->device));
    const size_t N = (size_t)h->N;
    std::vector<uint32_t> src;
    std::vector<double> share(N * wtr::JCT_SLOTS);
    if (int rc = junction_words(h, src)) return rc;
    if (int rc = download(h, {{share.data(), h->trn.jct.share, sizeof(double) * share.size()}})) return rc;
    for (size_t r = 0; r < N; ++r) {
        for (int k = 0; k < WT_JCT_SLOTS; ++k) {
            const uint32_t c = src[r] >> (wtr::JCT_BITS * k);
            const bool used = (c & wtr::JCT_USED) != 0;
            params[((size_t)k * WT_NJ + WT_J_STAGE) * N + r] = used ? (double)(c & 31u) : -1.0;
            params[((size_t)k * WT_NJ + WT_J_SHARE) * N + r] = used ? share[(size_t)k * N + r] : 0.0;
        }
        carry[r] = (src[r] & wtr::JCT_CARRY) ? 1.0 : 0.0;
    }
    return WT_OK;
}

int wt_ensemble_junction_clear(wt_ensemble *h)
{
    if (!h) return fail(WT_E_ARG, "NULL handle");
    if (!h->trn.jct.on) return WT_OK;
    if (h->trn.pipe.on) return fail(WT_E_STATE, k_junction_pipes);
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipStreamSynchronize(h->stream));   // queued launches may still use the records
    if (int rc = train_op(h, wtr::OP_RESTORE)) return rc;    // the bases back, carried flows included
    h->trn.jct.on = 0;
    if (int rc = train_op(h, wtr::OP_FEED)) return rc;       // then every link as the train program feeds it
    return sync_checked(h);
}

// wt_service_check and wt_tune_check: wt_program_check under the names and in the words the two programs came with
static int named_check(int program, int64_t n_reactors, const double *params)
{
    if (n_reactors < 1) return fail(WT_E_ARG, "n_reactors must be >= 1");
    if (!params) return fail(WT_E_ARG, "NULL argument");
    return wt_program_check(program, params, n_reactors);
}

int wt_service_check(int64_t n_reactors, const double *params) { return named_check(WT_PROG_SERVICE, n_reactors, params); }

int wt_ensemble_service_set(wt_ensemble *h, const double *params)
{
    if (int rc = check_program_set(h, WT_PROG_SERVICE, params)) return rc;
    if (int rc = wt_program_check(WT_PROG_SERVICE, params, h->N)) return rc;
    return load_program(h, WT_PROG_SERVICE, params);
}

int wt_ensemble_service_get(wt_ensemble *h, double *state)
{
    if (!h) return fail(WT_E_ARG, "NULL handle");
    return get_program(h, WT_PROG_SERVICE, {{state, h->sens.svc_st, wtsv::ST_DOUBLES, wtsv::SLOTS, wtsv::NSVS}});
}

int wt_ensemble_service_params(wt_ensemble *h, double *params) { return wt_ensemble_program_params(h, WT_PROG_SERVICE, params); }
int wt_ensemble_service_reset(wt_ensemble *h) { return reset_program(h, WT_PROG_SERVICE); }
int wt_ensemble_service_clear(wt_ensemble *h) { return stop_program(h, WT_PROG_SERVICE); }

// ---- the installation of the sensor suite: not a program of k_programs (no slots, no state, no zone limit)

int wt_install_check(int64_t n_reactors, const double *params)
{
    if (n_reactors < 1) return fail(WT_E_ARG, "n_reactors must be >= 1");
    if (!params) return fail(WT_E_ARG, "NULL argument");
    const std::string msg = install_error(n_reactors, params);
    return msg.empty() ? WT_OK : fail(WT_E_ARG, msg);
}

int wt_ensemble_install_set(wt_ensemble *h, const double *params)
{
    if (!h || !params) return fail(WT_E_ARG, "NULL argument");
    if (!h->sens.on) return fail(WT_E_STATE, k_service_no_suite);
    if (int rc = wt_install_check(h->N, params)) return rc;
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipStreamSynchronize(h->stream));   // queued launches may still read the old records
    return install_load(h, params, 1);
}

int wt_ensemble_install_get(wt_ensemble *h, double *params)
{
    if (!h || !params) return fail(WT_E_ARG, "NULL argument");
    if (!h->sens.on) return fail(WT_E_STATE, k_service_no_suite);
    HIP_TRY(hipSetDevice(h->device));
    std::vector<double> rec((size_t)h->N * wtin::REC_DOUBLES);
    if (int rc = download(h, {{rec.data(), h->ins.par, sizeof(double) * rec.size()}})) return rc;
    records_to_blocks(rec.data() + wtin::R_PARAMS, wtin::REC_DOUBLES, 1, wtin::NINS, h->N, params);
    return WT_OK;
}

int wt_ensemble_install_clear(wt_ensemble *h)
{
    if (!h) return fail(WT_E_ARG, "NULL handle");
    if (!h->sens.on) return WT_OK;              // no suite: nothing is set
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipStreamSynchronize(h->stream));   // queued launches may still read the records
    return install_load(h, nullptr, 0);
}

int wt_tune_check(int64_t n_reactors, const double *params) { return named_check(WT_PROG_TUNE, n_reactors, params); }

int wt_ensemble_tune_set(wt_ensemble *h, const double *params)
{
    if (int rc = check_program_set(h, WT_PROG_TUNE, params)) return rc;
    if (int rc = wt_program_check(WT_PROG_TUNE, params, h->N)) return rc;
    return load_program(h, WT_PROG_TUNE, params);
}

int wt_ensemble_tune_get(wt_ensemble *h, double *state)
{
    if (!h) return fail(WT_E_ARG, "NULL handle");
    return get_program(h, WT_PROG_TUNE, {{state, h->tun.st, wtu::ST_DOUBLES, wtu::LOOPS, wtu::NUS}});
}

int wt_ensemble_tune_params(wt_ensemble *h, double *params) { return wt_ensemble_program_params(h, WT_PROG_TUNE, params); }
int wt_ensemble_tune_reset(wt_ensemble *h) { return reset_program(h, WT_PROG_TUNE); }
int wt_ensemble_tune_clear(wt_ensemble *h) { return stop_program(h, WT_PROG_TUNE); }

// ---- model predictive control (wt_mpc.hpp): not a program of k_programs (three blocks, a prediction of
// its own); its arrays are plant I/O's, as the tune program's are

static_assert(WT_MPC_LOOPS == wtm::LOOPS && WT_NM == wtm::NM && WT_NMS == wtm::NMS && WT_MPC_H == wtm::H &&
              WT_MPC_ENABLE == wtm::M_ENABLE && WT_MPC_SENSOR == wtm::M_SENSOR && WT_MPC_SETPOINT == wtm::M_SETPOINT &&
              WT_MPC_EVERY == wtm::M_EVERY && WT_MPC_HORIZON == wtm::M_HORIZON && WT_MPC_U0 == wtm::M_U0 &&
              WT_MPC_OUT_MIN == wtm::M_OUT_MIN && WT_MPC_OUT_MAX == wtm::M_OUT_MAX && WT_MPC_DU_MAX == wtm::M_DU_MAX &&
              WT_MPC_T_START == wtm::M_T_START && WT_MPCS_PHASE == wtm::MS_PHASE && WT_MPCS_OUTPUT == wtm::MS_OUTPUT &&
              WT_MPCS_COUNT == wtm::MS_COUNT && WT_MPCS_BIAS == wtm::MS_BIAS && WT_MPCS_MOVE == wtm::MS_MOVE &&
              WT_MPCS_T_EXEC == wtm::MS_T_EXEC && WT_MPCS_ISE == wtm::MS_ISE && WT_MPCS_IAE == wtm::MS_IAE &&
              WT_MPCS_DOSE == wtm::MS_DOSE && WT_MPCS_N_EXEC == wtm::MS_N_EXEC && WT_MPCS_N_HELD == wtm::MS_N_HELD &&
              WT_MPCS_N_SAT == wtm::MS_N_SAT && WT_MPCS_N_RATE == wtm::MS_N_RATE && WT_MPCS_N_SKIPPED == wtm::MS_N_SKIPPED &&
              WT_MPC_WAITING == wtm::PH_WAITING && WT_MPC_RUNNING == wtm::PH_RUNNING && WT_INFO_MPC == 25, "model predictive control blocks of the C ABI");

static const char *const k_mpc_not_set = "no model predictive controller is set (wt_ensemble_mpc_set)";

// The first refusal of the three blocks, loop by loop over the reactors and at one loop of one reactor rule by rule in the
// header's order; empty: none.
static std::string mpc_error(int64_t N, const double *p, const double *step, const double *gain)
{
    for (int l = 0; l < WT_MPC_LOOPS; ++l)
        for (int64_t r = 0; r < N; ++r) {
            const auto at = [&](int k) { return p[((int64_t)l * WT_NM + k) * N + r]; };
            const auto row = [&](const double *b, int i) { return b[((int64_t)l * WT_MPC_H + i) * N + r]; };
            const auto rule = [&]() -> const char * {
                if (!whole_in(at(WT_MPC_ENABLE), 0, 1)) return "enable must be 0 or 1";
                if (!whole_in(at(WT_MPC_SENSOR), 0, WT_N_SENSORS - 1)) return "sensor must be an integer in 0..6";
                if (!whole_in(at(WT_MPC_EVERY), 1, 9007199254740991.0)) return "every must be a whole number >= 1";
                if (!whole_in(at(WT_MPC_HORIZON), 1, WT_MPC_H)) return "horizon must be an integer in 1..64";
                if (!(std::isfinite(at(WT_MPC_SETPOINT)) && std::isfinite(at(WT_MPC_U0)))) return "setpoint and u0 must be finite";
                if (!(std::isfinite(at(WT_MPC_OUT_MIN)) && std::isfinite(at(WT_MPC_OUT_MAX)) && at(WT_MPC_OUT_MIN) <= at(WT_MPC_OUT_MAX)))
                    return "out_min and out_max must be finite and out_min <= out_max";
                if (!(at(WT_MPC_DU_MAX) > 0.0)) return "du_max must be > 0 (+inf: no limit)";
                if (std::isnan(at(WT_MPC_T_START))) return "t_start must not be NaN";
                if (at(WT_MPC_ENABLE) == 0.0) return nullptr;      // the model of a loop that is off is not read
                for (int i = 0; i < WT_MPC_H; ++i)
                    if (!(std::isfinite(row(step, i)) && std::isfinite(row(gain, i)))) return "step and gain must be finite";
                bool any = false;
                for (int i = 0; i < (int)at(WT_MPC_HORIZON); ++i) any = any || row(gain, i) != 0.0;
                return any ? nullptr : "gain must not be all zero over the horizon";
            };
            if (const char *msg = rule()) return std::string(msg) + " (loop " + std::to_string(l) + ", reactor " + std::to_string(r) + ")";
        }
    return std::string();
}

int wt_mpc_check(int64_t n_reactors, const double *params, const double *step, const double *gain)
{
    if (n_reactors < 1) return fail(WT_E_ARG, "n_reactors must be >= 1");
    if (!params || !step || !gain) return fail(WT_E_ARG, "NULL argument");
    const std::string msg = mpc_error(n_reactors, params, step, gain);
    return msg.empty() ? WT_OK : fail(WT_E_ARG, msg);
}

// every controller waiting: state and prediction all 0 (the stream is idle)
static int mpc_restart(wt_ensemble *h)
{
    HIP_TRY(hipMemsetAsync(h->mpc.st, 0, sizeof(double) * wtm::ST_DOUBLES * (size_t)h->N, h->stream));
    HIP_TRY(hipMemsetAsync(h->mpc.pred, 0, sizeof(double) * wtm::ROW_DOUBLES * (size_t)h->N, h->stream));
    return WT_OK;
}

int wt_ensemble_mpc_set(wt_ensemble *h, const double *params, const double *step, const double *gain)
{
    if (!h || !params || !step || !gain) return fail(WT_E_ARG, "NULL argument");
    if (!h->sens.plc_on) return fail(WT_E_STATE, "model predictive controllers act on the plant I/O scan: enable plant I/O first");
    if (!wt::prog_in_item(levels_for(h->n))) return fail(WT_E_STATE, "model predictive controllers run in the kernels for up to 32 zones");
    if (int rc = wt_mpc_check(h->N, params, step, gain)) return rc;
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipStreamSynchronize(h->stream));   // queued launches may still read or write the old records
    const int64_t N = h->N;
    std::vector<double> par((size_t)N * wtm::PAR_DOUBLES), sr((size_t)N * wtm::ROW_DOUBLES), gr((size_t)N * wtm::ROW_DOUBLES);
    blocks_to_records(params, wtm::LOOPS, wtm::NM, N, par.data(), wtm::PAR_DOUBLES);
    blocks_to_records(step, wtm::LOOPS, wtm::H, N, sr.data(), wtm::ROW_DOUBLES);
    blocks_to_records(gain, wtm::LOOPS, wtm::H, N, gr.data(), wtm::ROW_DOUBLES);
    int rc = upload(h, (double *)h->mpc.par, par);
    if (rc == WT_OK) rc = upload(h, (double *)h->mpc.step, sr);
    if (rc == WT_OK) rc = upload(h, (double *)h->mpc.gain, gr);
    if (rc == WT_OK) rc = mpc_restart(h);
    if (rc == WT_OK) rc = sync_checked(h);      // the host vectors are freed on return
    h->mpc.on = rc == WT_OK ? 1 : 0;
    return rc;
}

static int mpc_ready(wt_ensemble *h)
{
    if (!h) return fail(WT_E_ARG, "NULL handle");
    if (!h->mpc.on) return fail(WT_E_STATE, k_mpc_not_set);
    HIP_TRY(hipSetDevice(h->device));
    return WT_OK;
}

int wt_ensemble_mpc_get(wt_ensemble *h, double *state)
{
    if (int rc = mpc_ready(h)) return rc;
    return download_records(h, {{state, h->mpc.st, wtm::ST_DOUBLES, wtm::LOOPS, wtm::NMS}});
}

int wt_ensemble_mpc_prediction(wt_ensemble *h, double *pred)
{
    if (int rc = mpc_ready(h)) return rc;
    return download_records(h, {{pred, h->mpc.pred, wtm::ROW_DOUBLES, wtm::LOOPS, wtm::H}});
}

int wt_ensemble_mpc_params(wt_ensemble *h, double *params, double *step, double *gain)
{
    if (int rc = mpc_ready(h)) return rc;
    return download_records(h, {{params, h->mpc.par, wtm::PAR_DOUBLES, wtm::LOOPS, wtm::NM},
                                {step, h->mpc.step, wtm::ROW_DOUBLES, wtm::LOOPS, wtm::H},
                                {gain, h->mpc.gain, wtm::ROW_DOUBLES, wtm::LOOPS, wtm::H}});
}

int wt_ensemble_mpc_reset(wt_ensemble *h)
{
    if (int rc = mpc_ready(h)) return rc;
    HIP_TRY(hipStreamSynchronize(h->stream));   // queued launches may still write the records
    if (int rc = mpc_restart(h)) return rc;
    return sync_checked(h);
}

int wt_ensemble_mpc_clear(wt_ensemble *h)
{
    if (!h) return fail(WT_E_ARG, "NULL handle");
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipStreamSynchronize(h->stream));   // queued launches may still use the records
    h->mpc.on = 0;
    return WT_OK;
}

// ---- response programs (wt_rsp.hpp): not programs of k_programs (they read the alarm and detector
// programs' records and write the controllers'); their arrays are plant I/O's, as the tune program's are

static_assert(WT_RSP_SLOTS == wtrp::SLOTS && WT_NR == wtrp::NR && WT_NRS == wtrp::NRS && WT_NRR == wtrp::NRR &&
              WT_RSP_CAUSE == wtrp::R_CAUSE && WT_RSP_INDEX == wtrp::R_INDEX && WT_RSP_DELAY == wtrp::R_DELAY &&
              WT_RSP_LOOP == wtrp::R_LOOP && WT_RSP_ACTION == wtrp::R_ACTION && WT_RSP_VALUE == wtrp::R_VALUE &&
              WT_RSP_RATE == wtrp::R_RATE && WT_RSP_LATCH == wtrp::R_LATCH && WT_RSP_CLEAR_DELAY == wtrp::R_CLEAR_DELAY &&
              WT_RSP_MIN_HOLD == wtrp::R_MIN_HOLD && WT_RSP_HANDBACK == wtrp::R_HANDBACK && WT_RSPS_PHASE == wtrp::RS_PHASE &&
              WT_RSPS_PENDING == wtrp::RS_PENDING && WT_RSPS_CLEARING == wtrp::RS_CLEARING && WT_RSPS_OUTPUT == wtrp::RS_OUTPUT &&
              WT_RSPS_T_FIRST == wtrp::RS_T_FIRST && WT_RSPS_T_ENGAGED == wtrp::RS_T_ENGAGED &&
              WT_RSPS_T_RELEASED == wtrp::RS_T_RELEASED && WT_RSPS_N_ENGAGED == wtrp::RS_N_ENGAGED &&
              WT_RSPS_TIME_ENGAGED == wtrp::RS_TIME_ENGAGED && WT_RSPS_N_OWNED == wtrp::RS_N_OWNED &&
              WT_RSPS_N_BLOCKED == wtrp::RS_N_BLOCKED && WT_RSPS_N_CAUSE == wtrp::RS_N_CAUSE &&
              WT_RSPS_N_TRACKED == wtrp::RS_N_TRACKED && WT_RSPS_N_HANDBACK == wtrp::RS_N_HANDBACK &&
              WT_RSPR_T_PREV == wtrp::RR_T_PREV && WT_RSPR_OWNER_CHLORINE == wtrp::RR_OWNER_CHLORINE &&
              WT_RSPR_OWNER_ACID == wtrp::RR_OWNER_ACID && WT_RSP_OFF == wtrp::C_OFF && WT_RSP_ALARM == wtrp::C_ALARM &&
              WT_RSP_DETECTOR == wtrp::C_DETECTOR && WT_RSP_BAD == wtrp::C_BAD && WT_RSP_HOLD == wtrp::ACT_HOLD &&
              WT_RSP_MANUAL == wtrp::ACT_MANUAL && WT_RSP_RAMP == wtrp::ACT_RAMP && WT_RSP_BUMP == wtrp::HB_BUMP &&
              WT_RSP_BUMPLESS == wtrp::HB_BUMPLESS && WT_RSP_IDLE == wtrp::PH_IDLE && WT_RSP_ENGAGED == wtrp::PH_ENGAGED &&
              WT_INFO_RESPOND == 26, "response program blocks of the C ABI");

static const char *const k_respond_not_set = "no response program is set (wt_ensemble_respond_set)";

// one slot of one reactor, rule by rule in the header's order
static const char *respond_rule(const double *c)
{
    if (!whole_in(c[WT_RSP_CAUSE], 0, wtrp::N_CAUSES - 1)) return "cause must be 0 (off), 1 (alarm), 2 (detector) or 3 (bad)";
    if (c[WT_RSP_CAUSE] == (double)WT_RSP_OFF) return nullptr;     // the other rows of a slot that is off are not read
    if (c[WT_RSP_CAUSE] == (double)WT_RSP_ALARM && !whole_in(c[WT_RSP_INDEX], 0, wta::SLOTS - 1))
        return "an ALARM cause's index must be an alarm slot in 0..3";
    if (c[WT_RSP_CAUSE] == (double)WT_RSP_DETECTOR && !whole_in(c[WT_RSP_INDEX], 0, wtk::SLOTS - 1))
        return "a DETECTOR cause's index must be a detector slot in 0..3";
    if (c[WT_RSP_CAUSE] == (double)WT_RSP_BAD && !whole_in(c[WT_RSP_INDEX], 0, WT_N_SENSORS - 1))
        return "a BAD cause's index must be a sensor index in 0..6";
    if (!whole_in(c[WT_RSP_LOOP], 0, wtrp::LOOPS - 1)) return "loop must be 0 (chlorine) or 1 (acid)";
    if (!whole_in(c[WT_RSP_ACTION], 0, wtrp::N_ACTIONS - 1)) return "action must be 0 (hold), 1 (manual) or 2 (ramp)";
    if (!whole_in(c[WT_RSP_LATCH], 0, 1)) return "latch must be 0 or 1";
    if (!whole_in(c[WT_RSP_HANDBACK], 0, 1)) return "handback must be 0 (bump) or 1 (bumpless)";
    for (const int f : {WT_RSP_DELAY, WT_RSP_CLEAR_DELAY, WT_RSP_MIN_HOLD, WT_RSP_RATE})
        if (!(c[f] >= 0.0)) return "delay, clear_delay, min_hold and rate must be >= 0 and not NaN";
    if (!(c[WT_RSP_VALUE] >= 0.0 && c[WT_RSP_VALUE] <= k_command_limit[(int)c[WT_RSP_LOOP]]))
        return "value must be within 0 and the loop's command limit (1.0 chlorine, 2.0 acid)";
    return nullptr;
}

int wt_respond_check(int64_t n_reactors, const double *params)
{
    if (n_reactors < 1) return fail(WT_E_ARG, "n_reactors must be >= 1");
    if (!params) return fail(WT_E_ARG, "NULL argument");
    double c[WT_NR];
    for (int s = 0; s < WT_RSP_SLOTS; ++s)
        for (int64_t r = 0; r < n_reactors; ++r) {
            for (int k = 0; k < WT_NR; ++k) c[k] = params[((int64_t)s * WT_NR + k) * n_reactors + r];
            if (const char *msg = respond_rule(c))
                return fail(WT_E_ARG, std::string(msg) + " (slot " + std::to_string(s) + ", reactor " + std::to_string(r) + ")");
        }
    return WT_OK;
}

// every slot idle: counts 0, times NaN, no owner, t_prev the loop time
static int respond_restart(wt_ensemble *h)
{
    const int64_t N = h->N;
    std::vector<double> st((size_t)N * wtrp::ST_DOUBLES, 0.0), rst((size_t)N * wtrp::RST_DOUBLES, 0.0), lt;
    for (size_t i = 0; i < st.size(); i += wtrp::NRS) {
        double *q = st.data() + i;
        q[wtrp::RS_PENDING] = q[wtrp::RS_CLEARING] = q[wtrp::RS_T_FIRST] = q[wtrp::RS_T_ENGAGED] = q[wtrp::RS_T_RELEASED] = NAN;
    }
    if (int rc = loop_time(h, lt)) return rc;       // (the download also waits for queued launches)
    for (int64_t r = 0; r < N; ++r) {
        double *q = rst.data() + r * wtrp::RST_DOUBLES;
        q[wtrp::RR_T_PREV] = lt[(size_t)r]; q[wtrp::RR_OWNER_CHLORINE] = q[wtrp::RR_OWNER_ACID] = -1.0;
    }
    if (int rc = upload(h, h->rsp.st, st)) return rc;
    if (int rc = upload(h, h->rsp.rst, rst)) return rc;
    HIP_TRY(hipStreamSynchronize(h->stream));   // the host vectors are freed on return
    return WT_OK;
}

int wt_ensemble_respond_set(wt_ensemble *h, const double *params)
{
    if (!h || !params) return fail(WT_E_ARG, "NULL argument");
    if (!h->sens.plc_on) return fail(WT_E_STATE, "response programs act on the plant I/O scan: enable plant I/O first");
    if (!wt::prog_in_item(levels_for(h->n))) return fail(WT_E_STATE, "response programs run in the kernels for up to 32 zones");
    if (int rc = wt_respond_check(h->N, params)) return rc;
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipStreamSynchronize(h->stream));   // queued launches may still read or write the old records
    std::vector<double> par((size_t)h->N * wtrp::PAR_DOUBLES);
    blocks_to_records(params, wtrp::SLOTS, wtrp::NR, h->N, par.data(), wtrp::PAR_DOUBLES);
    int rc = upload(h, (double *)h->rsp.par, par);
    if (rc == WT_OK) rc = respond_restart(h);
    if (rc == WT_OK) rc = sync_checked(h);      // the host vector is freed on return
    h->rsp.on = rc == WT_OK ? 1 : 0;
    return rc;
}

static int respond_ready(wt_ensemble *h)
{
    if (!h) return fail(WT_E_ARG, "NULL handle");
    if (!h->rsp.on) return fail(WT_E_STATE, k_respond_not_set);
    HIP_TRY(hipSetDevice(h->device));
    return WT_OK;
}

int wt_ensemble_respond_state(wt_ensemble *h, double *state, double *reactor_state)
{
    if (int rc = respond_ready(h)) return rc;
    return download_records(h, {{state, h->rsp.st, wtrp::ST_DOUBLES, wtrp::SLOTS, wtrp::NRS},
                                {reactor_state, h->rsp.rst, wtrp::RST_DOUBLES, 1, wtrp::NRR}});
}

int wt_ensemble_respond_params(wt_ensemble *h, double *params)
{
    if (int rc = respond_ready(h)) return rc;
    return download_records(h, {{params, h->rsp.par, wtrp::PAR_DOUBLES, wtrp::SLOTS, wtrp::NR}});
}

int wt_ensemble_respond_reset(wt_ensemble *h)
{
    if (int rc = respond_ready(h)) return rc;
    if (int rc = respond_restart(h)) return rc;
    return sync_checked(h);
}

int wt_ensemble_respond_clear(wt_ensemble *h)
{
    if (!h) return fail(WT_E_ARG, "NULL handle");
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipStreamSynchronize(h->stream));   // queued launches may still use the records
    h->rsp.on = 0;
    return WT_OK;
}

// ---- link programs (wt_lnk.hpp): not programs of k_programs (a seed beside the block, rings beside the
// state); their arrays are plant I/O's, as the response programs' are

static_assert(WT_LNK_SLOTS == wtl::SLOTS && WT_LNK_DEPTH == wtl::DEPTH && WT_NL == wtl::NL && WT_NLS == wtl::NLS &&
              WT_LNK_MODE == wtl::L_MODE && WT_LNK_TARGET == wtl::L_TARGET && WT_LNK_START == wtl::L_START &&
              WT_LNK_END == wtl::L_END && WT_LNK_A == wtl::L_A && WT_LNK_B == wtl::L_B && WT_LNK_TIMEOUT == wtl::L_TIMEOUT &&
              WT_LNK_FAIL == wtl::L_FAIL && WT_LNKS_N_REC == wtl::LS_N_REC && WT_LNKS_N_APPLIED == wtl::LS_N_APPLIED &&
              WT_LNKS_N_FRESH == wtl::LS_N_FRESH && WT_LNKS_N_LOST == wtl::LS_N_LOST && WT_LNKS_N_TIMEOUT == wtl::LS_N_TIMEOUT &&
              WT_LNKS_N_DRAW == wtl::LS_N_DRAW && WT_LNKS_T_FRESH == wtl::LS_T_FRESH && WT_LNKS_HELD_VALUE == wtl::LS_HELD_VALUE &&
              WT_LNKS_HELD_FAULT == wtl::LS_HELD_FAULT && WT_LNKS_TAPE_END == wtl::LS_TAPE_END && WT_LNK_OFF == wtl::M_OFF &&
              WT_LNK_DELAY == wtl::M_DELAY && WT_LNK_LOSS == wtl::M_LOSS && WT_LNK_REPLAY == wtl::M_REPLAY &&
              WT_INFO_LINK == 27, "link program blocks of the C ABI");

static const char *const k_link_not_set = "no link program is set (wt_ensemble_link_set)";

// one slot of one reactor, rule by rule in the header's order
static const char *link_rule(const double *c)
{
    const double mode = c[WT_LNK_MODE], a = c[WT_LNK_A], b = c[WT_LNK_B], timeout = c[WT_LNK_TIMEOUT], fl = c[WT_LNK_FAIL];
    if (!whole_in(mode, 0, wtl::N_MODES - 1)) return "mode must be 0 (off), 1 (delay), 2 (loss) or 3 (replay)";
    if (!whole_in(c[WT_LNK_TARGET], 0, wtl::N_TARGETS - 1)) return "target must be an integer in 0..9";
    if (!std::isfinite(c[WT_LNK_START]) || std::isnan(c[WT_LNK_END])) return "start must be finite and end a number (end may be +inf)";
    if (!(c[WT_LNK_START] <= c[WT_LNK_END])) return "start must not exceed end";
    const bool no_timeout = timeout == INFINITY;
    if (mode == (double)WT_LNK_OFF) {
        if (a != 0.0 || b != 0.0 || !no_timeout || fl != 0.0) return "a slot that is off takes no a, b, timeout or fail";
    } else if (mode == (double)WT_LNK_DELAY) {
        if (!whole_in(a, 0, wtl::DEPTH - 1) || !whole_in(b, 0, wtl::DEPTH - 1) || a + b > wtl::DEPTH - 1)
            return "a DELAY slot's delay (a) and jitter (b) must be whole numbers of scans with a + b <= 63";
        if (!no_timeout || fl != 0.0) return "a DELAY slot takes no timeout or fail";
    } else if (mode == (double)WT_LNK_LOSS) {
        if (!(a >= 0.0 && a <= 1.0)) return "a LOSS slot's probability (a) must be within 0 and 1";
        if (b != 0.0) return "a LOSS slot takes no b";
        if (!(timeout >= 0.0)) return "a LOSS slot's timeout must be >= 0 or +inf";
        if (no_timeout) {
            if (fl != 0.0) return "a LOSS slot without a timeout takes no fail";
        } else if (c[WT_LNK_TARGET] < (double)wtl::CMD_ACID) {
            if (!whole_in(fl, 1, 6)) return "a LOSS slot on a reading fails to a fault code (fail) in 1..6";
        } else if (!std::isfinite(fl)) {
            return "a LOSS slot on a command fails to a finite value (fail)";
        }
    } else {
        if (!whole_in(a, 1, wtl::DEPTH - 1)) return "a REPLAY slot's tape length (a) must be a whole number of scans in 1..63";
        if (b != 0.0 || !no_timeout || fl != 0.0) return "a REPLAY slot takes no b, timeout or fail";
    }
    return nullptr;
}

int wt_link_check(int64_t n_reactors, const double *params)
{
    if (n_reactors < 1) return fail(WT_E_ARG, "n_reactors must be >= 1");
    if (!params) return fail(WT_E_ARG, "NULL argument");
    double c[WT_NL];
    for (int s = 0; s < WT_LNK_SLOTS; ++s)
        for (int64_t r = 0; r < n_reactors; ++r) {
            for (int k = 0; k < WT_NL; ++k) c[k] = params[((int64_t)s * WT_NL + k) * n_reactors + r];
            if (const char *msg = link_rule(c))
                return fail(WT_E_ARG, std::string(msg) + " (slot " + std::to_string(s) + ", reactor " + std::to_string(r) + ")");
        }
    return WT_OK;
}

// every slot as set leaves it: counts and held_fault 0, t_fresh, held_value and tape_end NaN, the rings zeroed
static int link_restart(wt_ensemble *h)
{
    const size_t N = (size_t)h->N;
    std::vector<double> st(N * wtl::ST_DOUBLES, 0.0);
    for (size_t i = 0; i < st.size(); i += wtl::NLS) {
        double *q = st.data() + i;
        q[wtl::LS_T_FRESH] = q[wtl::LS_HELD_VALUE] = q[wtl::LS_TAPE_END] = NAN;
    }
    if (int rc = upload(h, h->lnk.st, st)) return rc;
    HIP_TRY(hipMemsetAsync(h->lnk.ring, 0, sizeof(double) * wtl::RING_ENTRIES * N, h->stream));
    HIP_TRY(hipMemsetAsync(h->lnk.fring, 0, sizeof(uint8_t) * wtl::RING_ENTRIES * N, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));   // the host vector is freed on return
    return WT_OK;
}

int wt_ensemble_link_set(wt_ensemble *h, const double *params, uint64_t seed)
{
    if (!h || !params) return fail(WT_E_ARG, "NULL argument");
    if (!h->sens.plc_on) return fail(WT_E_STATE, "link programs act on the plant I/O scan: enable plant I/O first");
    if (!wt::prog_in_item(levels_for(h->n))) return fail(WT_E_STATE, "link programs run in the kernels for up to 32 zones");
    if (int rc = wt_link_check(h->N, params)) return rc;
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipStreamSynchronize(h->stream));   // queued launches may still read or write the old records
    std::vector<double> par((size_t)h->N * wtl::PAR_DOUBLES);
    blocks_to_records(params, wtl::SLOTS, wtl::NL, h->N, par.data(), wtl::PAR_DOUBLES);
    int rc = upload(h, (double *)h->lnk.par, par);
    if (rc == WT_OK) rc = link_restart(h);
    if (rc == WT_OK) rc = sync_checked(h);      // the host vector is freed on return
    h->lnk.seed_lo = (uint32_t)(seed & 0xffffffffu); h->lnk.seed_hi = (uint32_t)(seed >> 32);
    h->lnk.on = rc == WT_OK ? 1 : 0;
    return rc;
}

static int link_ready(wt_ensemble *h)
{
    if (!h) return fail(WT_E_ARG, "NULL handle");
    if (!h->lnk.on) return fail(WT_E_STATE, k_link_not_set);
    HIP_TRY(hipSetDevice(h->device));
    return WT_OK;
}

int wt_ensemble_link_state(wt_ensemble *h, double *state)
{
    if (int rc = link_ready(h)) return rc;
    return download_records(h, {{state, h->lnk.st, wtl::ST_DOUBLES, wtl::SLOTS, wtl::NLS}});
}

int wt_ensemble_link_params(wt_ensemble *h, double *params, uint64_t *seed)
{
    if (int rc = link_ready(h)) return rc;
    if (seed) *seed = ((uint64_t)h->lnk.seed_hi << 32) | h->lnk.seed_lo;
    return download_records(h, {{params, h->lnk.par, wtl::PAR_DOUBLES, wtl::SLOTS, wtl::NL}});
}

int wt_ensemble_link_ring(wt_ensemble *h, double *values, double *faults, double *n_rec)
{
    if (int rc = link_ready(h)) return rc;
    const int64_t N = h->N;
    const size_t E = (size_t)N * wtl::RING_ENTRIES;
    std::vector<double> ring(E), st((size_t)N * wtl::ST_DOUBLES);
    std::vector<uint8_t> fring(E);
    if (int rc = download(h, {{ring.data(), h->lnk.ring, sizeof(double) * E}, {fring.data(), h->lnk.fring, sizeof(uint8_t) * E},
                              {st.data(), h->lnk.st, sizeof(double) * st.size()}})) return rc;
    // recording order: entry k is the k-th oldest sample the ring still holds; entries past the count are NaN and 0
    for (int64_t r = 0; r < N; ++r)
        for (int s = 0; s < wtl::SLOTS; ++s) {
            const double c = st[(size_t)r * wtl::ST_DOUBLES + s * wtl::NLS + wtl::LS_N_REC];
            const uint64_t n = (c >= 0.0 && c < 4294967296.0) ? (uint64_t)c : 0;      // wtl::whole
            const uint64_t kept = n < (uint64_t)wtl::DEPTH ? n : (uint64_t)wtl::DEPTH;
            const size_t at = ((size_t)r * wtl::SLOTS + s) * wtl::DEPTH;
            for (int k = 0; k < wtl::DEPTH; ++k) {
                const size_t o = ((size_t)s * wtl::DEPTH + k) * N + r;
                const bool have = (uint64_t)k < kept;
                const size_t i = at + (size_t)((n - kept + k) & (wtl::DEPTH - 1));
                if (values) values[o] = have ? ring[i] : NAN;
                if (faults) faults[o] = have ? (double)fring[i] : 0.0;
            }
            if (n_rec) n_rec[(size_t)s * N + r] = c;
        }
    return WT_OK;
}

int wt_ensemble_link_reset(wt_ensemble *h)
{
    if (int rc = link_ready(h)) return rc;
    HIP_TRY(hipStreamSynchronize(h->stream));   // queued launches may still use the records
    if (int rc = link_restart(h)) return rc;
    return sync_checked(h);
}

int wt_ensemble_link_clear(wt_ensemble *h)
{
    if (!h) return fail(WT_E_ARG, "NULL handle");
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipStreamSynchronize(h->stream));   // queued launches may still use the records
    h->lnk.on = 0;
    return WT_OK;
}

int wt_ensemble_sensors_service(wt_ensemble *h, int sensor, int action, int ref_mode, const double *ref, const double *ref2,
                                const uint8_t *mask)
{
    if (!h) return fail(WT_E_ARG, "NULL handle");
    if (!h->sens.on) return fail(WT_E_STATE, k_service_no_suite);
    if (const char *msg = service_action_error((double)sensor, (double)action, (double)ref_mode)) return fail(WT_E_ARG, msg);
    const size_t N = (size_t)h->N;
    for (const double *v : {ref, ref2})
        for (size_t r = 0; v && r < N; ++r)
            if (!std::isfinite(v[r])) return fail(WT_E_ARG, "ref and ref2 must be finite");
    HIP_TRY(hipSetDevice(h->device));
    // one device block for what the call brings: ref, ref2, then the mask
    double *in = nullptr;
    HIP_TRY(hipMalloc((void **)&in, sizeof(double) * 2 * N + N));
    uint8_t *m = (uint8_t *)(in + 2 * N);
    hipError_t e = hipSuccess;
    if (ref) e = hipMemcpyAsync(in, ref, sizeof(double) * N, hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess && ref2) e = hipMemcpyAsync(in + N, ref2, sizeof(double) * N, hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess && mask) e = hipMemcpyAsync(m, mask, N, hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess) {
        const wtsv::ServiceArgs a{h->sens, h->pH, h->Cl, h->T, h->time, h->flow, h->n, sensor, action, ref_mode,
                                  ref ? in : nullptr, ref2 ? in + N : nullptr, mask ? m : nullptr};
        hipLaunchKernelGGL(wtsv::service_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, h->stream, a);
        e = hipGetLastError();
    }
    const int rc = e == hipSuccess ? sync_checked(h) : ((void)hipStreamSynchronize(h->stream), fail(WT_E_HIP, std::string("sensors_service: ") + hipGetErrorString(e)));
    (void)hipFree(in);
    return rc;
}

int wt_ensemble_sensors_health(wt_ensemble *h, double *out)
{
    if (!h || !out) return fail(WT_E_ARG, "NULL argument");
    if (!h->sens.on) return fail(WT_E_STATE, k_service_no_suite);
    HIP_TRY(hipSetDevice(h->device));
    const size_t N = (size_t)h->N;
    std::vector<float> fs(wts::NSENS * wts::NF * N);
    std::vector<double> ds(wts::NSENS * wts::ND * N);
    std::vector<int32_t> is(wts::NSENS * wts::NI * N);
    if (int rc = download(h, {{fs.data(), h->sens.fs, sizeof(float) * fs.size()}, {ds.data(), h->sens.ds, sizeof(double) * ds.size()},
                              {is.data(), h->sens.is, sizeof(int32_t) * is.size()}}))
        return rc;
    for (size_t i = 0; i < (size_t)wts::NSENS; ++i)
        for (size_t r = 0; r < N; ++r) {
            double *o = out + i * WT_NSH * N + r;
            const double *D = ds.data() + i * wts::ND * N + r;
            o[WT_SH_CAL_OFFSET * N] = (double)fs[(i * wts::NF + wts::F_CAL_OFFSET) * N + r];
            o[WT_SH_CAL_TIME * N] = D[wts::D_CAL_TIME * N]; o[WT_SH_POWER_ON * N] = D[wts::D_POWER_ON * N];
            o[WT_SH_SLOW0 * N] = D[wts::D_SLOW0 * N]; o[WT_SH_SLOW1 * N] = D[wts::D_SLOW1 * N]; o[WT_SH_SLOW2 * N] = D[wts::D_SLOW2 * N];
            o[WT_SH_STATUS * N] = (double)is[(i * wts::NI + wts::I_STATUS) * N + r];
            o[WT_SH_FAULT * N] = (double)is[(i * wts::NI + wts::I_FAULT) * N + r];
        }
    return WT_OK;
}

int wt_wire_check(int length, int64_t n_reactors, const double *params)
{
    if (n_reactors < 1) return fail(WT_E_ARG, "n_reactors must be >= 1");
    if (length < 2 || length > 32) return fail(WT_E_ARG, "length must be in 2..32 (the length of the train program)");
    if (!params) return fail(WT_E_ARG, "NULL argument");
    const char *msg = wire_error(length, n_reactors, params);
    return msg ? fail(WT_E_ARG, msg) : WT_OK;
}

int wt_ensemble_wire_set(wt_ensemble *h, const double *params)
{
    if (!h) return fail(WT_E_ARG, "NULL handle");
    if (!h->trn.on) return fail(WT_E_STATE, k_train_not_set);
    if (!h->sens.plc_on) return fail(WT_E_STATE, "wires carry readings into the plant I/O scan: enable plant I/O first");
    if (!params) return fail(WT_E_ARG, "params is NULL");
    const int64_t N = h->N;
    if (const char *msg = wire_error(h->trn.length, N, params)) return fail(WT_E_ARG, msg);
    std::vector<uint64_t> src((size_t)N, 0);
    for (int64_t r = 0; r < N; ++r)
        for (int i = 0; i < WT_NSENS; ++i) {
            const double g = params[((int64_t)i * WT_NW + WT_W_STAGE) * N + r];
            if (g >= 0.0) src[(size_t)r] |= wtw::slot_word(i, (int)g, (int)params[((int64_t)i * WT_NW + WT_W_SENSOR) * N + r]);
        }
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipStreamSynchronize(h->stream));   // queued launches may still use the old records
    int rc = allocate(wire_arrays(h));          // (those of a running program are used again: set replaces it)
    if (rc == WT_OK) {
        hipError_t e = hipMemcpyAsync((void *)h->wir.src, src.data(), sizeof(uint64_t) * (size_t)N, hipMemcpyHostToDevice, h->stream);
        if (e != hipSuccess) rc = fail(WT_E_HIP, hipGetErrorString(e));
        if (rc == WT_OK) rc = wire_restart(h);
        if (rc == WT_OK) rc = sync_checked(h);  // the host vector is freed on return
    }
    if (rc != WT_OK) { (void)hipStreamSynchronize(h->stream); wire_release(h); return rc; }
    h->wir.on = 1;
    return WT_OK;
}

int wt_ensemble_wire_get(wt_ensemble *h, double *params, double *state)
{
    if (!h) return fail(WT_E_ARG, "NULL handle");
    if (!h->wir.on) return fail(WT_E_STATE, k_wire_not_set);
    HIP_TRY(hipSetDevice(h->device));
    const size_t N = (size_t)h->N;
    std::vector<uint64_t> src(params ? N : 0);
    if (int rc = download(h, {{params ? src.data() : nullptr, h->wir.src, sizeof(uint64_t) * N}})) return rc;
    if (params)
        for (size_t r = 0; r < N; ++r)
            for (int i = 0; i < WT_NSENS; ++i) {
                const uint32_t c = (uint32_t)(src[r] >> (wtw::SLOT_BITS * i));
                const bool wired = (c & wtw::WIRED) != 0;
                params[((size_t)i * WT_NW + WT_W_STAGE) * N + r] = wired ? (double)((c >> 3) & 31u) : -1.0;
                params[((size_t)i * WT_NW + WT_W_SENSOR) * N + r] = wired ? (double)(c & 7u) : (double)i;
            }
    return download_records(h, {{state, h->wir.st, wtw::ST_DOUBLES, WT_NSENS, WT_NWS}});
}

int wt_ensemble_wire_clear(wt_ensemble *h)
{
    if (!h) return fail(WT_E_ARG, "NULL handle");
    if (!h->wir.on) return WT_OK;
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipStreamSynchronize(h->stream));   // queued launches may still use the records
    wire_release(h);
    return WT_OK;
}

int wt_ensemble_score_set(wt_ensemble *h, const double *params, int curve_capacity, int bins, const double *fan_lo, const double *fan_hi)
{
    if (int rc = check_program_set(h, WT_PROG_SCORE, params)) return rc;
    if (curve_capacity < 0) return fail(WT_E_ARG, "curve_capacity must be >= 0 (0 = no ensemble curve)");
    if (bins < 0 || bins > wtsc::MAX_BINS) return fail(WT_E_ARG, "bins must be in 0..32 (0 = no fan)");
    if (bins > 0 && (!fan_lo || !fan_hi)) return fail(WT_E_ARG, "a fan needs fan_lo and fan_hi");
    for (int k = 0; bins > 0 && k < wtsc::SLOTS; ++k)
        if (!(std::isfinite(fan_lo[k]) && std::isfinite(fan_hi[k]) && fan_lo[k] < fan_hi[k]))
            return fail(WT_E_ARG, "fan_lo < fan_hi, both finite, for every slot");
    int64_t cells = 0;
    if (__builtin_mul_overflow((int64_t)curve_capacity * wtsc::SLOTS * (int64_t)sizeof(int32_t), (int64_t)(bins + 2), &cells))
        return fail(WT_E_ARG, "curve size overflows int64");
    if (int rc = wt_program_check(WT_PROG_SCORE, params, h->N)) return rc;
    const int64_t N = h->N;
    for (int k = 0; k < wtsc::SLOTS; ++k)
        for (int64_t r = 0; r < N; ++r)
            if (params[((int64_t)k * wtsc::NSP + wtsc::P_ZONE) * N + r] >= h->n) return fail(WT_E_ARG, "zone must be below the ensemble's zone count");
    if (int rc = stop_program(h, WT_PROG_SCORE)) return rc;   // set replaces any program (and its capacities)
    h->scr.curve_cap = curve_capacity; h->scr.bins = curve_capacity > 0 ? bins : 0;
    for (int k = 0; k < wtsc::SLOTS; ++k) {
        h->scr.fan_lo[k] = bins > 0 ? fan_lo[k] : 0.0; h->scr.fan_hi[k] = bins > 0 ? fan_hi[k] : 0.0;
        h->scr.fan_scale[k] = bins > 0 ? (double)bins / (fan_hi[k] - fan_lo[k]) : 0.0;
    }
    return load_program(h, WT_PROG_SCORE, params);
}

int wt_ensemble_score_get(wt_ensemble *h, double *slot_state, double *t_prev)
{
    if (!h) return fail(WT_E_ARG, "NULL handle");
    return get_program(h, WT_PROG_SCORE, {{slot_state, h->scr.st, wtsc::ST_DOUBLES, wtsc::SLOTS, wtsc::NSS}, {t_prev, h->scr.tp, 1, 1, 1}});
}

int wt_ensemble_score_curve(wt_ensemble *h, int32_t *counts, int32_t *fan, int *n_steps)
{
    if (int rc = program_ready(h, WT_PROG_SCORE)) return rc;
    const size_t cells = (size_t)h->scr.curve_cap * wtsc::SLOTS;
    if (n_steps) *n_steps = (int)(h->scr_steps < h->scr.curve_cap ? h->scr_steps : h->scr.curve_cap);
    return download(h, {{h->scr.counts ? counts : nullptr, h->scr.counts, sizeof(int32_t) * 3 * cells},
                        {h->scr.fan ? fan : nullptr, h->scr.fan, sizeof(int32_t) * (size_t)(h->scr.bins + 2) * cells}});
}

int wt_ensemble_score_fan_range(wt_ensemble *h, double *fan_lo, double *fan_hi)
{
    if (int rc = program_ready(h, WT_PROG_SCORE)) return rc;
    for (int k = 0; k < wtsc::SLOTS; ++k) {
        if (fan_lo) fan_lo[k] = h->scr.fan_lo[k];
        if (fan_hi) fan_hi[k] = h->scr.fan_hi[k];
    }
    return WT_OK;
}

int wt_ensemble_score_reset(wt_ensemble *h) { return reset_program(h, WT_PROG_SCORE); }
int wt_ensemble_score_clear(wt_ensemble *h) { return stop_program(h, WT_PROG_SCORE); }

int wt_ensemble_detect_set(wt_ensemble *h, const double *params, const double *labels)
{
    if (int rc = check_program_set(h, WT_PROG_DETECT, params)) return rc;
    if (int rc = wt_program_check(WT_PROG_DETECT, params, h->N)) return rc;
    if (!labels) return fail(WT_E_ARG, "NULL argument");
    const int64_t N = h->N;
    for (int64_t r = 0; r < N; ++r) {
        const double t0 = labels[wtk::KR_LABEL_START * N + r], t1 = labels[wtk::KR_LABEL_END * N + r];
        if (std::isnan(t0) || std::isnan(t1)) return fail(WT_E_ARG, "label_start and label_end must not be NaN");
        if (!(t1 >= t0)) return fail(WT_E_ARG, "label_end must be >= label_start");
    }
    // the labels go up first (load_program finds the arrays there and synchronises before `lab` is freed)
    std::vector<double> lab((size_t)N * wtk::NKR);
    blocks_to_records(labels, 1, wtk::NKR, N, lab.data(), wtk::NKR);
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipStreamSynchronize(h->stream));   // queued launches may still read the old labels
    if (int rc = allocate(detect_arrays(h))) return rc;
    if (int rc = upload(h, (double *)h->det.lab, lab)) { release(detect_arrays(h)); return rc; }
    return load_program(h, WT_PROG_DETECT, params);
}

int wt_ensemble_detect_get(wt_ensemble *h, double *slot_state, double *t_prev)
{
    if (!h) return fail(WT_E_ARG, "NULL handle");
    return get_program(h, WT_PROG_DETECT, {{slot_state, h->det.st, wtk::ST_DOUBLES, wtk::SLOTS, wtk::NKS}, {t_prev, h->det.tp, 1, 1, 1}});
}

int wt_ensemble_detect_labels(wt_ensemble *h, double *labels)
{
    if (!h || !labels) return fail(WT_E_ARG, "NULL argument");
    return get_program(h, WT_PROG_DETECT, {{labels, h->det.lab, wtk::NKR, 1, wtk::NKR}});
}

int wt_ensemble_detect_reset(wt_ensemble *h) { return reset_program(h, WT_PROG_DETECT); }
int wt_ensemble_detect_clear(wt_ensemble *h) { return stop_program(h, WT_PROG_DETECT); }

int wt_ensemble_trend_set(wt_ensemble *h, const double *params, int64_t capacity, int wrap)
{
    if (int rc = check_program_set(h, WT_PROG_TREND, params)) return rc;
    if (int rc = wt_program_check(WT_PROG_TREND, params, h->N)) return rc;
    if (capacity < 1) return fail(WT_E_ARG, "capacity must be >= 1");
    int64_t bytes = 0;
    if (__builtin_mul_overflow(capacity, (int64_t)(wtt::SLOTS * sizeof(double2)), &bytes) || __builtin_mul_overflow(bytes, h->N, &bytes))
        return fail(WT_E_ARG, "store size overflows int64");
    if (int rc = stop_program(h, WT_PROG_TREND)) return rc;   // set replaces any program (and its capacity)
    h->trd.cap = capacity; h->trd.wrap = wrap ? 1 : 0;
    return load_program(h, WT_PROG_TREND, params);
}

int wt_ensemble_trend_get(wt_ensemble *h, double *slot_state)
{
    if (!h) return fail(WT_E_ARG, "NULL handle");
    return get_program(h, WT_PROG_TREND, {{slot_state, h->trd.st, wtt::ST_DOUBLES, wtt::SLOTS, wtt::NTS}});
}

int wt_ensemble_trend_data(wt_ensemble *h, double *time, double *value)
{
    if (int rc = program_ready(h, WT_PROG_TREND)) return rc;
    const int64_t N = h->N, cap = h->trd.cap;
    std::vector<double> st((size_t)N * wtt::ST_DOUBLES);
    std::vector<double2> store((size_t)N * wtt::SLOTS * (size_t)cap);
    if (int rc = download(h, {{st.data(), h->trd.st, sizeof(double) * st.size()}, {store.data(), h->trd.store, sizeof(double2) * store.size()}}))
        return rc;
    for (int64_t r = 0; r < N; ++r)
        for (int s = 0; s < wtt::SLOTS; ++s) {
            const double n_rec = st[(size_t)((r * wtt::SLOTS + s) * wtt::NTS + wtt::TS_N_RECORDED)];
            const int64_t held = n_rec < (double)cap ? (int64_t)n_rec : cap;
            const int64_t first = n_rec > (double)cap ? (int64_t)std::fmod(n_rec, (double)cap) : 0;   // the oldest sample of a wrapped ring
            const double2 *ring = store.data() + (size_t)((r * wtt::SLOTS + s) * cap);
            for (int64_t k = 0; k < cap; ++k) {
                const double2 v = k < held ? ring[(first + k) % cap] : make_double2(NAN, NAN);
                const size_t o = (size_t)(((int64_t)s * cap + k) * N + r);
                if (time) time[o] = v.x;
                if (value) value[o] = v.y;
            }
        }
    return WT_OK;
}

int wt_ensemble_trend_reset(wt_ensemble *h) { return reset_program(h, WT_PROG_TREND); }
int wt_ensemble_trend_clear(wt_ensemble *h) { return stop_program(h, WT_PROG_TREND); }

int wt_ensemble_get_boundary(wt_ensemble *h, double *bc)
{
    if (!h || !bc) return fail(WT_E_ARG, "NULL argument");
    if (!h->have_bc) return fail(WT_E_STATE, "set_boundary must precede get_boundary");
    HIP_TRY(hipSetDevice(h->device));
    return download(h, {{bc, h->bc, sizeof(double) * WT_NB * (size_t)h->N}});
}

int wt_ensemble_info(wt_ensemble *h, int what, int64_t *value)
{
    if (!h || !value) return fail(WT_E_ARG, "NULL argument");
    // the program codes: WT_INFO_PROGRAM + p up to the trend program, then the two that came after WT_INFO_TRAIN was taken
    const int program = what == WT_INFO_SERVICE ? WT_PROG_SERVICE : what == WT_INFO_TUNE ? WT_PROG_TUNE
                      : what >= WT_INFO_PROGRAM && what < WT_INFO_TRAIN ? what - WT_INFO_PROGRAM : -1;
    if (program >= 0) {
        *value = *k_programs[program].arrays(h).on != 0;
        return WT_OK;
    }
    switch (what) {
    case WT_INFO_PLANT_IO: *value = h->sens.plc_on != 0; break;
    case WT_INFO_TRAIN: *value = h->trn.on != 0; break;
    case WT_INFO_PIPE: *value = h->trn.pipe.on != 0; break;
    case WT_INFO_WIRE: *value = h->wir.on != 0; break;
    case WT_INFO_SENSOR_HISTORY: *value = h->sens.hist_cap; break;
    case WT_INFO_DISTURB_HISTORY: *value = h->dst.hist_cap; break;
    case WT_INFO_SCORE_CURVE: *value = h->scr.curve_cap; break;
    case WT_INFO_SCORE_BINS: *value = h->scr.bins; break;
    case WT_INFO_TREND_CAPACITY: *value = h->trd.cap; break;
    case WT_INFO_TRAIN_LENGTH: *value = h->trn.length; break;
    case WT_INFO_WAVE_DIAG: *value = h->wave_diag != nullptr; break;
    case WT_INFO_BOUNDARY_UPLOADS: *value = h->bc_uploads; break;
    case WT_INFO_MARK: *value = h->mark != nullptr; break;
    case WT_INFO_JUNCTION: *value = h->trn.jct.on != 0; break;
    case WT_INFO_INSTALL: *value = h->ins.on != 0; break;
    case WT_INFO_MPC: *value = h->mpc.on != 0; break;
    case WT_INFO_RESPOND: *value = h->rsp.on != 0; break;
    case WT_INFO_LINK: *value = h->lnk.on != 0; break;
    default: return fail(WT_E_ARG, "unknown info code");
    }
    return WT_OK;
}

int wt_ensemble_program_params(wt_ensemble *h, int program, double *params)
{
    if (!h || !params) return fail(WT_E_ARG, "NULL argument");
    if (program < 0 || program >= N_PROGRAMS) return fail(WT_E_ARG, "unknown program");
    const Program &p = k_programs[program];
    const double *rec = (const double *)*p.arrays(h).arrays[0].first;   // the parameter records: the group's first array
    return get_program(h, program, {{params, rec, p.slots * p.fields, p.slots, p.fields}});
}

int wt_ensemble_diagnostics(wt_ensemble *h, double *out)
{
    if (!h || !out) return fail(WT_E_ARG, "NULL argument");
    if (!h->have_state) return fail(WT_E_STATE, "set_state must precede diagnostics");
    HIP_TRY(hipSetDevice(h->device));
    const size_t bytes = sizeof(double) * wtd::N_DIAG * (size_t)h->N;
    if (!h->diag_out) HIP_TRY(hipMalloc((void **)&h->diag_out, bytes));
    wtd::DiagArgs a;
    a.N = h->N; a.n = h->n; a.par = h->par; a.pH = h->pH; a.Cl = h->Cl; a.T = h->T; a.H = h->dH; a.out = h->diag_out;
    hipLaunchKernelGGL(wtd::diagnostics_kernel, dim3((unsigned)((h->N + 63) / 64)), dim3(64), 0, h->stream, a);
    HIP_TRY(hipGetLastError());
    return download(h, {{out, h->diag_out, bytes}});
}

int wt_ensemble_set_placement(wt_ensemble *h, int mode)
{
    if (!h) return fail(WT_E_ARG, "NULL handle");
    if (mode != WT_PLACE_IDENTITY && mode != WT_PLACE_ADAPTIVE) return fail(WT_E_ARG, "placement mode must be WT_PLACE_IDENTITY or WT_PLACE_ADAPTIVE");
    HIP_TRY(hipSetDevice(h->device));
    if (mode == WT_PLACE_IDENTITY)
        hipLaunchKernelGGL(wtpl::iota_kernel, dim3((unsigned)((h->N + 255) / 256)), dim3(256), 0, h->stream, h->perm, h->N);
    HIP_TRY(hipMemsetAsync(h->cost, 0, sizeof(int32_t) * (size_t)h->N, h->stream));
    HIP_TRY(hipGetLastError());
    h->placement = mode;
    h->cost_steps = 0;
    return WT_OK;
}

int wt_ensemble_get_placement(wt_ensemble *h, int *mode, int32_t *perm)
{
    if (!h) return fail(WT_E_ARG, "NULL handle");
    if (mode) *mode = h->placement;
    if (!perm) return WT_OK;
    HIP_TRY(hipSetDevice(h->device));
    return download(h, {{perm, h->perm, sizeof(int32_t) * (size_t)h->N}});
}

int wt_ensemble_placement_info(wt_ensemble *h, int64_t *redeals, int64_t *history_steps)
{
    if (!h) return fail(WT_E_ARG, "NULL handle");
    if (redeals) *redeals = h->redeals;
    if (history_steps) *history_steps = h->cost_steps;
    return WT_OK;
}

int wt_ensemble_set_step_limit(wt_ensemble *h, int max_attempts)
{
    if (!h) return fail(WT_E_ARG, "NULL handle");
    if (max_attempts < 0) return fail(WT_E_ARG, "max_attempts must be >= 0 (0 = unlimited)");
    h->step_limit = max_attempts;
    return WT_OK;
}

int wt_ensemble_set_sync(wt_ensemble *h, int sync_outer)
{
    if (!h) return fail(WT_E_ARG, "NULL handle");
    (void)sync_outer;   // the reactors of a wavefront always start an outer step together (see include/wtphys.h)
    return WT_OK;
}

int wt_ensemble_set_schedule(wt_ensemble *h, int n_streams, int chunk_steps)
{
    if (!h) return fail(WT_E_ARG, "NULL handle");
    if (n_streams < 0 || n_streams > WT_MAX_STREAMS) return fail(WT_E_ARG, "n_streams out of range");
    if (chunk_steps < 0) return fail(WT_E_ARG, "chunk_steps must be >= 0 (0 = one scan / launch per call)");
    h->sched_mode = n_streams > 0 ? WT_SCHED_STREAMS : WT_SCHED_QUEUE;
    h->n_sub = n_streams > 0 ? n_streams : default_streams(h->N, h->R);
    h->chunk_steps = chunk_steps;
    return WT_OK;
}

int wt_ensemble_get_schedule(wt_ensemble *h, int *mode, int *n_streams, int *chunk_steps, int *workers)
{
    if (!h) return fail(WT_E_ARG, "NULL handle");
    if (mode) *mode = h->sched_mode;
    if (n_streams) *n_streams = h->sched_mode == WT_SCHED_STREAMS ? h->n_sub : 0;
    if (chunk_steps) *chunk_steps = h->chunk_steps;
    if (workers) *workers = h->sched_mode == WT_SCHED_QUEUE ? h->q_workers : 0;
    return WT_OK;
}

int wt_ensemble_item_steps(wt_ensemble *h, int n_steps)
{
    if (!h || n_steps <= 0) return 0;
    if (h->sched_mode == WT_SCHED_QUEUE) return (h->n_groups <= h->q_workers && h->knob_tickets <= 0) ? n_steps : queue_item_steps(h, n_steps);
    const int chunk = h->chunk_steps > 0 ? h->chunk_steps : n_steps;
    return chunk < n_steps ? chunk : n_steps;
}

int wt_ensemble_queue_error(wt_ensemble *h, int *error)
{
    if (!h || !error) return fail(WT_E_ARG, "NULL argument");
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipStreamSynchronize(h->stream));
    *error = (h->err_host[0] ? 1 : 0) | (h->err_host[1] ? 2 : 0);      // bit 0: hand-off timed out, bit 1: a group was left behind; sticky until the handle is destroyed
    return WT_OK;
}

int wt_ensemble_item_trace(wt_ensemble *h, int64_t *out, int capacity, int *n_items)
{
    if (!h || !n_items) return fail(WT_E_ARG, "NULL argument");
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipStreamSynchronize(h->stream));
    if (!h->trace) {     // first call switches tracing on
        if (capacity <= 0) return fail(WT_E_ARG, "capacity must be positive");
        HIP_TRY(hipMalloc((void **)&h->trace, sizeof(int64_t) * 5 * (size_t)capacity));
        h->trace_cap = capacity; *n_items = 0;
        return WT_OK;
    }
    int32_t w[wt::Q_WORDS];
    HIP_TRY(hipMemcpy(w, h->q_ctrl, sizeof w, hipMemcpyDeviceToHost));
    const int n = w[wt::Q_TRACE] < h->trace_cap ? w[wt::Q_TRACE] : h->trace_cap;
    *n_items = n;
    if (out && n > 0) {
        if (capacity < n) return fail(WT_E_ARG, "trace buffer too small");
        HIP_TRY(hipMemcpy(out, h->trace, sizeof(int64_t) * 5 * (size_t)n, hipMemcpyDeviceToHost));
    }
    return WT_OK;
}

int wt_ensemble_get_bad_temperature(wt_ensemble *h, double *value)
{
    if (!h || !value) return fail(WT_E_ARG, "NULL argument");
    HIP_TRY(hipSetDevice(h->device));
    return download(h, {{value, h->bad_T, sizeof(double) * h->N}});
}

int wt_ensemble_synchronize(wt_ensemble *h)
{
    if (!h) return fail(WT_E_ARG, "NULL handle");
    HIP_TRY(hipSetDevice(h->device));
    return sync_checked(h);
}

// Small ensembles: pack everything a snapshot can ask for into one device image, one copy into pinned memory, one
// synchronisation, then scatter into the caller's arrays on the host.  (N = 1: 9 pageable copies of a few dozen
// bytes each were most of the drop-in's per-step latency.)
static int packed_snapshot(wt_ensemble *h, double *pH, double *Cl, double *T, double *time, double *flow,
                           double *H, double *rho, double *kdecay, uint32_t *flags)
{
    const int64_t cnt = h->N * h->n;
    wt::SnapshotArgs a{cnt, h->N, h->pH, h->Cl, h->T, h->dH, h->dRho, h->dK, h->time, h->flow, h->status, h->q_sticky, (double *)h->snap_dev};
    hipLaunchKernelGGL(wt::snapshot_pack_kernel, dim3((unsigned)((cnt + 255) / 256)), dim3(256), 0, h->stream, a);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(h->snap_host, h->snap_dev, h->snap_bytes, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    const double *img = (const double *)h->snap_host;
    const size_t b = sizeof(double) * (size_t)cnt, bn = sizeof(double) * (size_t)h->N;
    double *zone[6] = {pH, Cl, T, H, rho, kdecay};
    for (int i = 0; i < 6; ++i) if (zone[i]) memcpy(zone[i], img + (size_t)i * cnt, b);
    const double *tail = img + 6 * (size_t)cnt;
    if (time) memcpy(time, tail, bn);
    if (flow) memcpy(flow, tail + h->N, bn);
    const uint32_t *w = (const uint32_t *)(tail + 2 * h->N);
    if (flags) memcpy(flags, w, sizeof(uint32_t) * (size_t)h->N);
    if (w[h->N] != 0) return fail(WT_E_HIP, k_incomplete);
    return WT_OK;
}

int wt_ensemble_get_state(wt_ensemble *h, double *pH, double *Cl, double *T, double *time, double *flow)
{
    if (!h) return fail(WT_E_ARG, "NULL handle");
    HIP_TRY(hipSetDevice(h->device));
    if (h->snap_host) return packed_snapshot(h, pH, Cl, T, time, flow, nullptr, nullptr, nullptr, nullptr);
    const size_t b = sizeof(double) * (size_t)h->N * h->n, bn = sizeof(double) * h->N;
    return download(h, {{pH, h->pH, b}, {Cl, h->Cl, b}, {T, h->T, b}, {time, h->time, bn}, {flow, h->flow, bn}});
}

int wt_ensemble_get_snapshot(wt_ensemble *h, double *pH, double *Cl, double *T, double *time, double *flow,
                             double *H, double *rho, double *kdecay, uint32_t *flags)
{
    if (!h) return fail(WT_E_ARG, "NULL handle");
    HIP_TRY(hipSetDevice(h->device));
    if (h->snap_host) return packed_snapshot(h, pH, Cl, T, time, flow, H, rho, kdecay, flags);
    const size_t b = sizeof(double) * (size_t)h->N * h->n, bn = sizeof(double) * h->N;
    return download(h, {{pH, h->pH, b}, {Cl, h->Cl, b}, {T, h->T, b}, {time, h->time, bn}, {flow, h->flow, bn},
                        {H, h->dH, b}, {rho, h->dRho, b}, {kdecay, h->dK, b}, {flags, h->status, sizeof(uint32_t) * h->N}});
}

int wt_ensemble_get_derived(wt_ensemble *h, double *H, double *rho, double *kdecay)
{
    if (!h) return fail(WT_E_ARG, "NULL handle");
    HIP_TRY(hipSetDevice(h->device));
    const size_t b = sizeof(double) * (size_t)h->N * h->n;
    return download(h, {{H, h->dH, b}, {rho, h->dRho, b}, {kdecay, h->dK, b}});
}

int wt_ensemble_get_status(wt_ensemble *h, uint32_t *flags)
{
    if (!h || !flags) return fail(WT_E_ARG, "NULL argument");
    HIP_TRY(hipSetDevice(h->device));
    return download(h, {{flags, h->status, sizeof(uint32_t) * h->N}});
}

int wt_ensemble_clear_status(wt_ensemble *h)
{
    if (!h) return fail(WT_E_ARG, "NULL handle");
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipMemsetAsync(h->status, 0, sizeof(uint32_t) * h->N, h->stream));
    return WT_OK;
}

int wt_ensemble_get_stats(wt_ensemble *h, wt_solver_stats *stats)
{
    if (!h || !stats) return fail(WT_E_ARG, "NULL argument");
    HIP_TRY(hipSetDevice(h->device));
    return download(h, {{stats, h->stats, sizeof(int32_t) * 5 * h->N}});
}

int wt_ensemble_rhs(wt_ensemble *h, const double *pH, const double *Cl, const double *T,
                    double *dpH, double *dCl, double *dT, uint32_t *flags)
{
    if (!h || !pH || !Cl || !T || !dpH || !dCl || !dT || !flags) return fail(WT_E_ARG, "NULL argument");
    if (!h->have_bc) return fail(WT_E_STATE, "set_boundary must precede rhs");
    HIP_TRY(hipSetDevice(h->device));
    const size_t cnt = (size_t)h->N * h->n, b = sizeof(double) * cnt;
    double *buf = nullptr; uint32_t *fl = nullptr;
    HIP_TRY(hipMalloc((void **)&buf, 6 * b));
    if (hipMalloc((void **)&fl, sizeof(uint32_t) * h->N) != hipSuccess) { (void)hipFree(buf); return fail(WT_E_HIP, "hipMalloc failed"); }
    hipError_t e = hipMemcpyAsync(buf, pH, b, hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(buf + cnt, Cl, b, hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(buf + 2 * cnt, T, b, hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess) {
        wt::RhsArgs a;
        a.N = h->N; a.n = h->n; a.R = h->R; a.par = h->par; a.bc = h->bc;
        a.pH = buf; a.Cl = buf + cnt; a.T = buf + 2 * cnt;
        a.dpH = buf + 3 * cnt; a.dCl = buf + 4 * cnt; a.dT = buf + 5 * cnt; a.flags = fl;
        const unsigned grid = (unsigned)((h->N + h->R - 1) / h->R);
        if (row_mode(h->n)) hipLaunchKernelGGL(wt::rhs_kernel<true>, dim3(grid), dim3(64), 0, h->stream, a);
        else hipLaunchKernelGGL(wt::rhs_kernel<false>, dim3(grid), dim3(64), 0, h->stream, a);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(dpH, buf + 3 * cnt, b, hipMemcpyDeviceToHost, h->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(dCl, buf + 4 * cnt, b, hipMemcpyDeviceToHost, h->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(dT, buf + 5 * cnt, b, hipMemcpyDeviceToHost, h->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(flags, fl, sizeof(uint32_t) * h->N, hipMemcpyDeviceToHost, h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    (void)hipFree(buf); (void)hipFree(fl);
    if (e != hipSuccess) return fail(WT_E_HIP, std::string("rhs: ") + hipGetErrorString(e));
    return WT_OK;
}

int wt_ensemble_export_state_device(wt_ensemble *h, void *dst_device)
{
    if (!h || !dst_device) return fail(WT_E_ARG, "NULL argument");
    HIP_TRY(hipSetDevice(h->device));
    const size_t cnt = (size_t)h->N * h->n, b = sizeof(double) * cnt;
    double *d = (double *)dst_device;
    HIP_TRY(hipMemcpyAsync(d, h->pH, b, hipMemcpyDeviceToDevice, h->stream));
    HIP_TRY(hipMemcpyAsync(d + cnt, h->Cl, b, hipMemcpyDeviceToDevice, h->stream));
    HIP_TRY(hipMemcpyAsync(d + 2 * cnt, h->T, b, hipMemcpyDeviceToDevice, h->stream));
    return WT_OK;
}

int wt_ensemble_timer_start(wt_ensemble *h)
{
    if (!h) return fail(WT_E_ARG, "NULL handle");
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipEventRecord(h->ev0, h->stream));
    return WT_OK;
}

int wt_ensemble_timer_stop(wt_ensemble *h, float *elapsed_ms)
{
    if (!h || !elapsed_ms) return fail(WT_E_ARG, "NULL argument");
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipEventRecord(h->ev1, h->stream));
    HIP_TRY(hipEventSynchronize(h->ev1));
    HIP_TRY(hipEventElapsedTime(elapsed_ms, h->ev0, h->ev1));
    return WT_OK;
}

int wt_ensemble_checkpoint_size(wt_ensemble *h, int64_t *bytes)
{
    if (!h || !bytes) return fail(WT_E_ARG, "NULL argument");
    *bytes = checkpoint_bytes(h);
    return WT_OK;
}

int wt_ensemble_checkpoint_save(wt_ensemble *h, void *blob, int64_t bytes)
{
    if (!h || !blob) return fail(WT_E_ARG, "NULL argument");
    const int64_t total = checkpoint_bytes(h);
    if (bytes < total) return fail(WT_E_ARG, "checkpoint_save: the buffer is smaller than wt_ensemble_checkpoint_size");
    HIP_TRY(hipSetDevice(h->device));
    if (int rc = sync_checked(h)) return rc;        // an incomplete state is not saved, as it is not downloaded
    unsigned char *b = (unsigned char *)blob;
    std::memset(b, 0, (size_t)total);               // the padding is zero: two saves of one state give the same bytes
    size_t at = WT_CKP_HEADER_BYTES;
    const auto word = [&](uint32_t w) { std::memcpy(b + at, &w, 4); at += 4; };
    std::vector<Copy> copies;
    for (const Part &p : k_parts) {
        const PartView v = view(p, h);
        word(tag_word(p.tag)); word((uint32_t)v.scalars.size());
        for (const Scalar &s : v.scalars) { const int64_t x = scalar_get(s); std::memcpy(b + at, &x, 8); at += 8; }
        word((uint32_t)v.payload.size()); word(0);
        for (const auto &a : v.payload) {
            const int64_t len = (int64_t)a.second;
            std::memcpy(b + at, &len, 8); at += 8;
            copies.push_back({b + at, *a.first, a.second});
            at += pad8(a.second);
        }
    }
    if (int rc = download(h, copies)) return rc;
    wt_checkpoint_header hd;
    std::memset(&hd, 0, sizeof hd);
    std::memcpy(hd.magic, WT_CKP_MAGIC, 4);
    hd.format = WT_CKP_FORMAT; hd.abi = WT_ABI_VERSION; hd.n_zones = (uint32_t)h->n; hd.n_reactors = h->N; hd.bytes = total;
    hd.layout = layout_fingerprint(); hd.n_parts = N_PARTS;
    hd.checksum = wtck::fnv1a(b + WT_CKP_HEADER_BYTES, (size_t)total - WT_CKP_HEADER_BYTES);
    std::memcpy(b, &hd, sizeof hd);
    return WT_OK;
}

int wt_checkpoint_check(const void *blob, int64_t bytes, int64_t *n_reactors, int *n_zones)
{
    return parse_blob(blob, bytes, n_reactors, n_zones, nullptr);
}

int wt_ensemble_checkpoint_load(wt_ensemble *h, const void *blob, int64_t bytes)
{
    if (!h) return fail(WT_E_ARG, "NULL handle");
    Source src;
    int64_t N = 0; int n = 0;
    if (int rc = parse_blob(blob, bytes, &N, &n, &src, h)) return rc;
    if (!same_constants(h, src.arrays[PART_CORE][0].first, src.arrays[PART_CORE][0].second))
        return fail(WT_E_ARG, "checkpoint_load: the reactor constants differ from the handle's");
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipStreamSynchronize(h->stream));
    instrumentation_off(h);
    if (int rc = restore(h, src)) return rc;
    HIP_TRY(hipStreamSynchronize(h->stream));       // the caller's blob is free on return
    return WT_OK;
}

int wt_ensemble_copy(wt_ensemble *dst, wt_ensemble *src)
{
    if (!dst || !src) return fail(WT_E_ARG, "NULL handle");
    if (dst == src) return fail(WT_E_ARG, "copy: dst and src are the same handle");
    if (dst->N != src->N || dst->n != src->n) return fail(WT_E_ARG, "copy: the handles differ in n_reactors or n_zones");
    if (dst->device != src->device) return fail(WT_E_ARG, "copy: the handles are on different devices");
    if (!same_constants(dst, src->par_sent.data(), sizeof(double) * src->par_sent.size()))
        return fail(WT_E_ARG, "copy: the reactor constants differ");
    HIP_TRY(hipSetDevice(src->device));
    if (int rc = sync_checked(src)) return rc;
    HIP_TRY(hipStreamSynchronize(dst->stream));
    instrumentation_off(dst);
    if (int rc = restore(dst, source_of(src))) return rc;
    HIP_TRY(hipStreamSynchronize(dst->stream));     // src may go on at once
    return WT_OK;
}

int wt_ensemble_mark(wt_ensemble *h)
{
    if (!h) return fail(WT_E_ARG, "NULL handle");
    HIP_TRY(hipSetDevice(h->device));
    if (int rc = sync_checked(h)) return rc;
    Source live = source_of(h);
    size_t total = 0;
    for (const auto &part : live.arrays)
        for (const auto &a : part) total += (a.second + 255) & ~(size_t)255;
    void *buf = nullptr;
    if (total) {
        const hipError_t e = hipMalloc(&buf, total);
        if (e != hipSuccess) return fail(WT_E_HIP, std::string("mark: ") + hipGetErrorString(e));
    }
    std::vector<Copy> copies;
    size_t at = 0;
    for (auto &part : live.arrays)
        for (auto &a : part) {
            void *to = (char *)buf + at;
            copies.push_back({to, a.first, a.second});
            a.first = to;
            at += (a.second + 255) & ~(size_t)255;
        }
    if (int rc = device_copies(copies, h->stream, h->knob_memcpy != 0)) { (void)hipStreamSynchronize(h->stream); (void)hipFree(buf); return rc; }
    drop_mark(h);                                   // (the stream was idle: nothing reads the old mark)
    h->mark = new wt_mark();
    h->mark->buf = buf;
    h->mark->src = std::move(live);
    return WT_OK;
}

int wt_ensemble_rewind(wt_ensemble *h)
{
    if (!h) return fail(WT_E_ARG, "NULL handle");
    if (!h->mark) return fail(WT_E_STATE, "rewind: no mark is set (wt_ensemble_mark)");
    return restore(h, h->mark->src);
}

int wt_ensemble_unmark(wt_ensemble *h)
{
    if (!h) return fail(WT_E_ARG, "NULL handle");
    if (!h->mark) return WT_OK;
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipStreamSynchronize(h->stream));       // a queued rewind may still read it
    drop_mark(h);
    return WT_OK;
}

int wt_selftest_copy_table(int device, const int64_t *bytes, int count, int *mismatches)
{
    if (!mismatches || count < 0 || (count > 0 && !bytes)) return fail(WT_E_ARG, "bad argument");
    *mismatches = 0;
    if (count == 0) return WT_OK;
    constexpr size_t GUARD = 64;
    std::vector<size_t> off((size_t)count + 1, 0);
    for (int i = 0; i < count; ++i) {
        if (bytes[i] < 0) return fail(WT_E_ARG, "bad argument");
        off[(size_t)i + 1] = off[(size_t)i] + (((size_t)bytes[i] + GUARD + 255) & ~(size_t)255);
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return fail(WT_E_NOGPU, "no HIP device available: libwtphys has no CPU path");
    if (device < 0 || device >= ndev) return fail(WT_E_ARG, "bad device index");
    HIP_TRY(hipSetDevice(device));
    const size_t total = off[(size_t)count];
    std::vector<unsigned char> from(total), to(total, 0xA5), got(total);
    for (size_t i = 0; i < total; ++i) from[i] = (unsigned char)((i * 2654435761u) >> 13);
    unsigned char *d_from = nullptr, *d_to = nullptr;
    HIP_TRY(hipMalloc((void **)&d_from, total));
    if (hipMalloc((void **)&d_to, total) != hipSuccess) { (void)hipFree(d_from); return fail(WT_E_HIP, "hipMalloc failed"); }
    hipError_t e = hipMemcpy(d_from, from.data(), total, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d_to, to.data(), total, hipMemcpyHostToDevice);
    int rc = WT_OK;
    if (e == hipSuccess) {
        std::vector<Copy> copies;
        for (int i = 0; i < count; ++i) copies.push_back({d_to + off[(size_t)i], d_from + off[(size_t)i], (size_t)bytes[i]});
        rc = device_copies(copies, nullptr, false);
        if (rc == WT_OK) e = hipDeviceSynchronize();
    }
    if (rc == WT_OK && e == hipSuccess) e = hipMemcpy(got.data(), d_to, total, hipMemcpyDeviceToHost);
    (void)hipFree(d_from); (void)hipFree(d_to);
    if (rc != WT_OK) return rc;
    if (e != hipSuccess) return fail(WT_E_HIP, hipGetErrorString(e));
    int bad = 0;
    for (int i = 0; i < count; ++i)
        for (size_t k = off[(size_t)i]; k < off[(size_t)i + 1]; ++k) {
            const bool inside = k - off[(size_t)i] < (size_t)bytes[i];
            if (got[k] != (inside ? from[k] : (unsigned char)0xA5) && bad < 0x7fffffff) ++bad;
        }
    *mismatches = bad;
    return WT_OK;
}

int wt_selftest_shuffles(int device, int n_zones, int *mismatches)
{
    if (!mismatches || n_zones < 2 || n_zones > WT_MAX_ZONES) return fail(WT_E_ARG, "bad argument");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return fail(WT_E_NOGPU, "no HIP device available: libwtphys has no CPU path");
    HIP_TRY(hipSetDevice(device));
    int *d = nullptr;
    HIP_TRY(hipMalloc((void **)&d, 64 * sizeof(int)));
    wt::ShuffleTestArgs a{n_zones, d};
    if (row_mode(n_zones)) hipLaunchKernelGGL(wt::shuffle_selftest_kernel<true>, dim3(1), dim3(64), 0, 0, a);
    else hipLaunchKernelGGL(wt::shuffle_selftest_kernel<false>, dim3(1), dim3(64), 0, 0, a);
    int host[64];
    hipError_t e = hipMemcpy(host, d, sizeof host, hipMemcpyDeviceToHost);
    (void)hipFree(d);
    if (e != hipSuccess) return fail(WT_E_HIP, hipGetErrorString(e));
    int total = 0;
    for (int i = 0; i < 64; ++i) total += host[i];
    *mismatches = total;
    return WT_OK;
}

int wt_wave_diag_slots(void) { return wt::WT_DIAG_SLOTS; }

int wt_ensemble_wave_diag(wt_ensemble *h, int64_t *out, int64_t capacity, int64_t *n_waves)
{
    if (!h || !n_waves) return fail(WT_E_ARG, "NULL argument");
    HIP_TRY(hipSetDevice(h->device));
    const int64_t nw = h->n_groups;
    *n_waves = nw;
    if (!h->wave_diag) {   // first call switches the diagnostics on
        HIP_TRY(hipMalloc((void **)&h->wave_diag, sizeof(int64_t) * wt::WT_DIAG_SLOTS * (size_t)nw));
        HIP_TRY(hipMemsetAsync(h->wave_diag, 0, sizeof(int64_t) * wt::WT_DIAG_SLOTS * (size_t)nw, h->stream));
        HIP_TRY(hipStreamSynchronize(h->stream));
        return WT_OK;
    }
    if (out) {
        if (capacity < nw) return fail(WT_E_ARG, "wave_diag buffer too small");
        HIP_TRY(hipMemcpyAsync(out, h->wave_diag, sizeof(int64_t) * wt::WT_DIAG_SLOTS * (size_t)nw, hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(hipStreamSynchronize(h->stream));
    }
    return WT_OK;
}

int64_t wt_ensemble_size(const wt_ensemble *h) { return h ? h->N : 0; }
int wt_ensemble_zones(const wt_ensemble *h) { return h ? h->n : 0; }

int wt_ph_solve(int device, int64_t n, const double *Kw, const double *Ka1, const double *Ka2,
                const double *CT_mol, const double *alk_mgL, const double *guess,
                double tol, int max_iter, double *pH_out, int32_t *iters, int32_t *rc)
{
    if (n < 0 || !Kw || !Ka1 || !Ka2 || !CT_mol || !alk_mgL || !guess || !pH_out || !iters || !rc)
        return fail(WT_E_ARG, "NULL argument");
    if (n == 0) return WT_OK;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return fail(WT_E_NOGPU, "no HIP device available: libwtphys has no CPU path");
    if (device < 0 || device >= ndev) return fail(WT_E_ARG, "bad device index");
    HIP_TRY(hipSetDevice(device));
    const size_t b = sizeof(double) * (size_t)n;
    double *buf = nullptr; int32_t *ib = nullptr;
    HIP_TRY(hipMalloc((void **)&buf, 7 * b));
    if (hipMalloc((void **)&ib, 2 * sizeof(int32_t) * (size_t)n) != hipSuccess) { (void)hipFree(buf); return fail(WT_E_HIP, "hipMalloc failed"); }
    const double *src[6] = {Kw, Ka1, Ka2, CT_mol, alk_mgL, guess};
    hipError_t e = hipSuccess;
    for (int i = 0; i < 6 && e == hipSuccess; ++i) e = hipMemcpy(buf + (size_t)i * n, src[i], b, hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        wt::PhArgs a;
        a.n = n; a.Kw = buf; a.Ka1 = buf + n; a.Ka2 = buf + 2 * n; a.CT = buf + 3 * n; a.alk = buf + 4 * n;
        a.guess = buf + 5 * n; a.tol = tol; a.max_iter = max_iter; a.pH = buf + 6 * n; a.iters = ib; a.rc = ib + n;
        const unsigned grid = (unsigned)((n + 255) / 256);
        hipLaunchKernelGGL(wt::ph_solve_kernel, dim3(grid), dim3(256), 0, 0, a);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e == hipSuccess) e = hipMemcpy(pH_out, buf + 6 * (size_t)n, b, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(iters, ib, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(rc, ib + n, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost);
    (void)hipFree(buf); (void)hipFree(ib);
    if (e != hipSuccess) return fail(WT_E_HIP, std::string("ph_solve: ") + hipGetErrorString(e));
    return WT_OK;
}

} // extern "C"
