// wt_queue.hpp -- the device-side work queue: a FIFO of wavefront-groups that are ready for their next work item, so
// that one launch advances the whole ensemble by any number of outer steps and no wavefront waits for a launch
// boundary.  The control words are Q_* of wt_args.hpp; the kernels that reset and check the queue are in wt_device.hpp.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "wt_args.hpp"

namespace wt {

// ---- device-side work queue: FIFO of wavefront-groups that are ready for their next item (wave-uniform calls) ----
// Tickets 0 .. n_groups-1 are the groups themselves, last group first (every group starts ready; the slots are dealt in
// order of solver cost, so the expensive groups are the ones that must not start late); ticket n_groups + p is the
// p-th push.
// Q_AVAIL counts published, unclaimed entries, so a claimed ticket is always (about to be) written: the only wait
// is for a pusher that sits between its tail increment and its slot store.
__device__ __forceinline__ int queue_resolve(ArgPtr a, int ticket)
{
    const int n_groups = a->n_groups;
    if (ticket < n_groups) return n_groups - 1 - ticket;
    const unsigned long long want = (unsigned long long)(unsigned)(ticket + 1);
    unsigned long long *slot = a->q_slots + (ticket - n_groups) % a->q_cap;
    for (int spin = 0; spin < (1 << 22); ++spin) {
        const unsigned long long w = __hip_atomic_load(slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if ((w >> 32) == want) return (int)(w & 0xffffffffull);
        __builtin_amdgcn_s_sleep(2);
    }
    __hip_atomic_store(a->q_ctrl + Q_ERROR, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // never seen; the host reports it
    return -1;
}

__device__ __forceinline__ void queue_push(ArgPtr a, int group)
{
    int32_t *ctrl = a->q_ctrl;
    const int p = __hip_atomic_fetch_add(ctrl + Q_TAIL, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const unsigned long long w = ((unsigned long long)(unsigned)(a->n_groups + p + 1) << 32) | (unsigned)group;
    __hip_atomic_store(a->q_slots + p % a->q_cap, w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_fetch_add(ctrl + Q_AVAIL, 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
}

// Next group for this worker, or -1 to retire.  own >= 0: the group just advanced still has steps to go; it goes to
// the back of the queue if another group is waiting (rotation: with more groups than resident wavefronts nobody
// idles) -- unless `hold`: the group is behind the ensemble's average progress (an expensive group: the same worker
// time buys it fewer steps) and keeps its worker until it has caught up, so that all groups finish together instead of
// the expensive ones trailing at the end of the launch.  Otherwise this worker simply carries on with it.  Only an
// exchange hands data to another CU, so only then the wavefront releases what it wrote (and the taker acquires).
// (Tried and dropped: letting groups whose items run long keep their worker, and dealing last launch's slow groups
// first -- a group's cost comes in bursts when a reactor crosses a stratification switch, not as a persistent rate,
// so neither shortens the tail of a short launch; see DESIGN.md.)
__device__ __forceinline__ int queue_next(ArgPtr pa, int own, bool hold, bool &exchanged)
{
    ArgPtr a = fresh(pa);
    const bool lane0 = (threadIdx.x & 63) == 0;
    int ticket = -1;
    if (lane0 && !(own >= 0 && hold)) {
        // Claim one published entry.  A failed claim takes Q_AVAIL below its true value until it is restored, which
        // can make a concurrent claimer fail although an entry has just been published; so whoever fails looks again
        // after restoring: the last of the failed claimers to restore sees the true count.  (One atomic per claim in
        // the common case; a compare-and-swap loop here costs O(workers^2) atomics when a launch starts.)
        int32_t *avail = a->q_ctrl + Q_AVAIL;
        do {
            const int old = __hip_atomic_fetch_add(avail, -1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (old > 0) { ticket = __hip_atomic_fetch_add(a->q_ctrl + Q_HEAD, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); break; }
            __hip_atomic_fetch_add(avail, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        } while (__hip_atomic_load(avail, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > 0);
    }
    ticket = __builtin_amdgcn_readfirstlane(ticket);
    exchanged = ticket >= 0;
    if (ticket < 0) return own;                 // nothing waiting (or holding on): carry on with the own group, or retire
    if (own >= 0) {
        // publish the group's state before anybody can take its next item
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    int next = -1;
    if (lane0) {
        if (own >= 0) queue_push(a, own);
        next = queue_resolve(a, ticket);
    }
    return __builtin_amdgcn_readfirstlane(next);
}

} // namespace wt
