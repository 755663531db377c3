"""What a rewind, a clone and a checkpoint through the host cost, against the warm-up a rewind saves.

    python tools/checkpoint_probe.py [N] [n] [steps]        (10 000 x 8, 190 warm-up steps by default)

A plant with sensors, plant I/O, both PI loops and eight trend slots of capacity 512 is warmed up, then marked.  Five
repeats in rotating order, medians and ranges, each between two synchronisations:
  rewind_kernel   wt_ensemble_rewind on the fast path, the copies as one launch of wtck::copy_table_kernel
  rewind_memcpy   the same on a handle created under WT_CKP_MEMCPY=1: one hipMemcpyAsync per array
  clone           ReactorEnsemble.clone(): a new handle, its allocations, the device-to-device copy
  host            checkpoint() + restore() through the host
with the blob size, the device bytes of a mark's payload, the warm-up time, and the bitwise checks that the rewound
handles, the clone and the restored handle all continue alike.  One JSON line."""
import json, os, time
from probe_common import arguments, pi_loops, plant, outputs, rotate, same, timed_step, wt

DT = 10.0
N, n, K, cols, bc = arguments(190)


def warmed(memcpy):
    if memcpy:
        os.environ["WT_CKP_MEMCPY"] = "1"       # read when the handle is created
    ens = plant(cols, bc, n)
    os.environ.pop("WT_CKP_MEMCPY", None)
    chlorine, acid, _ = pi_loops(cols, N)
    ens.enable_control(chlorine, acid)
    ens.set_trends(*[wt.Trend("image_value", k % 7) for k in range(8)], capacity=512)
    _, seconds = timed_step(ens, DT, K)
    ens.mark()
    ens.synchronize()
    return ens, seconds


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return time.perf_counter() - t0, out


def run(variant, rep):
    if variant == "rewind_kernel":
        return timed(lambda: (kernel.rewind(), kernel.synchronize()))
    if variant == "rewind_memcpy":
        return timed(lambda: (memcpy.rewind(), memcpy.synchronize()))
    if variant == "clone":
        seconds, c = timed(lambda: (lambda c: (c.synchronize(), c)[1])(kernel.clone()))
        c.close()
        return seconds, None
    blob = []
    seconds, _ = timed(lambda: (blob.append(kernel.checkpoint()), kernel.restore(blob[0]), kernel.synchronize()))
    return seconds, len(blob[0])


kernel, warm_kernel = warmed(False)
memcpy, warm_memcpy = warmed(True)
run("rewind_kernel", -1), run("rewind_memcpy", -1)          # the first launch of the copy kernel loads its code
times, median, last = rotate(("rewind_kernel", "rewind_memcpy", "clone", "host"), 5, run)

# all four continue alike: the rewound handles, a clone and the handle restored from its own blob
getters = ("sensor_readings", "boundary", "control_state", "trend_state")
clone = kernel.clone()
for ens in (kernel, memcpy, clone):
    ens.step(DT, n_steps=20, download=False)
ref = outputs(kernel, *getters)
kernel.rewind()
kernel.restore(kernel.checkpoint())
kernel.step(DT, n_steps=20, download=False)
print(json.dumps({
    "N": N, "n": n, "warmup_steps": K, "blob_bytes": last["host"][1],
    "warmup_s": [warm_kernel, warm_memcpy],
    "median_s": median, "range_s": {v: [min(t), max(t)] for v, t in times.items()},
    "same_bits": {"memcpy": same(ref, outputs(memcpy, *getters)), "clone": same(ref, outputs(clone, *getters)),
                  "host": same(ref, outputs(kernel, *getters))}}))
