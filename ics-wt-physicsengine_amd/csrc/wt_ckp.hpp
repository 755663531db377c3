// wt_ckp.hpp -- the device side of checkpoint, copy and rewind: one kernel that performs all of a
// checkpoint's device-to-device array copies in one launch, and the hash both the blob's checksum and its layout
// fingerprint use.  The step kernels do not include this header.
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdint>

namespace wtck {

constexpr int MAX_ENTRIES = 128;     // copies per launch: the table travels in the kernel-argument block
constexpr int CHUNK = 16384;         // bytes a workgroup moves per trip of its grid-stride loop
constexpr int THREADS = 256;

// Up to MAX_ENTRIES disjoint copies.  first[e] is the index of entry e's first chunk, first[count] the chunk total;
// an entry of b bytes has ceil(b / CHUNK) chunks, so every entry here has at least one byte (the host skips the rest).
// Bases are 16-byte aligned (hipMalloc gives 256), so every chunk start is.
struct CopyTable {
    int count, chunks;
    const void *src[MAX_ENTRIES];
    void *dst[MAX_ENTRIES];
    int64_t bytes[MAX_ENTRIES];
    int32_t first[MAX_ENTRIES + 1];
};
static_assert(sizeof(CopyTable) <= 4096, "the table must fit the kernel-argument block");

// A workgroup takes chunk indices from a grid-stride loop, finds the chunk's entry by binary search in `first` and
// moves it with 16-byte loads and stores; the last chunk of an entry moves its bytes % 16 remainder singly.
__global__ __launch_bounds__(THREADS) void copy_table_kernel(const CopyTable t)
{
    for (int c = (int)blockIdx.x; c < t.chunks; c += (int)gridDim.x) {
        int lo = 0, hi = t.count;                  // first[lo] <= c < first[hi]
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (t.first[mid] <= c) lo = mid; else hi = mid;
        }
        const int64_t off = (int64_t)(c - t.first[lo]) * CHUNK, left = t.bytes[lo] - off;
        const int n = left < CHUNK ? (int)left : CHUNK;
        const char *s = (const char *)t.src[lo] + off;
        char *d = (char *)t.dst[lo] + off;
        const int vec = n >> 4;
        for (int i = (int)threadIdx.x; i < vec; i += THREADS) ((uint4 *)d)[i] = ((const uint4 *)s)[i];
        const int tail = n & 15;
        if ((int)threadIdx.x < tail) d[vec * 16 + (int)threadIdx.x] = s[vec * 16 + (int)threadIdx.x];
    }
}

// 64-bit FNV-1a, continued from `hash`
constexpr uint64_t FNV_BASIS = 14695981039346656037ull, FNV_PRIME = 1099511628211ull;

inline uint64_t fnv1a(const void *p, size_t bytes, uint64_t hash = FNV_BASIS)
{
    const unsigned char *b = (const unsigned char *)p;
    for (size_t i = 0; i < bytes; ++i) { hash ^= b[i]; hash *= FNV_PRIME; }
    return hash;
}

inline uint64_t fnv1a_u64(uint64_t v, uint64_t hash)
{
    unsigned char b[8];
    for (int i = 0; i < 8; ++i) b[i] = (unsigned char)(v >> (8 * i));
    return fnv1a(b, 8, hash);
}

} // namespace wtck
