// f3dg_scan.h -- the prefix sums of binning (f3dg_binning.hip, f3dg_small.hip): one inclusive scan over the lanes of a wave64, one
// exclusive scan over the threads of a workgroup built on it, one in-place scan of an array by a workgroup built on that, and the
// call's status from the total. Integer sums only: every result is exact, a u32 prefix is the u64 prefix modulo 2^32.
//
// The workgroup helpers hold barriers: EVERY thread of the workgroup must reach each call, with the same trip count. A thread that
// has nothing to add passes 0.
#pragma once
#include "f3dg_common.h"

namespace {

// inclusive sum of x over the lanes 0 .. lane of a wave64 (Hillis-Steele, six steps)
template <typename T>
__device__ __forceinline__ T wave_scan_inclusive(T x, unsigned lane)
{
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const T y = __shfl_up(x, off, 64);
        if (lane >= (unsigned)off) x += y;
    }
    return x;
}

// exclusive sum of x over the threads 0 .. threadIdx.x - 1 of a workgroup of WAVES waves, and the workgroup's total. wtot[WAVES] is
// LDS scratch: every thread reads all of it after the one barrier, so the caller puts a barrier before the next use of wtot.
template <int WAVES, typename T>
__device__ __forceinline__ T block_scan_exclusive(T x, T* wtot, T& total)
{
    const unsigned lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const T incl = wave_scan_inclusive(x, lane);
    if (lane == 63u) wtot[wave] = incl;
    __syncthreads();
    T before = incl - x;
    total = 0;
#pragma unroll
    for (unsigned w = 0; w < (unsigned)WAVES; w++) {
        const T t = wtot[w];
        if (w < wave) before += t;
        total += t;
    }
    return before;
}
template <int WAVES, typename T>
__device__ __forceinline__ T block_scan_exclusive(T x, T* wtot)
{
    T total;
    return block_scan_exclusive<WAVES>(x, wtot, total);
}

// exclusive scan of a[0, n) in place by one workgroup of WAVES waves, starting from `start`; n is a multiple of ITEMS. A thread takes
// ITEMS consecutive entries per round (16-byte loads and stores where ITEMS is a multiple of 4) and holds the carry of the earlier
// rounds itself. The threads' sums are scanned in T, which the caller names, and the entries get the low 32 bits; what the carry
// gained is the sum of the entries, which is returned. With T = unsigned long long that sum is exact -- a single round of block sums
// can exceed 2^32, and the overflow status depends on the exact total --, with T = unsigned it is the sum modulo 2^32.
template <int WAVES, int ITEMS, typename T>
__device__ __forceinline__ T scan_array_in_place(unsigned* __restrict__ a, unsigned n, unsigned start, T* wtot)
{
    static_assert(ITEMS == 1 || ITEMS % 4 == 0, "one entry or whole uint4s per thread");
    T carry = start;
    for (unsigned base = 0; base < n; base += 64u * WAVES * ITEMS) {
        const unsigned i = base + (unsigned)ITEMS * threadIdx.x;
        unsigned v[ITEMS];
        if constexpr (ITEMS == 1) {
            v[0] = i < n ? a[i] : 0u;
        } else {
#pragma unroll
            for (int q = 0; q < ITEMS / 4; q++) {
                const uint4 w = i < n ? reinterpret_cast<const uint4*>(a + i)[q] : make_uint4(0u, 0u, 0u, 0u);
                v[4 * q] = w.x; v[4 * q + 1] = w.y; v[4 * q + 2] = w.z; v[4 * q + 3] = w.w;
            }
        }
        T mine = 0, round;
#pragma unroll
        for (int q = 0; q < ITEMS; q++) mine += v[q];
        unsigned run = (unsigned)(carry + block_scan_exclusive<WAVES>(mine, wtot, round));
        carry += round;
        if (i < n) {
            if constexpr (ITEMS == 1) {
                a[i] = run;
            } else {
#pragma unroll
                for (int q = 0; q < ITEMS / 4; q++) {
                    uint4 o;
                    o.x = run; run += v[4 * q]; o.y = run; run += v[4 * q + 1]; o.z = run; run += v[4 * q + 2]; o.w = run; run += v[4 * q + 3];
                    reinterpret_cast<uint4*>(a + i)[q] = o;
                }
            }
        }
        __syncthreads();          // wtot is written again in the next round
    }
    return carry - start;
}

// the call's status from its instance total: the clamped count (a wrapped 32-bit total must not pass for a small one, later kernels
// index the instance arrays with it) and the overflow flag, written by thread 0 and returned to every thread
__device__ __forceinline__ bool set_status(F3dgHeader* __restrict__ hdr, unsigned long long total)
{
    const bool overflow = total > (unsigned long long)hdr->capacity;
    if (threadIdx.x == 0) {
        hdr->num_rendered = total > 0xFFFFFFFFull ? 0xFFFFFFFFu : (unsigned)total;
        hdr->overflow = overflow ? 1u : 0u;
    }
    return overflow;
}

} // namespace
