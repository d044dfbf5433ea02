// f3dg_compact.h -- the stream compaction of the mesh routes (f3dg_mesh.hip, f3dg_tsdf.hip, f3dg_mesh_clean.hip): n elements, one thread
// each in workgroups of F3DG_BLOCK, the kept ones written in input order.
//   1. one keep bit per element: a wave's ballot is the 64-bit flag word of its 64 elements, lane 0 stores it;
//   2. the workgroup's count of kept elements, from the wave popcounts through LDS, into a count array;
//   3. one workgroup scans the count array in place (exclusive; scan_array_in_place, f3dg_scan.h). The array is padded to whole
//      F3DG_COMPACT_SCAN_ITEMS and the host clears the padding;
//   4. the output row of a kept element: its workgroup's scanned count, the popcounts of the earlier words of its workgroup, the bits
//      below its own;
//   5. the caller drops the rows past its capacity.
// Integer sums only: every rank is exact and the output is a function of the keep bits alone. (f3dg_mesh.hip stores no flag words
// -- it rebuilds the ballots -- and scans its count arrays, 125 k entries at its own size, with the three-launch scan instead of 3.)
//
// block_ballot and block_flag_and_count hold a barrier, and block_count / block_rank read what lies behind it: EVERY thread of the
// workgroup must reach each call. A thread with nothing to keep passes false.
#pragma once
#include "f3dg_common.h"
#include "f3dg_scan.h"

namespace {

typedef unsigned long long u64;
typedef unsigned int u32;

#define F3DG_COMPACT_SCAN_ITEMS 16      // count entries a thread takes per round of compact_scan_counts: 4,096 workgroups a round

static_assert(F3DG_BLOCK == 256, "compact_rank: a workgroup's flags are four 64-bit words");

// ------------------------------------------------------------------------------------------------ host
size_t f3dg_align256(size_t x) { return (x + 255) & ~(size_t)255; }

struct CompactPlan {
    u32 n_blocks, n_words, n_scan;          // workgroups, 64-bit flag words, count entries (n_blocks rounded up to whole scan items)
    size_t flag_bytes, count_bytes;         // of the flag words and of the count array, each rounded up to 256
};

CompactPlan compact_plan(u32 n)
{
    CompactPlan P;
    P.n_blocks = (n + F3DG_BLOCK - 1) / F3DG_BLOCK;
    P.n_words = (n + 63u) / 64u;
    P.n_scan = (P.n_blocks + F3DG_COMPACT_SCAN_ITEMS - 1) / F3DG_COMPACT_SCAN_ITEMS * F3DG_COMPACT_SCAN_ITEMS;
    P.flag_bytes = f3dg_align256((size_t)P.n_words * 8);
    P.count_bytes = f3dg_align256((size_t)P.n_scan * 4);
    return P;
}

// zeros in counts[n_blocks, n_scan): the scan reads whole items, the workgroups write [0, n_blocks) only
hipError_t compact_clear_padding(hipStream_t s, u32* counts, const CompactPlan& P)
{
    if (P.n_scan == P.n_blocks) return hipSuccess;
    return hipMemsetAsync(counts + P.n_blocks, 0, (size_t)(P.n_scan - P.n_blocks) * 4, s);
}

// ------------------------------------------------------------------------------------------------ device: flags and counts
// the wave's ballot as the flag word of its 64 elements; i is the thread's element
__device__ __forceinline__ void store_flag_word(u64* __restrict__ flags, u64 m, u32 i, u32 n)
{
    if ((threadIdx.x & 63u) == 0u && i < n) flags[i >> 6] = m;
}

// the wave's ballot of `keep`, its popcount into w_cnt[F3DG_BLOCK / 64] (LDS). No barrier: a kernel that counts two kinds of element
// calls this once per kind and puts ONE __syncthreads() behind them; everybody else calls block_ballot.
__device__ __forceinline__ u64 wave_ballot(bool keep, u32* w_cnt)
{
    const u64 m = __ballot(keep);
    if ((threadIdx.x & 63u) == 0u) w_cnt[threadIdx.x >> 6] = (u32)__popcll(m);
    return m;
}

// wave_ballot and the barrier: the popcount of every wave of the workgroup is in w_cnt on return. The threads read w_cnt afterwards
// (block_count, block_rank): the caller puts a barrier before it writes w_cnt again.
__device__ __forceinline__ u64 block_ballot(bool keep, u32* w_cnt)
{
    const u64 m = wave_ballot(keep, w_cnt);
    __syncthreads();
    return m;
}

// kept elements of the workgroup (after block_ballot)
__device__ __forceinline__ u32 block_count(const u32* w_cnt)
{
    u32 n = 0;
#pragma unroll
    for (int w = 0; w < F3DG_BLOCK / 64; w++) n += w_cnt[w];
    return n;
}

// steps 1 and 2 in one: element i of n, flag word and workgroup count stored
__device__ __forceinline__ void block_flag_and_count(bool keep, u32 i, u32 n, u64* __restrict__ flags, u32* __restrict__ counts, u32* w_cnt)
{
    store_flag_word(flags, block_ballot(keep, w_cnt), i, n);
    if (threadIdx.x == 0) counts[blockIdx.x] = block_count(w_cnt);
}

// step 3, by one workgroup; the sum of the counts. wtot[F3DG_BLOCK / 64] is LDS and free again on return.
__device__ __forceinline__ u64 compact_scan_counts(u32* __restrict__ counts, u32 n_scan, u64* wtot)
{
    return scan_array_in_place<F3DG_BLOCK / 64, F3DG_COMPACT_SCAN_ITEMS, u64>(counts, n_scan, 0u, wtot);
}

// ------------------------------------------------------------------------------------------------ device: ranks
// kept threads of the workgroup before this one, from its wave's ballot m and the wave counts (after block_ballot): no flag words needed
__device__ __forceinline__ u32 block_rank(u64 m, const u32* w_cnt)
{
    const u32 lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    u32 r = (u32)__popcll(m & ((1ull << lane) - 1ull));
    for (u32 w = 0; w < wave; w++) r += w_cnt[w];
    return r;
}

__device__ __forceinline__ bool compact_kept(const u64* __restrict__ flags, u32 i) { return (flags[i >> 6] >> (i & 63u)) & 1ull; }

// step 4: kept elements before element i, from the stored flag words and the scanned counts. Any thread may ask for any i < n; the
// words read are those of i's own workgroup.
__device__ __forceinline__ u64 compact_rank(const u64* __restrict__ flags, const u32* __restrict__ counts, u32 i)
{
    const u32 w = i >> 6;
    u64 r = (u64)counts[i / F3DG_BLOCK] + (u64)__popcll(flags[w] & ((1ull << (i & 63u)) - 1ull));
    for (u32 k = w & ~(F3DG_BLOCK / 64 - 1u); k < w; k++) r += (u64)__popcll(flags[k]);
    return r;
}

} // namespace
