// f3dg_binning.hip -- tile binning: block sums, key duplication, stable LSD radix sort, tile ranges.
//
// Replaces, for ALL views of a call at once (reference RAST/cuda_rasterizer/rasterizer_impl.cu):
//   cub::DeviceScan::InclusiveSum      :332      -> sums per 256 depth positions + block_sums_scan_kernel / view_segments_kernel (placing the
//                                                    instances); scan_* kernels (reduce / scan / propagate: the general scan). Every
//                                                    prefix sum here is one of the three of f3dg_scan.h: wave, workgroup, array in place
//   the blocking D2H of num_rendered   :336      -> count stays on the device (workspace header)
//   duplicateWithKeys                  :70-111   -> duplicate_sorted_kernel
//   cub::DeviceRadixSort::SortPairs    :358-363  -> gsort_* (depth, per Gaussian) and radix2_*_var (tile, per instance) passes of 8 bits
//   cudaMemset(ranges) + identifyTileRanges :365, :149-171 -> memset + group_bounds_kernel
//
// The final list is the reference's: per view, ascending (tile, depth bits, Gaussian id) -- what a stable sort of its 64-bit keys
// (tile << 32 | float_bits(depth)) gives. It is built depth-first (see "depth-first binning" below): the Gaussians of every view are
// sorted by depth once, the instances are generated in that order, and ONE stable pass over the tile bits (two above 256 tiles)
// groups them; no instance is ever sorted by depth. Depths are > 0.2 so their IEEE bits order as unsigned ints.
//
// Wave64 notes: the in-block ranking of the scatter uses 64-lane ballots (one per digit bit) to find, for every
// lane, the set of lanes holding the same digit; ranks are popcounts of that 64-bit mask below the lane. Keys
// are consumed in (wave, round, lane) order which IS memory order, so stability needs no extra bookkeeping.
#include "f3dg_common.h"
#include "f3dg_scan.h"

namespace {

typedef unsigned long long u64;
typedef unsigned int u32;
typedef unsigned short u16;
typedef unsigned char u8;

// ------------------------------------------------------------------------------------------------ scan
// Three-kernel scan of n u32 values: per-block sums -> scan of block sums (one workgroup) -> per-block scan.
__global__ void __launch_bounds__(F3DG_BLOCK)
scan_reduce_kernel(const u32* __restrict__ in, u64 n, u32* __restrict__ block_sums)
{
    __shared__ u32 wsum[F3DG_BLOCK / 64];
    const u64 base = (u64)blockIdx.x * F3DG_SCAN_CHUNK;
    u32 s = 0;
#pragma unroll
    for (int i = 0; i < F3DG_SCAN_ITEMS; i++) {
        const u64 k = base + (u64)i * F3DG_BLOCK + threadIdx.x;
        if (k < n) s += in[k];
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) block_sums[blockIdx.x] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
}

// Exclusive scan of the block sums in place, by one workgroup looping over them; also publishes the total (the call's status).
__global__ void __launch_bounds__(1024)
scan_blocksums_kernel(u32* __restrict__ block_sums, u32 nblocks, F3dgHeader* __restrict__ hdr)
{
    __shared__ u64 wtot[16];
    // (64 bits: a batch can hold more than 2^32 instances, V * P * tiles)
    const u64 total = scan_array_in_place<16, 1, u64>(block_sums, nblocks, 0u, wtot);
    if (hdr) set_status(hdr, total);
}

__global__ void __launch_bounds__(F3DG_BLOCK)
scan_apply_kernel(const u32* in, u32* out /* may alias in */, u64 n, const u32* __restrict__ block_sums,
                  int exclusive)
{
    // each thread owns SCAN_ITEMS CONSECUTIVE values (blocked arrangement) so the scan is a plain running sum
    __shared__ u32 wtot[F3DG_BLOCK / 64];
    const u64 base = (u64)blockIdx.x * F3DG_SCAN_CHUNK + (u64)threadIdx.x * F3DG_SCAN_ITEMS;
    u32 v[F3DG_SCAN_ITEMS];
    u32 s = 0;
    if (base + F3DG_SCAN_ITEMS <= n) {           // 64 contiguous bytes per thread: four 16-byte loads
#pragma unroll
        for (int i = 0; i < F3DG_SCAN_ITEMS / 4; i++) {
            const uint4 w = reinterpret_cast<const uint4*>(in + base)[i];
            v[4 * i] = w.x; v[4 * i + 1] = w.y; v[4 * i + 2] = w.z; v[4 * i + 3] = w.w;
        }
    } else {
#pragma unroll
        for (int i = 0; i < F3DG_SCAN_ITEMS; i++) v[i] = (base + i < n) ? in[base + i] : 0;
    }
#pragma unroll
    for (int i = 0; i < F3DG_SCAN_ITEMS; i++) s += v[i];
    u32 run = block_sums[blockIdx.x] + block_scan_exclusive<F3DG_BLOCK / 64>(s, wtot);
    u32 o[F3DG_SCAN_ITEMS];
#pragma unroll
    for (int i = 0; i < F3DG_SCAN_ITEMS; i++) {
        const u32 before = run;
        run += v[i];
        o[i] = exclusive ? before : run;
    }
    if (base + F3DG_SCAN_ITEMS <= n) {
#pragma unroll
        for (int i = 0; i < F3DG_SCAN_ITEMS / 4; i++)
            reinterpret_cast<uint4*>(out + base)[i] = make_uint4(o[4 * i], o[4 * i + 1], o[4 * i + 2], o[4 * i + 3]);
    } else {
#pragma unroll
        for (int i = 0; i < F3DG_SCAN_ITEMS; i++)
            if (base + i < n) out[base + i] = o[i];
    }
}

// ================================================================================================ depth-first binning
// Round 1 grouped the instances by tile first and then sorted every (view, tile) group by depth in LDS; that per-tile sort was the
// largest binning kernel (1.0 of 2.3 ms at C2, 4.9 of 12 ms at C5: latency-bound), and it sorted every INSTANCE (R = 3-7 per
// Gaussian). A Gaussian's depth is the same in all its tiles, so the depth order is established once per (view, Gaussian) instead:
//   1. gsort: stable LSD radix sort of each view's P Gaussians by their depth bits (4 passes of 8 bits over V*P keys; culled
//      Gaussians get the key ~0 and produce no instances) -> perm[V][P], ascending (depth, Gaussian id);
//   2. the tile rectangles gathered in that order, their areas summed per 256 positions and those sums scanned, and the instances are
//      GENERATED in (view, depth, id) order, as two streams: group (view << tile_bits | tile, u16 or u32) and Gaussian id;
//   3. stable pass(es) over the tile bits INSIDE every view's segment of the instance arrays: the result is in (view, tile, depth,
//      id) order, i.e. the final list, and a view's instances never leave one XCD's L2;
//   4. identifyTileRanges on the final group stream.
// Same final list as a stable 64-bit sort of (tile << 32 | depth) keys, i.e. the reference's.

// ------------------------------------------------------------------------------------------------ segmented radix passes
// Two-stream (key, payload) stable 8-bit radix pass over SEGMENTS of the arrays (a segment = one view): elements never leave their
// segment, so the arrays stay view-major and a view's data stays in one XCD's L2 (f3dg_xcd_map / the per-XCD work lists below).
// A workgroup takes one chunk of F3DG_SORT_CHUNK elements of one segment. The counts of digit d of chunk c go to
// hist[obase + d * cps + c] (obase = 256 * chunks of all earlier segments), so that ONE exclusive scan of the whole array yields the
// global output positions: every segment owns exactly its own index range of the output.
struct SegChunk {
    u64 seg_base;   // first element of the segment in the key / payload arrays
    u64 obase;      // first entry of the segment's [256][cps] block of the histogram
    u32 n;          // elements of the segment
    u32 cps;        // chunks of the segment
    u32 c;          // the chunk
    u32 seg;        // the segment (fixed segments only)
};

// Variable-length segments (the instances of every view): built on the device by view_segments_kernel
struct SegTable {
    const u32* vstart;      // [V + 1] first instance of every view
    const u32* bglob;       // [V + 1] chunks of all earlier views
    const u32* xprefix;     // [8][xstride] XCD x works on the views x, x + 8, ...: chunks of its earlier views
    u32 xstride;            // V / 8 + 2
    u32 V;
};

// digit of a key in one pass
struct ShiftDigit {
    int shift;
    u32 mask = 255u;        // (a pass over fewer than 8 bits: the tile passes split their bits evenly)
    __device__ __forceinline__ u32 operator()(u32 k) const { return (k >> shift) & mask; }
};

template <typename K, typename DIGIT, bool MINMAX = false>
__device__ __forceinline__ void hist_chunk(const K* __restrict__ keys, const SegChunk& ck, const DIGIT digit, u32* __restrict__ hist,
                                           u32 (*h)[256], u32* __restrict__ minmax = nullptr)
{
    u32 kmin = 0xFFFFFFFFu, kmax = 0u;        // MINMAX: range of the keys other than ~0 (Gaussians that touch no tile)
#pragma unroll
    for (int w = 0; w < F3DG_BLOCK / 64; w++) h[w][threadIdx.x] = 0;
    __syncthreads();
    u32* hw = h[threadIdx.x >> 6];
    constexpr int VEC = 16 / (int)sizeof(K);                   // keys per 16-byte load
    typedef K __attribute__((ext_vector_type(VEC))) KV;
    // the chunk's elements [g0, g1) of the array, read as ALIGNED 16-byte vectors (a segment may start anywhere): the first and the
    // last vector are masked. (The few bytes read outside the chunk are inside the array, whose regions are padded to 256 bytes.)
    const u64 base = (u64)ck.c * F3DG_SORT_CHUNK;
    const u64 g0 = ck.seg_base + base;
    const u64 g1 = ck.seg_base + ((u64)ck.n - base < (u64)F3DG_SORT_CHUNK ? (u64)ck.n : base + F3DG_SORT_CHUNK);
    for (u64 a = (g0 & ~(u64)(VEC - 1)) + (u64)threadIdx.x * VEC; a < g1; a += (u64)F3DG_BLOCK * VEC) {
        const KV w = *reinterpret_cast<const KV*>(keys + a);
#pragma unroll
        for (int q = 0; q < VEC; q++) {
            if (a + q >= g0 && a + q < g1) {
                const u32 key = (u32)w[q];
                atomicAdd(&hw[digit(key)], 1u);
                if (MINMAX && key != 0xFFFFFFFFu) { kmin = key < kmin ? key : kmin; kmax = key > kmax ? key : kmax; }
            }
        }
    }
    __shared__ u32 wmm[2][F3DG_BLOCK / 64];
    if (MINMAX) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const u32 a = __shfl_down(kmin, off, 64), b = __shfl_down(kmax, off, 64);
            kmin = a < kmin ? a : kmin; kmax = b > kmax ? b : kmax;
        }
        if ((threadIdx.x & 63) == 0) { wmm[0][threadIdx.x >> 6] = kmin; wmm[1][threadIdx.x >> 6] = kmax; }
    }
    __syncthreads();
    if (MINMAX && threadIdx.x == 0) {       // the chunk's range (kmin > kmax: no key other than ~0); reduced per view by gsort_range_kernel
        u32 a = wmm[0][0], b = wmm[1][0];
#pragma unroll
        for (int w = 1; w < F3DG_BLOCK / 64; w++) { a = wmm[0][w] < a ? wmm[0][w] : a; b = wmm[1][w] > b ? wmm[1][w] : b; }
        minmax[0] = a; minmax[1] = b;
    }
    hist[ck.obase + (u64)threadIdx.x * ck.cps + ck.c] = h[0][threadIdx.x] + h[1][threadIdx.x] + h[2][threadIdx.x] + h[3][threadIdx.x];
}

struct ScatterShared {
    u32 cnt[F3DG_BLOCK / 64][256];
    u32 lbase[256];
    u32 gdelta[256];
    u32 wtot[F3DG_BLOCK / 64];
    u32 sval[F3DG_SORT_CHUNK];
};

// the key a pass hands to the next one: as it is, or without the bits that no later pass reads (compact views of the depth sort)
struct KeepKey {
    __device__ __forceinline__ u32 operator()(u32 k) const { return k; }
};
// 32 -> 16 bits behind pass 0 of a compact view: bits 8..23 of key - kbase (every key that touches a tile is below 2^24 there); the
// key ~0 of a Gaussian that touches no tile becomes 0xFFFF, digit 255 of both later passes as before
struct Narrow16 {
    u32 kbase;
    __device__ __forceinline__ u32 operator()(u32 k) const { return k == 0xFFFFFFFFu ? 0xFFFFu : (k - kbase) >> 8; }
};
// 16 -> 8 bits behind pass 1 of a compact view: what is left is the digit of pass 2
struct Narrow8 {
    __device__ __forceinline__ u32 operator()(u32 k) const { return k >> 8; }
};

// The entry of the scanned histogram that holds the first output position of digit threadIdx.x of a chunk (F3DG_BLOCK = 256 digits).
__device__ __forceinline__ u64 chunk_offset_entry(const SegChunk& ck) { return ck.obase + (u64)threadIdx.x * ck.cps + ck.c; }

// IOTA: the payload of the input is its position inside the segment (first pass of the depth sort).
// K is the key type read (and staged in LDS: the digit is taken from it), KO the one written, narrow(key). keys_in is indexed like
// vals_in, by seg_base + position in the segment, and keys_out like vals_out, by the position the scan gives: for keys narrower than
// 32 bits the caller passes pointers moved to where that index finds the segment's keys (gsort_keys).
// goff is offsets[chunk_offset_entry(ck)], which the caller loads BEFORE the call: the address depends on the chunk alone, so the
// round trip runs beside the key loads and the ranking instead of standing alone between two barriers. A persistent caller names its
// next chunk (next, or null): that chunk's entry is asked for ahead of the write-out and returned in goff.
template <typename K, typename KO, bool IOTA, typename DIGIT, typename NARROW>
__device__ __forceinline__ void scatter_chunk(const K* __restrict__ keys_in, const u32* __restrict__ vals_in, KO* __restrict__ keys_out,
                                              u32* __restrict__ vals_out, const SegChunk& ck, const DIGIT digit, const NARROW narrow,
                                              const u32* __restrict__ offsets /* exclusive scan of hist */, u32& goff, const SegChunk* next, ScatterShared& sh, K* skey)
{
    // the chunk is digit-sorted inside LDS (stable), then written out in coalesced runs
    const u32 n = ck.n;
    const u64 block_base = (u64)ck.c * F3DG_SORT_CHUNK;
    const u32 in_block = (u32)((n - block_base) < (u64)F3DG_SORT_CHUNK ? (n - block_base) : (u64)F3DG_SORT_CHUNK);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int w = 0; w < F3DG_BLOCK / 64; w++) sh.cnt[w][threadIdx.x] = 0;
    __syncthreads();

    const u64 wave_base = block_base + (u64)wave * (64 * F3DG_SORT_ITEMS);
    u32 key[F3DG_SORT_ITEMS];
    u32 val[F3DG_SORT_ITEMS];
    u32 rank[F3DG_SORT_ITEMS];
    const u64 lane_lt = ((u64)1 << lane) - 1;
#pragma unroll
    for (int r = 0; r < F3DG_SORT_ITEMS; r++) {          // all loads first
        const u64 i = wave_base + (u64)r * 64 + lane;
        const bool valid = i < n;
        key[r] = valid ? (u32)keys_in[ck.seg_base + i] : 0u;
        val[r] = IOTA ? (u32)i : (valid ? vals_in[ck.seg_base + i] : 0u);
    }
#pragma unroll
    for (int r = 0; r < F3DG_SORT_ITEMS; r++) {
        const u64 i = wave_base + (u64)r * 64 + lane;
        const bool valid = i < n;
        const u32 d = digit(key[r]);
        // lanes with the same digit: a lane differs from lane L in bit b exactly where ballot(bit b) disagrees with L's own bit
        // (sign-extended over the mask: one v_bfe_i32); the eight mismatch masks are OR-ed (v_or3) and inverted once
        u64 diff = 0;
#pragma unroll
        for (int b = 0; b < 8; b++) {
            const u32 own = (u32)((int)(d << (31 - b)) >> 31);
            const u64 bal = __ballot(own != 0u);
            diff |= bal ^ (((u64)own << 32) | own);
        }
        const u64 same = __ballot(valid) & ~diff;
        const u32 below = (u32)__popcll(same & lane_lt);
        const u32 prev = sh.cnt[wave][d];
        rank[r] = prev + below;
        __builtin_amdgcn_wave_barrier();
        if (valid && below == 0) sh.cnt[wave][d] = prev + (u32)__popcll(same);
        __builtin_amdgcn_wave_barrier();
    }
    __syncthreads();
    {
        const u32 d = threadIdx.x;
        const u32 c0 = sh.cnt[0][d], c1 = sh.cnt[1][d], c2 = sh.cnt[2][d], c3 = sh.cnt[3][d];
        const u32 tot = c0 + c1 + c2 + c3;
        const u32 excl = block_scan_exclusive<F3DG_BLOCK / 64>(tot, sh.wtot);
        sh.lbase[d] = excl;
        sh.gdelta[d] = goff - excl;
        sh.cnt[0][d] = excl;
        sh.cnt[1][d] = excl + c0;
        sh.cnt[2][d] = excl + c0 + c1;
        sh.cnt[3][d] = excl + c0 + c1 + c2;
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < F3DG_SORT_ITEMS; r++) {
        const u64 i = wave_base + (u64)r * 64 + lane;
        if (i < n) {
            const u32 d = digit(key[r]);
            const u32 slot = sh.cnt[wave][d] + rank[r];
            skey[slot] = (K)key[r];
            sh.sval[slot] = val[r];
        }
    }
    __syncthreads();
    if (next) goff = offsets[chunk_offset_entry(*next)];
    for (u32 slot = threadIdx.x; slot < in_block; slot += F3DG_BLOCK) {
        const K k = skey[slot];
        const u32 d = digit((u32)k);
        const u32 pos = sh.gdelta[d] + slot;          // global position (the scan spans all segments)
        if (keys_out) keys_out[pos] = (KO)narrow((u32)k);
        vals_out[pos] = sh.sval[slot];
    }
}

// ---- equal segments of seg_len elements (the per-view depth sort of the Gaussians): one chunk per workgroup.
// Pass 0, which reads every key cold anyway, also finds every chunk's key range, reduced to every view's [kmin, kmax] (minmax[2 v],
// [2 v + 1]) by gsort_range_kernel before the pass's scatter runs. A view whose range fits 2^24 above kbase = kmin & ~0xFFFF is
// "compact": its third pass sorts by (key - kbase) >> 16 and is its last, the fourth returns at once -- histogram, per-view scan and
// scatter; only under the general scan, which spans all views, its histogram is a stand-in with the right sum so that the scan keeps
// the other views' positions --, and the view's order is the OUTPUT OF PASS 2 (see gsort_gather_rects_kernel). Depth ranges within a
// factor of 2-4 -- object-centric cameras -- are compact; others take the four plain passes.
//
// A compact view's keys also lose, pass by pass, the bytes that no later pass reads: pass 0 writes (key - kbase) >> 8 in 16 bits
// (Narrow16; kbase is a multiple of 2^16, so bits 8..15 are the key's own, the digit of pass 1), pass 1 writes the top 8 of those
// (Narrow8), which IS the digit of pass 2, and pass 2 writes no keys. The digits are the ones of the 32-bit keys, so the order is
// the same element for element. The narrow keys of view v lie at the start of the view's own P * 4 bytes of the key array, which a
// non-compact view of the same call fills with 32-bit keys: one launch per pass serves both, a workgroup branches on its view.
__device__ __forceinline__ SegChunk fixed_chunk(u32 seg_len, u32 cps)
{
    u32 seg, c;
    f3dg_xcd_map(blockIdx.x, gridDim.x / cps, cps, seg, c);
    SegChunk ck;
    ck.seg_base = (u64)seg * seg_len; ck.obase = (u64)seg * 256u * cps; ck.n = seg_len; ck.cps = cps; ck.c = c; ck.seg = seg;
    return ck;
}

// the chunk with its segment's first key counted in units of K from the base of the (u32) key array: what hist_chunk, whose aligned
// vectors are counted from that base, takes for narrow keys
template <typename K>
__device__ __forceinline__ SegChunk narrow_chunk(SegChunk ck)
{
    ck.seg_base *= 4u / (u32)sizeof(K);
    return ck;
}
// the key array as keys of type K, moved so that the index of the payload arrays (seg_base + position in the segment, which is also
// the output position the scan gives) finds the segment's narrow keys
template <typename K>
__device__ __forceinline__ K* gsort_keys(const u32* keys, const SegChunk& ck)
{
    return reinterpret_cast<K*>(const_cast<u32*>(keys)) + ck.seg_base * (4u / (u32)sizeof(K) - 1u);
}

__device__ __forceinline__ bool gsort_compact(const u32* __restrict__ minmax, u32 view, u32& kbase)
{
    const u32 kmin = minmax[2 * view], kmax = minmax[2 * view + 1];
    kbase = kmin & 0xFFFF0000u;
    return kmin <= kmax && ((kmax - kbase) >> 24) == 0u;
}

template <int PASS>
__global__ void __launch_bounds__(F3DG_BLOCK)
gsort_hist_kernel(const u32* __restrict__ keys, u32 seg_len, u32 cps, u32* __restrict__ hist, const u32* __restrict__ minmax,
                  u32* __restrict__ chunk_minmax, int standin /* pass 3 of a compact view: 1 when ONE scan spans all views */)
{
    __shared__ u32 h[F3DG_BLOCK / 64][256];
    const SegChunk ck = fixed_chunk(seg_len, cps);
    if constexpr (PASS == 0) {               // (no view's range is known yet: the digit is the low byte of the 32-bit key either way)
        hist_chunk<u32, ShiftDigit, true>(keys, ck, ShiftDigit{0}, hist, h, chunk_minmax + 2 * ((size_t)ck.seg * cps + ck.c));
    } else {
        u32 kbase;
        const bool compact = gsort_compact(minmax, ck.seg, kbase);
        if (!compact) {
            hist_chunk<u32, ShiftDigit>(keys, ck, ShiftDigit{8 * PASS}, hist, h);
        } else if constexpr (PASS == 1) {
            hist_chunk<u16, ShiftDigit>(reinterpret_cast<const u16*>(keys), narrow_chunk<u16>(ck), ShiftDigit{0}, hist, h);
        } else if constexpr (PASS == 2) {
            hist_chunk<u8, ShiftDigit>(reinterpret_cast<const u8*>(keys), narrow_chunk<u8>(ck), ShiftDigit{0}, hist, h);
        } else if (standin) {
            const u64 base = (u64)ck.c * F3DG_SORT_CHUNK;
            const u32 in_chunk = (u32)((ck.n - base) < (u64)F3DG_SORT_CHUNK ? (ck.n - base) : (u64)F3DG_SORT_CHUNK);
            hist[ck.obase + (u64)threadIdx.x * ck.cps + ck.c] = threadIdx.x == 0 ? in_chunk : 0u;
        }
    }
}

// exclusive scan of one view's [256][cps] histogram block in place, starting from the view's first output position: the views'
// position ranges are known in advance (seg_len each), so every view is scanned by its own workgroup -- one launch per pass
// instead of the three of the general scan
__global__ void __launch_bounds__(1024)
gsort_scan_kernel(u32 n_per_seg /* 256 cps */, u32 seg_len, u32* __restrict__ hist, const u32* __restrict__ skip_compact /* pass 3: minmax */)
{
    __shared__ u32 wtot[16];
    u32 kbase;
    if (skip_compact && gsort_compact(skip_compact, blockIdx.x, kbase)) return;      // nothing reads the table of a compact view's pass 3
    // (n_per_seg is a multiple of 256: whole uint4s)
    scan_array_in_place<16, 4, u32>(hist + (size_t)blockIdx.x * n_per_seg, n_per_seg, blockIdx.x * seg_len, wtot);
}

// key range of every view from the ranges of its chunks (one wave per view)
__global__ void __launch_bounds__(64)
gsort_range_kernel(u32 cps, const u32* __restrict__ chunk_minmax, u32* __restrict__ minmax)
{
    u32 kmin = 0xFFFFFFFFu, kmax = 0u;
    for (u32 c = threadIdx.x; c < cps; c += 64) {
        const u32 a = chunk_minmax[2 * ((size_t)blockIdx.x * cps + c)], b = chunk_minmax[2 * ((size_t)blockIdx.x * cps + c) + 1];
        kmin = a < kmin ? a : kmin; kmax = b > kmax ? b : kmax;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const u32 a = __shfl_down(kmin, off, 64), b = __shfl_down(kmax, off, 64);
        kmin = a < kmin ? a : kmin; kmax = b > kmax ? b : kmax;
    }
    if (threadIdx.x == 0) { minmax[2 * blockIdx.x] = kmin; minmax[2 * blockIdx.x + 1] = kmax; }
}

template <int PASS>
__global__ void __launch_bounds__(F3DG_BLOCK)
gsort_scatter_kernel(const u32* __restrict__ keys_in, const u32* __restrict__ vals_in, u32* __restrict__ keys_out,
                     u32* __restrict__ vals_out, u32 seg_len, u32 cps, const u32* __restrict__ offsets, const u32* __restrict__ minmax)
{
    __shared__ ScatterShared sh;
    __shared__ u32 skey[F3DG_SORT_CHUNK];          // (keys of the type the pass reads: a narrow pass uses the front of it)
    const SegChunk ck = fixed_chunk(seg_len, cps);
    u32 goff = offsets[chunk_offset_entry(ck)];
    u32 kbase;
    const bool compact = gsort_compact(minmax, ck.seg, kbase);
    // (the keys are not read again after a view's LAST pass -- pass 2 of a compact view, pass 3 otherwise --: it does not write them)
    if (!compact) {
        scatter_chunk<u32, u32, PASS == 0, ShiftDigit, KeepKey>(keys_in, vals_in, PASS == 3 ? (u32*)nullptr : keys_out, vals_out, ck, ShiftDigit{8 * PASS},
                                                                KeepKey{}, offsets, goff, nullptr, sh, skey);
    } else if constexpr (PASS == 0) {    // the payload of the input is its position inside the segment
        scatter_chunk<u32, u16, true, ShiftDigit, Narrow16>(keys_in, vals_in, gsort_keys<u16>(keys_out, ck), vals_out, ck, ShiftDigit{0}, Narrow16{kbase},
                                                            offsets, goff, nullptr, sh, skey);
    } else if constexpr (PASS == 1) {
        scatter_chunk<u16, u8, false, ShiftDigit, Narrow8>(gsort_keys<u16>(keys_in, ck), vals_in, gsort_keys<u8>(keys_out, ck), vals_out, ck, ShiftDigit{0},
                                                           Narrow8{}, offsets, goff, nullptr, sh, reinterpret_cast<u16*>(skey));
    } else if constexpr (PASS == 2) {
        scatter_chunk<u8, u8, false, ShiftDigit, KeepKey>(gsort_keys<u8>(keys_in, ck), vals_in, (u8*)nullptr, vals_out, ck, ShiftDigit{0}, KeepKey{},
                                                          offsets, goff, nullptr, sh, reinterpret_cast<u8*>(skey));
    }
}

// ---- the instances of every view (variable segments): persistent workgroups. Workgroup b belongs to XCD b % 8 and walks that
// XCD's list of (view, chunk) pairs -- views x, x + 8, ... chunk by chunk -- with stride gridDim.x / 8.

// exclusive scan in place of one view's nb block sums (gsort_gather_rects_kernel), view-local; the view's total goes to view_total[view]
// in 64 bits (a batch can hold more than 2^32 instances: V * P * tiles)
__global__ void __launch_bounds__(1024)
block_sums_scan_kernel(u32 nb, u32* __restrict__ block_sums, u64* __restrict__ view_total)
{
    __shared__ u64 wtot[16];
    const u64 total = scan_array_in_place<16, 1, u64>(block_sums + (size_t)blockIdx.x * nb, nb, 0u, wtot);
    if (threadIdx.x == 0) view_total[blockIdx.x] = total;
}

// vstart / bglob / xprefix from the views' instance totals, and the call's status: the total of all views (64 bits: a wrapped 32-bit
// total must not pass for a small one, later kernels index the instance arrays with it) against the capacity. All tables zero --
// no chunks -- on overflow.
__global__ void __launch_bounds__(512)
view_segments_kernel(int V, const u64* __restrict__ view_total, F3dgHeader* __restrict__ hdr, u32* __restrict__ vstart,
                     u32* __restrict__ bglob, u32* __restrict__ xprefix, u32 xstride)
{
    __shared__ u64 wtot_v[8];
    __shared__ u32 wtot_c[8];
    const u32 lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    // first instance of every view (its low 32 bits are the whole of it unless the call overflows)
    u64 total = 0;
    for (u32 v0 = 0; v0 < (u32)V; v0 += 512) {
        const u32 v = v0 + threadIdx.x;
        u64 round;
        const u64 before = block_scan_exclusive<8>(v < (u32)V ? view_total[v] : 0ull, wtot_v, round);
        if (v < (u32)V) vstart[v] = (u32)(total + before);
        total += round;
        __syncthreads();
    }
    const bool dead = set_status(hdr, total);
    if (threadIdx.x == 0) vstart[V] = dead ? 0u : (u32)total;
    if (dead)
        for (u32 v = threadIdx.x; v < (u32)V; v += 512) vstart[v] = 0u;
    __syncthreads();
    auto chunks_of = [&](u32 v) -> u32 {
        const u32 n = vstart[v + 1] - vstart[v];
        return (n + F3DG_SORT_CHUNK - 1) / F3DG_SORT_CHUNK;
    };
    // global chunk prefix, view order
    u32 chunks = 0;
    for (u32 v0 = 0; v0 < (u32)V; v0 += 512) {
        const u32 v = v0 + threadIdx.x;
        u32 round;
        const u32 before = block_scan_exclusive<8>(v < (u32)V ? chunks_of(v) : 0u, wtot_c, round);
        if (v < (u32)V) bglob[v] = chunks + before;
        chunks += round;
        __syncthreads();
    }
    if (threadIdx.x == 0) bglob[V] = chunks;
    // per-XCD prefix: wave x scans the chunks of the views x, x + 8, ...
    const u32 nk = ((u32)V > wave) ? ((u32)V - wave + 7u) / 8u : 0u;
    u32 run = 0;
    for (u32 k0 = 0; k0 < nk; k0 += 64) {
        const u32 k = k0 + lane;
        const u32 c = k < nk ? chunks_of(wave + 8u * k) : 0u;
        const u32 x = wave_scan_inclusive(c, lane);
        if (k < nk) xprefix[wave * xstride + k] = run + x - c;
        run += __shfl(x, 63, 64);
    }
    if (lane == 0) xprefix[wave * xstride + nk] = run;
}

// exclusive scan of one view's [256][chunks of the view] histogram block of a tile pass in place, starting from the view's first
// instance (as gsort_scan_kernel: the views' output ranges are known, vstart). radix2_hist_var_kernel writes every entry of a live
// block, so nothing is cleared beforehand and nothing outside the live blocks is touched -- but ranges_from_offsets_kernel reads the
// entry after a view's block as the end of its digit 255: the first entry of the next view's block (= vstart of that view, and of
// any view without instances in between), and behind the last block a sentinel that holds the total.
__global__ void __launch_bounds__(1024)
tile_scan_kernel(u32 V, const u32* __restrict__ vstart, const u32* __restrict__ bglob, u32* __restrict__ hist)
{
    __shared__ u32 wtot[16];
    const u32 b0 = bglob[blockIdx.x], n = 256u * (bglob[blockIdx.x + 1] - b0);
    if (blockIdx.x == 0 && threadIdx.x == 0) hist[256ull * bglob[V]] = vstart[V];
    // (16 consecutive entries per thread: four 16-byte loads; n is a multiple of 256)
    scan_array_in_place<16, 16, u32>(hist + 256ull * b0, n, vstart[blockIdx.x], wtot);
}

// identifyTileRanges when ONE pass sorted the tile bits: the scanned histogram already holds the first position of every
// (view, tile) group -- hist[256 bglob[v] + digit * chunks_v] -- and the next entry in scan order is where it ends
__global__ void __launch_bounds__(F3DG_BLOCK)
ranges_from_offsets_kernel(u32 V, u32 T, int tile_bits, const u32* __restrict__ bglob, const u32* __restrict__ offsets,
                           const F3dgHeader* __restrict__ hdr, uint2* __restrict__ ranges)
{
    const u32 i = blockIdx.x * F3DG_BLOCK + threadIdx.x;
    if (i >= V * T) return;
    const u32 v = i / T, t = i % T;
    const u32 b0 = bglob[v], cpv = bglob[v + 1] - b0;
    uint2 r = make_uint2(0u, 0u);
    if (cpv != 0u && !hdr->overflow) {
        const u32 d = ((v << tile_bits) | t) & 255u;           // the digit of the group: below 8 tile bits it holds view bits too
        const u32 lo = offsets[256ull * b0 + (u64)d * cpv], hi = offsets[256ull * b0 + (u64)(d + 1u) * cpv];
        if (hi > lo) r = make_uint2(lo, hi);
    }
    ranges[i] = r;
}

// next (view, chunk) of this workgroup's XCD list; false when the list is exhausted. k is the cursor into the XCD's views.
__device__ __forceinline__ bool var_chunk(const SegTable& st, u32 f, u32& k, SegChunk& ck)
{
    const u32 x = blockIdx.x & 7u;
    const u32* xp = st.xprefix + x * st.xstride;
    const u32 nk = (st.V > x) ? (st.V - x + 7u) / 8u : 0u;
    while (k < nk && f >= xp[k + 1]) k++;
    if (k >= nk) return false;
    const u32 v = x + 8u * k;
    const u32 s0 = st.vstart[v], b0 = st.bglob[v];
    ck.seg_base = s0; ck.n = st.vstart[v + 1] - s0; ck.cps = st.bglob[v + 1] - b0; ck.obase = 256ull * b0; ck.c = f - xp[k];
    return true;
}

template <typename K>
__global__ void __launch_bounds__(F3DG_BLOCK)
radix2_hist_var_kernel(const K* __restrict__ keys, SegTable st, int shift, u32 mask, u32* __restrict__ hist)
{
    __shared__ u32 h[F3DG_BLOCK / 64][256];
    u32 k = 0;
    SegChunk ck;
    for (u32 f = blockIdx.x >> 3; var_chunk(st, f, k, ck); f += gridDim.x >> 3)
        hist_chunk<K, ShiftDigit>(keys, ck, ShiftDigit{shift, mask}, hist, h);
}

// (four waves per SIMD is what the LDS allows; the registers are held to it, 128, now that the next chunk's offset is carried along)
template <typename K>
__global__ void __launch_bounds__(F3DG_BLOCK) __attribute__((amdgpu_waves_per_eu(4, 4)))
radix2_scatter_var_kernel(const K* __restrict__ keys_in, const u32* __restrict__ vals_in, K* __restrict__ keys_out,
                          u32* __restrict__ vals_out, SegTable st, int shift, u32 mask, const u32* __restrict__ offsets)
{
    __shared__ ScatterShared sh;
    __shared__ K skey[F3DG_SORT_CHUNK];
    const u32 stride = gridDim.x >> 3;
    u32 k = 0, f = blockIdx.x >> 3;
    SegChunk ck, next;
    bool live = var_chunk(st, f, k, ck);
    u32 goff = live ? offsets[chunk_offset_entry(ck)] : 0u;
    while (live) {
        // the next chunk is looked up first: its entry of the offsets is asked for while this chunk is written out
        u32 kn = k;
        const bool more = var_chunk(st, f + stride, kn, next);
        scatter_chunk<K, K, false, ShiftDigit, KeepKey>(keys_in, vals_in, keys_out, vals_out, ck, ShiftDigit{shift, mask}, KeepKey{}, offsets, goff,
                                                        more ? &next : (const SegChunk*)nullptr, sh, skey);
        __syncthreads();          // the LDS staging area is reused by the next chunk
        ck = next; k = kn; f += stride; live = more;
    }
}

// instances of a tile rectangle (written by the projection kernel: x = rminx | rmaxx << 16, y = rminy | rmaxy << 16) = its
// tiles_touched. ONE definition: gsort_gather_rects_kernel reserves the output range that duplicate_sorted_kernel fills.
__device__ __forceinline__ u32 rect_instances(u32 x, u32 y)
{
    const u32 rminx = x & F3DG_RECT_COORD, rmaxx = (x >> 16) & F3DG_RECT_COORD, rminy = y & F3DG_RECT_COORD, rmaxy = (y >> 16) & F3DG_RECT_COORD;
    return (rmaxx > rminx && rmaxy > rminy) ? (rmaxx - rminx) * (rmaxy - rminy) : 0u;
}

// tile rectangles gathered into sorted order: the one random gather of the path. The instances are placed from the sums of their
// counts over every F3DG_BLOCK consecutive depth positions of a view -- the 256 Gaussians of one duplicate_sorted_kernel workgroup --,
// block_sums[view][nb]: the per-position counts never reach memory, duplicate_sorted_kernel rebuilds them from the rectangles.
__global__ void __launch_bounds__(F3DG_BLOCK)
gsort_gather_rects_kernel(int P, u32* __restrict__ gv0, u32* __restrict__ gv1, const u32* __restrict__ minmax,
                          const uint2* __restrict__ rects, u32* __restrict__ block_sums, u32* __restrict__ rx)
{
    constexpr int ITEMS = 4;                  // four independent gathers in flight per thread
    __shared__ u32 wsum[ITEMS][F3DG_BLOCK / 64];
    unsigned view, chunk;                     // a view's rectangles (8 P bytes) are gathered through one XCD's L2
    const unsigned cpv = (unsigned)((P + F3DG_BLOCK * ITEMS - 1) / (F3DG_BLOCK * ITEMS));
    f3dg_xcd_map(blockIdx.x, gridDim.x / cpv, cpv, view, chunk);
    const size_t vb = (size_t)view * P;
    // the view's order is in gv1 after three passes (compact key range) or in gv0 after four; the other one takes ry
    u32 kbase;
    const bool pass2 = gsort_compact(minmax, view, kbase);
    const u32* perm = pass2 ? gv1 : gv0;
    u32* ry = pass2 ? gv0 : gv1;
    const int k0 = (int)(chunk * F3DG_BLOCK * ITEMS + threadIdx.x);
    u32 id[ITEMS];
    uint2 r[ITEMS];
    // (positions past P read the view's last one, P - 1, and are masked afterwards: loads under a condition become branches with a
    // wait each, and the gathers would go out one after the other)
#pragma unroll
    for (int i = 0; i < ITEMS; i++) { const int k = k0 + i * F3DG_BLOCK; id[i] = perm[vb + (k < P ? k : P - 1)]; }
#pragma unroll
    for (int i = 0; i < ITEMS; i++) r[i] = rects[vb + id[i]];
#pragma unroll
    for (int i = 0; i < ITEMS; i++) {
        const int k = k0 + i * F3DG_BLOCK;
        const u32 live = k < P ? 0xFFFFFFFFu : 0u;
        r[i].x &= live; r[i].y &= live;
        if (k < P) {
            rx[vb + k] = r[i].x;
            ry[vb + k] = r[i].y;
        }
        // item i of all threads is block ITEMS * chunk + i of the view (positions past P hold the empty rectangle)
        u32 sum = rect_instances(r[i].x, r[i].y);
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) sum += __shfl_down(sum, off, 64);
        if ((threadIdx.x & 63) == 0) wsum[i][threadIdx.x >> 6] = sum;
    }
    __syncthreads();
    const unsigned nb = (unsigned)((P + F3DG_BLOCK - 1) / F3DG_BLOCK);
    const unsigned blk = chunk * ITEMS + threadIdx.x;
    if (threadIdx.x < ITEMS && blk < nb)
        block_sums[(size_t)view * nb + blk] = wsum[threadIdx.x][0] + wsum[threadIdx.x][1] + wsum[threadIdx.x][2] + wsum[threadIdx.x][3];
}

// duplicateWithKeys in (view, depth, id) order: sorted position k of view v emits the tiles of Gaussian perm[v][k]. The runs of a
// workgroup's 256 Gaussians are consecutive in the output (a few instances each), so they are assembled in LDS and written out as
// whole lines, DUP_CAP instances per window.
#define F3DG_DUP_CAP 3072
template <typename G>
__global__ void __launch_bounds__(F3DG_BLOCK)
duplicate_sorted_kernel(int P, int tile_bits, int grid_x, const u32* __restrict__ gv0, const u32* __restrict__ gv1,
                        const u32* __restrict__ minmax, const u32* __restrict__ rx,
                        const u32* __restrict__ block_base /* [V][gridDim.x], view-local */, const u32* __restrict__ vstart /* or null */,
                        const F3dgHeader* __restrict__ hdr, G* __restrict__ kgrp, u32* __restrict__ vals)
{
    __shared__ G sk[F3DG_DUP_CAP];
    __shared__ u32 sv[F3DG_DUP_CAP];
    __shared__ u32 wtot[F3DG_BLOCK / 64];
    if (hdr->overflow) return;
    const int k = blockIdx.x * F3DG_BLOCK + threadIdx.x;
    const int v = blockIdx.y;
    u32 kbase;
    const bool pass2 = gsort_compact(minmax, (u32)v, kbase);      // as in gsort_gather_rects_kernel
    const u32* perm = pass2 ? gv1 : gv0;
    const u32* ry = pass2 ? gv0 : gv1;                             // the view's spare order buffer
    // output range of the workgroup: it starts at the view's first instance plus the instances of the view's earlier workgroups
    // (vstart null: the bases are global already, binning_tail)
    const u32 base = (vstart ? vstart[v] : 0u) + block_base[(size_t)v * gridDim.x + blockIdx.x];
    // the workgroup's output range [base, base + n) is assembled in LDS one window of F3DG_DUP_CAP instances at a time and written out
    // as whole lines: a thread emits the part of its Gaussian's run that falls into the window. (Until round 3 a workgroup whose
    // Gaussians cover more than one window wrote its runs directly -- a few bytes per lane, lines apart: with large splats, 24 tiles
    // per Gaussian at sigma0 = 0.05, that was every workgroup and the kernel ran at 1 TB/s.)
    u32 cnt = 0, x = 0, y = 0, g = 0;
    if (k < P) {
        const size_t pos = (size_t)v * P + k;
        x = rx[pos]; y = ry[pos]; g = perm[pos];         // (g is used where cnt != 0 only, but asked for with the rectangle, not behind it)
        cnt = rect_instances(x, y);
    }
    // a thread's run starts off0 instances into the range, which holds n: exclusive prefix and total of cnt over the workgroup
    u32 n;
    const u32 off0 = block_scan_exclusive<F3DG_BLOCK / 64>(cnt, wtot, n);
    const u32 rminx = x & F3DG_RECT_COORD, rmaxx = (x >> 16) & F3DG_RECT_COORD, rminy = y & F3DG_RECT_COORD, rmaxy = (y >> 16) & F3DG_RECT_COORD;
    const u32 view_base = (u32)v << tile_bits;
    // quadrant mask of an instance (f3dg_common.h: F3DG_ID_BITS): the halves of the first / last tile column and row that the
    // conservative box misses are cleared
    auto halves = [](u32 t, u32 tmin, u32 tmax, u32 word) -> u32 {
        u32 m = 3u;
        if (t == tmin && (word & F3DG_RECT_SKIP_LO)) m &= ~1u;
        if (t + 1u == tmax && (word & F3DG_RECT_SKIP_HI)) m &= ~2u;
        return m;
    };
    for (u32 wb = 0; wb < n; wb += (u32)F3DG_DUP_CAP) {
        const u32 lo = off0 > wb ? off0 : wb;
        const u32 hi = off0 + cnt < wb + (u32)F3DG_DUP_CAP ? off0 + cnt : wb + (u32)F3DG_DUP_CAP;
        if (lo < hi) {
            const u32 w = rmaxx - rminx, j0 = lo - off0;
            u32 ty = rminy + j0 / w, tx = rminx + j0 % w;
            u32 my = halves(ty, rminy, rmaxy, y);
            for (u32 j = lo; j < hi; j++) {
                const u32 mx = halves(tx, rminx, rmaxx, x);
                sk[j - wb] = (G)(view_base | (ty * (u32)grid_x + tx));
                sv[j - wb] = g | ((((my & 1u) ? mx : 0u) | ((my & 2u) ? mx << 2 : 0u)) << F3DG_ID_BITS);
                if (++tx == rmaxx) { tx = rminx; ty++; my = halves(ty, rminy, rmaxy, y); }
            }
        }
        __syncthreads();
        const u32 in_win = n - wb < (u32)F3DG_DUP_CAP ? n - wb : (u32)F3DG_DUP_CAP;
        for (u32 i = threadIdx.x; i < in_win; i += F3DG_BLOCK) {
            kgrp[base + wb + i] = sk[i];
            vals[base + wb + i] = sv[i];
        }
        __syncthreads();
    }
}

// debug export only: the 64-bit sort keys of the reference, (view << tile_bits | tile) << 32 | depth bits, of the final list
__global__ void __launch_bounds__(F3DG_BLOCK)
export_keys_kernel(u32 nseg, int P, int tile_bits, int T, const uint2* __restrict__ ranges, const F3dgHeader* __restrict__ hdr,
                   const u32* __restrict__ point_list, const float* __restrict__ depths, u64* __restrict__ keys_out)
{
    if (hdr->overflow) return;
    for (u32 seg = blockIdx.x; seg < nseg; seg += gridDim.x) {
        const uint2 r = ranges[seg];
        const u32 view = seg / (u32)T, tile = seg % (u32)T;
        const u64 hi = (u64)((view << tile_bits) | tile) << 32;
        for (u32 i = r.x + threadIdx.x; i < r.y; i += F3DG_BLOCK)
            keys_out[i] = hi | (u64)__float_as_uint(depths[(size_t)view * P + (point_list[i] & F3DG_ID_MASK)]);
    }
}

// identifyTileRanges: first / one-past-last index of every (view, tile) group of the final list, ranges[view * T + tile] (zeroed before)
template <typename G>
__global__ void __launch_bounds__(F3DG_BLOCK)
group_bounds_kernel(const G* __restrict__ kgrp, const F3dgHeader* __restrict__ hdr, int tile_bits, int T, u32* __restrict__ ranges)
{
    // every thread looks at 8 consecutive entries (one or two 16-byte loads) plus the entry on either side
    const u32 L = hdr->overflow ? 0u : hdr->num_rendered;
    const u32 tmask = (1u << tile_bits) - 1u;
    for (u64 base = ((u64)blockIdx.x * F3DG_BLOCK + threadIdx.x) * 8u; base < L; base += (u64)gridDim.x * F3DG_BLOCK * 8u) {
        G v[8];
        if (base + 8 <= L) {
            typedef G __attribute__((ext_vector_type(8))) G8;
            const G8 w = *reinterpret_cast<const G8*>(kgrp + base);          // base is a multiple of 8: aligned
#pragma unroll
            for (int i = 0; i < 8; i++) v[i] = w[i];
        } else {
#pragma unroll
            for (int i = 0; i < 8; i++) v[i] = base + i < L ? kgrp[base + i] : (G)0;
        }
        u32 prev = base > 0 ? (u32)kgrp[base - 1] : 0u;
        const u32 next = base + 8 < L ? (u32)kgrp[base + 8] : 0u;
#pragma unroll
        for (int i = 0; i < 8; i++) {
            const u64 idx = base + i;
            if (idx < L) {
                const u32 cur = (u32)v[i];
                const u32 nxt = i < 7 ? (u32)v[i + 1] : next;
                const u32 seg = (cur >> tile_bits) * (u32)T + (cur & tmask);
                if (idx == 0 || prev != cur) ranges[2u * seg] = (u32)idx;
                if (idx == L - 1 || nxt != cur) ranges[2u * seg + 1u] = (u32)idx + 1u;
                prev = cur;
            }
        }
    }
}

int bits_for(unsigned long long n_values)   // number of bits needed to represent values 0 .. n_values-1
{
    int b = 0;
    while (b < 64 && (n_values - 1) >> b) b++;
    return n_values <= 1 ? 0 : b;
}

} // namespace

int f3dg_launch_scan_inclusive(hipStream_t s, const unsigned* in, unsigned* out, unsigned long long n,
                               unsigned* tmp, unsigned tmp_elems, int exclusive, F3dgHeader* hdr_total)
{
    if (n == 0) return F3DG_OK;
    const unsigned nblocks = (unsigned)((n + F3DG_SCAN_CHUNK - 1) / F3DG_SCAN_CHUNK);
    if (nblocks > tmp_elems) return F3DG_ERR_WORKSPACE;
    F3DG_KLAUNCH(scan_reduce_kernel, dim3(nblocks), dim3(F3DG_BLOCK), 0, s, in, (u64)n, tmp);
    F3DG_KLAUNCH(scan_blocksums_kernel, dim3(1), dim3(1024), 0, s, tmp, nblocks, hdr_total);
    F3DG_KLAUNCH(scan_apply_kernel, dim3(nblocks), dim3(F3DG_BLOCK), 0, s, in, out, (u64)n, tmp, exclusive);
    F3DG_HIP_CHECK(hipGetLastError());
    return F3DG_OK;
}

int f3dg_tile_bits(int T) { return bits_for((unsigned long long)T); }

// Number of 8-bit passes over the instances: only the tile bits (instances are generated in (view, depth, id) order).

int f3dg_sort_passes(int V, int T)
{
    (void)V;
    const int bits = f3dg_tile_bits(T);
    return bits == 0 ? 0 : (bits + 7) / 8;
}

template <typename G>
static int binning_tail(hipStream_t s, int V, int P, int grid_x, int T, int tile_bits, const F3dgLayout& L, char* ws, F3dgHeader* hdr)
{
    int rc = F3DG_OK;
    const size_t VP = (size_t)V * P;
    u32* scan_tmp = reinterpret_cast<u32*>(ws + L.scan_tmp);
    u32* hist = reinterpret_cast<u32*>(ws + L.hist);
    u32* gk[2] = { reinterpret_cast<u32*>(ws + L.gsort), reinterpret_cast<u32*>(ws + L.gsort) + VP };
    u32* gv[2] = { reinterpret_cast<u32*>(ws + L.gsort) + 2 * VP, reinterpret_cast<u32*>(ws + L.gsort) + 3 * VP };
    G* kgrp[2] = { reinterpret_cast<G*>(ws + L.keys[0]), reinterpret_cast<G*>(ws + L.keys[1]) };   // (view << tile_bits | tile) per instance
    u32* vals[2] = { reinterpret_cast<u32*>(ws + L.vals[0]), reinterpret_cast<u32*>(ws + L.vals[1]) };
    const dim3 pgrid((P + F3DG_BLOCK - 1) / F3DG_BLOCK, V);

    // 1. per-view stable sort of the Gaussians by their sort keys (written by the projection kernel into gk[0]: the depth bits,
    //    ~0 for Gaussians that touch no tile); the first pass takes the Gaussian id from the position
    const u32 cps = (u32)((P + F3DG_SORT_CHUNK - 1) / F3DG_SORT_CHUNK);
    const u32 gblocks = (u32)V * cps;
    u32* minmax = reinterpret_cast<u32*>(ws + L.segtab) + L.segtab_minmax;
    u32* chunk_minmax = minmax + 2 * (size_t)V;
    const bool view_scan = cps <= 64;      // one workgroup per view (<= 4 rounds of 4096 entries) or the general three-kernel scan
#define F3DG_GSORT_PASS(PASS, IN, OUT)                                                                                                     \
    F3DG_KLAUNCH((gsort_hist_kernel<PASS>), dim3(gblocks), dim3(F3DG_BLOCK), 0, s, gk[IN], (u32)P, cps, hist, minmax, chunk_minmax, view_scan ? 0 : 1); \
    if (view_scan)                                                                                                                         \
        F3DG_KLAUNCH(gsort_scan_kernel, dim3(V), dim3(1024), 0, s, 256u * cps, (u32)P, hist, PASS == 3 ? minmax : (const u32*)nullptr); \
    else {                                                                                                                                 \
        rc = f3dg_launch_scan_inclusive(s, hist, hist, (unsigned long long)256 * gblocks, scan_tmp, L.scan_tmp_elems, 1, nullptr);        \
        if (rc != F3DG_OK) return rc;                                                                                                      \
    }                                                                                                                                      \
    if (PASS == 0)     /* the views' key ranges, from the chunks' that the histogram found: every scatter asks gsort_compact */           \
        F3DG_KLAUNCH(gsort_range_kernel, dim3(V), dim3(64), 0, s, cps, chunk_minmax, minmax);                                            \
    F3DG_KLAUNCH((gsort_scatter_kernel<PASS>), dim3(gblocks), dim3(F3DG_BLOCK), 0, s, gk[IN], gv[IN], gk[OUT], gv[OUT], (u32)P, cps, hist, minmax)
    F3DG_GSORT_PASS(0, 0, 1);
    F3DG_GSORT_PASS(1, 1, 0);
    F3DG_GSORT_PASS(2, 0, 1);
    F3DG_GSORT_PASS(3, 1, 0);
#undef F3DG_GSORT_PASS
    // a view's order (perm) is gv[1] after pass 2 if its key range is compact, gv[0] after pass 3 otherwise; the other one takes ry
    u32* block_sums = gk[1];              // [V][nb]: instances of every 256 consecutive depth positions, then their view-local exclusive prefix
    u32* rx = gk[0];
    u64* view_total = reinterpret_cast<u64*>(chunk_minmax);      // (the chunks' key ranges are spent: gsort_range_kernel reduced them)
    const u32 nb = (u32)((P + F3DG_BLOCK - 1) / F3DG_BLOCK);
    SegTable st;
    u32* segtab = reinterpret_cast<u32*>(ws + L.segtab);
    const u32 xstride = (u32)V / 8u + 2u;
    st.vstart = segtab; st.bglob = segtab + (V + 1); st.xprefix = segtab + 2 * (V + 1); st.xstride = xstride; st.V = (u32)V;

    // 2. instances in (view, depth, id) order: every workgroup of 256 depth positions gets its output range from the view's start
    //    (view_segments_kernel, which also settles the call's total and overflow status) and the view-local prefix of the block sums
    F3DG_KLAUNCH(gsort_gather_rects_kernel, dim3((unsigned)V * (unsigned)((P + 4 * F3DG_BLOCK - 1) / (4 * F3DG_BLOCK))), dim3(F3DG_BLOCK), 0, s, P, gv[0], gv[1], minmax,
                           reinterpret_cast<const uint2*>(ws + L.rects), block_sums, rx);
    const int passes = f3dg_sort_passes(V, T);
    if (passes > 0) {
        F3DG_KLAUNCH(block_sums_scan_kernel, dim3(V), dim3(1024), 0, s, nb, block_sums, view_total);
        F3DG_KLAUNCH(view_segments_kernel, dim3(1), dim3(512), 0, s, V, view_total, hdr, segtab, segtab + (V + 1), segtab + 2 * (V + 1), xstride);
    } else {
        // a one-tile image has no tile pass and no use for the segment tables: the general scan over the (short) array of block sums
        // makes the bases global and settles the status
        rc = f3dg_launch_scan_inclusive(s, block_sums, block_sums, (unsigned long long)V * nb, scan_tmp, L.scan_tmp_elems, 1, hdr);
        if (rc != F3DG_OK) return rc;
    }
    int src = passes & 1;                                                      // so that the tile pass(es) end in half 0
    F3DG_KLAUNCH((duplicate_sorted_kernel<G>), pgrid, dim3(F3DG_BLOCK), 0, s, P, tile_bits, grid_x, gv[0], gv[1], minmax, rx, block_sums,
                       passes > 0 ? segtab : (const u32*)nullptr, hdr, kgrp[src], vals[src]);

    // 3. stable pass(es) over the tile bits inside every view's segment of the instance arrays: (view, tile, depth, id) order
    if (passes > 0) {
        const size_t nbmax = (size_t)L.sort_blocks + (size_t)V;                // >= sum over the views of ceil(instances / chunk)
        const u32 per_xcd = (u32)((nbmax + 7) / 8 < 160 ? (nbmax + 7) / 8 : 160);   // 5 workgroups per CU of the scatter's LDS
        const u32 per_xcd_h = (u32)((nbmax + 7) / 8 < 512 ? (nbmax + 7) / 8 : 512);
        // the scan of a pass's histogram: one workgroup per view over the view's live block (16,384 entries = 64 chunks a round) while
        // a view of average size -- by the capacity, which is all the host knows -- takes at most 8 rounds; otherwise (few views of
        // very many instances) the general scan over the whole cleared table, whose zero tail also yields the end of the last digit
        const bool tile_view_scan = nbmax <= (size_t)512 * (size_t)V;
        // two passes (257..65,536 tiles: 512^2 images have 1,024): the tile bits are split EVENLY, 5 + 5 instead of 8 + 2 -- a pass costs
        // the same whatever its digit width, and a chunk's runs of equal digits, which leave LDS as coalesced stores, are 8 x longer
        // with 32 digits than with 256
        const int split = passes == 2 ? (tile_bits + 1) / 2 : 8;
        for (int p = 0; p < passes; p++) {
            const int shift = split * p;
            const u32 mask = passes == 2 ? (1u << (p == 0 ? split : tile_bits - split)) - 1u : 255u;
            if (!tile_view_scan) F3DG_HIP_CHECK(hipMemsetAsync(hist, 0, sizeof(u32) * 256 * nbmax, s));
            F3DG_KLAUNCH((radix2_hist_var_kernel<G>), dim3(8 * per_xcd_h), dim3(F3DG_BLOCK), 0, s, kgrp[src], st, shift, mask, hist);
            if (tile_view_scan)
                F3DG_KLAUNCH(tile_scan_kernel, dim3(V), dim3(1024), 0, s, (u32)V, st.vstart, st.bglob, hist);
            else {
                rc = f3dg_launch_scan_inclusive(s, hist, hist, (unsigned long long)256 * nbmax, scan_tmp, L.scan_tmp_elems, 1, nullptr);
                if (rc != F3DG_OK) return rc;
            }
            // (a single pass: the group stream is not needed again, the ranges come from the scanned histogram)
            F3DG_KLAUNCH((radix2_scatter_var_kernel<G>), dim3(8 * per_xcd), dim3(F3DG_BLOCK), 0, s, kgrp[src], vals[src],
                               passes == 1 ? (G*)nullptr : kgrp[src ^ 1], vals[src ^ 1], st, shift, mask, hist);
            src ^= 1;
        }
        if (passes == 1) {
            const u32 nseg = (u32)V * (u32)T;
            F3DG_KLAUNCH(ranges_from_offsets_kernel, dim3((nseg + F3DG_BLOCK - 1) / F3DG_BLOCK), dim3(F3DG_BLOCK), 0, s, (u32)V, (u32)T, tile_bits,
                               segtab + (V + 1), hist, hdr, reinterpret_cast<uint2*>(ws + L.ranges));
            F3DG_HIP_CHECK(hipGetLastError());
            return F3DG_OK;
        }
    }
    // 4. identifyTileRanges on the final list
    F3DG_HIP_CHECK(hipMemsetAsync(ws + L.ranges, 0, sizeof(uint2) * (size_t)V * T, s));
    F3DG_KLAUNCH((group_bounds_kernel<G>), dim3(2048), dim3(F3DG_BLOCK), 0, s, kgrp[0], hdr, tile_bits, T, reinterpret_cast<u32*>(ws + L.ranges));
    F3DG_HIP_CHECK(hipGetLastError());
    return F3DG_OK;
}

int f3dg_launch_binning(hipStream_t s, int V, int P, int W, int H, const F3dgLayout& L, char* ws, int export_offsets)
{
    const int grid_x = (W + F3DG_TILE - 1) / F3DG_TILE, grid_y = (H + F3DG_TILE - 1) / F3DG_TILE;
    const int T = grid_x * grid_y;
    const int tile_bits = f3dg_tile_bits(T);
    F3dgHeader* hdr = reinterpret_cast<F3dgHeader*>(ws + L.header);

    int rc = F3DG_OK;
    if (export_offsets) {
        // the (view, Gaussian)-ordered prefix sum of the reference (point_offsets) is only an exported intermediate here
        rc = f3dg_launch_scan_inclusive(s, reinterpret_cast<const u32*>(ws + L.tiles), reinterpret_cast<u32*>(ws + L.offsets),
                                        (unsigned long long)V * P, reinterpret_cast<u32*>(ws + L.scan_tmp), L.scan_tmp_elems, 0, nullptr);
        if (rc != F3DG_OK) return rc;
    }
    // group stream type that fits (view << tile_bits | tile)
    const bool small = (((unsigned long long)(V > 0 ? V - 1 : 0) << tile_bits) | ((1ull << tile_bits) - 1ull)) <= 0xFFFFull;
    rc = small ? binning_tail<unsigned short>(s, V, P, grid_x, T, tile_bits, L, ws, hdr)
               : binning_tail<u32>(s, V, P, grid_x, T, tile_bits, L, ws, hdr);
    if (rc != F3DG_OK) return rc;
    F3DG_HIP_CHECK(hipGetLastError());
    return F3DG_OK;
}

// debug export: rebuild the reference's 64-bit sort keys of the final list into the workspace's key region (half 0)
int f3dg_launch_export_keys(hipStream_t s, int V, int P, int W, int H, const F3dgLayout& L, char* ws)
{
    const int grid_x = (W + F3DG_TILE - 1) / F3DG_TILE, grid_y = (H + F3DG_TILE - 1) / F3DG_TILE;
    const int T = grid_x * grid_y;
    const u32 nseg = (u32)V * (u32)T;
    const u32 rg = nseg < 65535u * 4u ? nseg : 65535u * 4u;
    F3DG_KLAUNCH(export_keys_kernel, dim3(rg), dim3(F3DG_BLOCK), 0, s, nseg, P, f3dg_tile_bits(T), T,
                       reinterpret_cast<const uint2*>(ws + L.ranges), reinterpret_cast<const F3dgHeader*>(ws + L.header),
                       reinterpret_cast<const u32*>(ws + L.vals[0]), reinterpret_cast<const float*>(ws + L.depths),
                       reinterpret_cast<u64*>(ws + L.keys[0]));
    F3DG_HIP_CHECK(hipGetLastError());
    return F3DG_OK;
}
