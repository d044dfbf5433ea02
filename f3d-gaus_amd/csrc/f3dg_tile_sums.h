// f3dg_tile_sums.h -- the per-frame sums of the loss kernels (f3dg_ssim.hip, f3dg_geometry_loss.hip, the masked L1 of f3dg_warp.hip):
// TERMS float32 sums over the pixels of every frame (SSIM: plane) of a call, in two stages and in ONE fixed order. No float atomics,
// so the sums are bit-reproducible, and a frame's sums read no other frame's data. The order is part of the contract
// (include/f3dg.h); tests/tile_sums_truth.py restates it and tests/test_tile_sums_gpu.py holds the kernels to its bits.
//
//   tiles     a frame is cut into tiles F3DG_TILE_W = 32 wide and F3DG_TILE_H = 16 high, row-major; one workgroup of 256 threads per
//             (frame, tile), blockIdx.x = frame * tiles_per_frame + tile.
//   thread    tid covers column tid % 32 of the tile in row tid / 32 and in the row F3DG_TILE_ROWS = 8 below it. Its TERMS running sums
//             start at 0.0f and take the first row's pixel, then the second's; a pixel outside the image is skipped. What a pixel adds,
//             and in which order inside the pixel (the masked L1: channels ascending), is the kernel's business.
//   tile      the 256 thread sums of a term lie in s_red[term][tid] (LDS); the tree s[i] += s[i + half] for i < half, half = 128 ... 1,
//             leaves the tile's sum in s[0], and thread 0 stores the TERMS sums in the tile's slot partials[frame][tile][TERMS].
//   frame     f3dg_frame_sums_kernel: one wave per frame; lane l starts at 0.0f and adds the slots of tiles l, l + 64, ... in ascending
//             order, then the same tree over the 64 lanes, half = 32 ... 1, and lane 0 stores frame_sums[frame][TERMS].
//
// Barriers: tile_sums_reduce holds one __syncthreads() in front of every level of its tree -- the first also orders the writes to s_red
// before the reads -- so EVERY thread of the workgroup must reach the call, also a thread with no pixel inside the image (its sums are 0).
//
// The backward kernels of the geometry terms and of the masked L1 share a plainer grid, one thread per (frame, pixel) in workgroups of
// F3DG_BLOCK consecutive pixels of one frame: frame_pixel_grid / frame_pixel_of_block at the end.
#pragma once
#include "f3dg_common.h"

#define F3DG_TILE_W 32                                      // one 32-lane LDS lane group per tile row
#define F3DG_TILE_H 16                                      // two pixels per thread
#define F3DG_TILE_THREADS 256
#define F3DG_TILE_ROWS (F3DG_TILE_THREADS / F3DG_TILE_W)    // rows of a tile the threads cover at once: 8

static_assert(F3DG_TILE_H % F3DG_TILE_ROWS == 0 && (F3DG_TILE_THREADS & (F3DG_TILE_THREADS - 1)) == 0, "whole rounds of rows; a power-of-two tree");

// ------------------------------------------------------------------------------------------------ second stage
template <int TERMS>
__global__ void __launch_bounds__(64)
f3dg_frame_sums_kernel(unsigned tiles_per_frame, const float* __restrict__ partials, float* __restrict__ frame_sums)
{
    __shared__ float s[TERMS * 64];
    const unsigned lane = threadIdx.x, f = blockIdx.x;
    const float* p = partials + TERMS * (size_t)f * tiles_per_frame;
    float acc[TERMS];
    for (int q = 0; q < TERMS; q++) acc[q] = 0.0f;
    for (unsigned i = lane; i < tiles_per_frame; i += 64u)
        for (int q = 0; q < TERMS; q++) acc[q] = acc[q] + p[TERMS * (size_t)i + q];
    for (int q = 0; q < TERMS; q++) s[q * 64 + lane] = acc[q];
    for (unsigned half = 32u; half >= 1u; half >>= 1) {
        __syncthreads();
        if (lane < half)
            for (int q = 0; q < TERMS; q++) s[q * 64 + lane] = s[q * 64 + lane] + s[q * 64 + lane + half];
    }
    if (lane == 0)
        for (int q = 0; q < TERMS; q++) frame_sums[TERMS * (size_t)f + q] = s[q * 64];
}

namespace {

struct TileGrid { unsigned tiles_x, tiles_y; };             // tiles of one frame (by value to the kernels)

// ------------------------------------------------------------------------------------------------ host
// Tiles of one frame and workgroups of the call. false when a size is not positive, when frame_elements -- what a kernel indexes with an
// int inside one frame; 0 where it has no such index -- is beyond 0x7FFFFFF0, or when the grid does not fit 31 bits.
bool tile_grid(int n_frames, int W, int H, long long frame_elements, TileGrid& g, unsigned& blocks)
{
    if (n_frames <= 0 || W <= 0 || H <= 0 || frame_elements > 0x7FFFFFF0ll) return false;
    g.tiles_x = ((unsigned)W + F3DG_TILE_W - 1u) / F3DG_TILE_W;
    g.tiles_y = ((unsigned)H + F3DG_TILE_H - 1u) / F3DG_TILE_H;
    const unsigned long long n = (unsigned long long)g.tiles_x * g.tiles_y * (unsigned long long)n_frames;
    blocks = (unsigned)n;
    return n <= 0x7FFFFFFFull;
}

// bytes of `partials` for a grid of `blocks` workgroups
template <int TERMS>
size_t tile_partials_bytes(unsigned blocks) { return (size_t)blocks * TERMS * sizeof(float); }

// what the *_partials_bytes entries return: 0 where tile_grid says no
template <int TERMS>
size_t tile_partials_bytes(int n_frames, int W, int H, long long frame_elements)
{
    TileGrid g;
    unsigned blocks;
    return tile_grid(n_frames, W, H, frame_elements, g, blocks) ? tile_partials_bytes<TERMS>(blocks) : 0;
}

// the second stage on `stream`: n_frames workgroups of one wave
template <int TERMS>
int tile_frame_sums(hipStream_t stream, int n_frames, TileGrid g, const float* partials, float* frame_sums)
{
    F3DG_KLAUNCH(f3dg_frame_sums_kernel<TERMS>, dim3((unsigned)n_frames), dim3(64), 0, stream, g.tiles_x * g.tiles_y, partials, frame_sums);
    F3DG_HIP_CHECK(hipGetLastError());
    return F3DG_OK;
}

// ------------------------------------------------------------------------------------------------ device: first stage
struct TileOfBlock {
    unsigned frame, tile;       // blockIdx.x = frame * tiles_per_frame + tile
    int x0, y0;                 // first pixel of the tile
};

__device__ __forceinline__ TileOfBlock tile_of_block(TileGrid grid)
{
    const unsigned per_frame = grid.tiles_x * grid.tiles_y;
    TileOfBlock t;
    t.frame = blockIdx.x / per_frame;
    t.tile = blockIdx.x - t.frame * per_frame;
    t.x0 = (int)(t.tile % grid.tiles_x) * F3DG_TILE_W;
    t.y0 = (int)(t.tile / grid.tiles_x) * F3DG_TILE_H;
    return t;
}

// the thread's column and its first row inside the tile; round j of F3DG_TILE_H / F3DG_TILE_ROWS is row ty + j * F3DG_TILE_ROWS
__device__ __forceinline__ void tile_thread(int tid, int& tx, int& ty)
{
    tx = tid % F3DG_TILE_W;
    ty = tid / F3DG_TILE_W;
}

// s_red[TERMS * F3DG_TILE_THREADS] <- this thread's sums (the SSIM forward writes s_red itself, ssim_fwd_vpass)
template <int TERMS>
__device__ __forceinline__ void tile_sums_put(float* s_red, const float (&acc)[TERMS], int tid)
{
#pragma unroll
    for (int q = 0; q < TERMS; q++) s_red[q * F3DG_TILE_THREADS + tid] = acc[q];
}

// the tree over s_red and the store of the tile's slot. Every thread of the workgroup reaches this call.
template <int TERMS>
__device__ __forceinline__ void tile_sums_reduce(float* s_red, int tid, float* __restrict__ partials)
{
    for (int half = F3DG_TILE_THREADS / 2; half >= 1; half >>= 1) {
        __syncthreads();
        if (tid < half) {
#pragma unroll
            for (int q = 0; q < TERMS; q++)
                s_red[q * F3DG_TILE_THREADS + tid] = s_red[q * F3DG_TILE_THREADS + tid] + s_red[q * F3DG_TILE_THREADS + tid + half];
        }
    }
    if (tid == 0) {
        float* out = partials + TERMS * (size_t)blockIdx.x;        // [frame][tile][TERMS]
#pragma unroll
        for (int q = 0; q < TERMS; q++) out[q] = s_red[q * F3DG_TILE_THREADS];
    }
}

// ------------------------------------------------------------------------------------------------ the backward's pixel grid
// workgroups of F3DG_BLOCK consecutive pixels of one frame; false when the grid does not fit 31 bits
bool frame_pixel_grid(int n_frames, int H, int W, unsigned& blocks_per_frame, unsigned& blocks)
{
    const unsigned long long per_frame = ((unsigned long long)H * W + F3DG_BLOCK - 1) / F3DG_BLOCK;
    if (per_frame * (unsigned long long)n_frames > 0x7FFFFFFFull) return false;
    blocks_per_frame = (unsigned)per_frame;
    blocks = (unsigned)(per_frame * n_frames);
    return true;
}

// the thread's frame and its pixel n inside it (the caller returns where n >= H W)
__device__ __forceinline__ void frame_pixel_of_block(unsigned blocks_per_frame, unsigned& f, int& n)
{
    f = blockIdx.x / blocks_per_frame;
    n = (int)(blockIdx.x - f * blocks_per_frame) * F3DG_BLOCK + (int)threadIdx.x;
}

} // namespace
