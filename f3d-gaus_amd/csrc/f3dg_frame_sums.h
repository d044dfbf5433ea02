// f3dg_frame_sums.h -- the fixed-order second stage of the per-frame loss sums (f3dg_geometry_loss.hip, f3dg_warp.hip): the first stage
// leaves TERMS sums per tile in `partials` ([frame][tile][TERMS]); one wave per frame adds that frame's slots -- lane l takes tiles l,
// l + 64, ... in ascending order, then a pairwise tree over the 64 lanes in LDS (ssim_plane_sums_kernel with TERMS columns). No atomics:
// the sums are bit-reproducible and a frame's sums read no other frame's slots.
#pragma once
#include "f3dg_common.h"

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
