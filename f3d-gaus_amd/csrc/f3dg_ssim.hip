// f3dg_ssim.hip -- fused differentiable image loss: SSIM map, its per-plane mean, and the L1 / L2 sums of a batch of frames in ONE
// forward kernel (plus a tiny fixed-order second-stage sum), and dL/dimg1 of all three in ONE backward kernel.
//
// Replaces, for the objective (1 - lambda) L1 + lambda (1 - SSIM) of the reference's trainer (train.py:92, utils/loss_utils.py:33-63) and
// the per-frame metrics of metrics.py:72, five depthwise 11 x 11 conv2d calls, ~20 elementwise kernels and their autograd graph.
//
// A plane is one H x W channel of one frame; a workgroup of 256 threads (4 wave64) owns a 32 x 16 pixel tile of one plane:
//   forward   stage a, b with a 5-pixel halo (2 x 26 x 42 floats)  ->  horizontal taps of a, b, aa, bb, ab (5 x 26 x 32)  ->  vertical
//             taps, the map, the three derivative planes, and the tile's sums of m, |a - b|, (a - b)^2 from the interior still in LDS
//   backward  stage w dm/dmu1, w dm/dsigma1^2, w dm/dsigma12 with the halo (3 x 26 x 42)  ->  horizontal taps (3 x 26 x 32)  ->  vertical
//             taps and the per-pixel chain rule
// The phases are in f3dg_ssim_tile.h. Every LDS access of a wave is two 32-lane groups that each read or write 32 consecutive dwords of
// one tile row (the tile is exactly one lane group wide), so no access has a bank conflict whatever the row stride is: the vertical
// pass needs no padding. LDS per workgroup: forward 28,448 B (5 workgroups = 20 waves per CU), backward 23,088 B (7 = 28 waves).
//
// Sums: the two-stage, fixed-order scheme of f3dg_tile_sums.h with TERMS = 3 (m, |a - b|, (a - b)^2) and a plane as its frame.
#include "f3dg_common.h"
#include "f3dg_ssim_tile.h"
#include "f3dg_tile_sums.h"

namespace {

__device__ __forceinline__ SsimTile ssim_tile(const TileOfBlock& b, int W, int H)
{
    SsimTile t;
    t.W = W; t.H = H;
    t.y0 = b.y0;
    t.x0 = b.x0;
    t.plane_off = (size_t)b.frame * (size_t)H * (size_t)W;
    return t;
}

__global__ void __launch_bounds__(F3DG_TILE_THREADS)
ssim_fwd_kernel(TileGrid grid, int W, int H, const float* __restrict__ img1, const float* __restrict__ img2, float* __restrict__ map,
                float* __restrict__ dm_dmu1, float* __restrict__ dm_dsigma1_sq, float* __restrict__ dm_dsigma12, float* __restrict__ partials)
{
    __shared__ float s_a[F3DG_SSIM_STAGE], s_b[F3DG_SSIM_STAGE];
    __shared__ float s_h[5 * F3DG_SSIM_HROWS];
    __shared__ float s_red[3 * F3DG_TILE_THREADS];
    const int tid = threadIdx.x;
    const SsimTile t = ssim_tile(tile_of_block(grid), W, H);
    ssim_fwd_stage(t, img1, img2, s_a, s_b, tid);
    __syncthreads();
    ssim_fwd_hpass(s_a, s_b, s_h, tid);
    __syncthreads();
    ssim_fwd_vpass(t, s_a, s_b, s_h, map, dm_dmu1, dm_dsigma1_sq, dm_dsigma12, s_red, tid);
    if (!partials) return;                      // (uniform: a kernel argument)
    tile_sums_reduce<3>(s_red, tid, partials);
}

__global__ void __launch_bounds__(F3DG_TILE_THREADS)
ssim_bwd_kernel(TileGrid grid, int W, int H, const float* __restrict__ img1, const float* __restrict__ img2,
                const float* __restrict__ dL_dmap, const float* __restrict__ plane_weights, const float* __restrict__ dm_dmu1,
                const float* __restrict__ dm_dsigma1_sq, const float* __restrict__ dm_dsigma12, float* __restrict__ dL_dimg1)
{
    __shared__ float s_x[3 * F3DG_SSIM_STAGE];
    __shared__ float s_h[3 * F3DG_SSIM_HROWS];
    const int tid = threadIdx.x;
    const TileOfBlock b = tile_of_block(grid);
    const unsigned plane = b.frame;
    const SsimTile t = ssim_tile(b, W, H);
    float w_ssim = 0.0f, w_l1 = 0.0f, w_l2 = 0.0f;
    if (plane_weights) {
        w_ssim = plane_weights[3 * (size_t)plane];
        w_l1 = plane_weights[3 * (size_t)plane + 1];
        w_l2 = plane_weights[3 * (size_t)plane + 2];
    }
    ssim_bwd_stage(t, dL_dmap, w_ssim, dm_dmu1, dm_dsigma1_sq, dm_dsigma12, s_x, tid);
    __syncthreads();
    ssim_bwd_hpass(s_x, s_h, tid);
    __syncthreads();
    ssim_bwd_vpass(t, s_h, img1, img2, w_l1, w_l2, dL_dimg1, tid);
}

} // namespace

extern "C" size_t f3dg_ssim_partials_bytes(int n_planes, int W, int H)
{
    return tile_partials_bytes<3>(n_planes, W, H, 0);
}

extern "C" int f3dg_ssim_forward(void* stream, int n_planes, int W, int H, const float* img1, const float* img2, float* map,
                                 float* dm_dmu1, float* dm_dsigma1_sq, float* dm_dsigma12, float* partials, size_t partials_bytes,
                                 float* plane_sums)
{
    if (n_planes <= 0 || W <= 0 || H <= 0 || !img1 || !img2) return F3DG_ERR_BAD_ARG;
    if (plane_sums && !partials) return F3DG_ERR_BAD_ARG;
    TileGrid g;
    unsigned blocks;
    if (!tile_grid(n_planes, W, H, 0, g, blocks)) return F3DG_ERR_UNSUPPORTED;
    if (partials && partials_bytes < tile_partials_bytes<3>(blocks)) return F3DG_ERR_WORKSPACE;
    if (!map && !dm_dmu1 && !dm_dsigma1_sq && !dm_dsigma12 && !partials) return F3DG_OK;
    F3DG_KLAUNCH(ssim_fwd_kernel, dim3(blocks), dim3(F3DG_TILE_THREADS), 0, (hipStream_t)stream, g, W, H, img1, img2, map,
                 dm_dmu1, dm_dsigma1_sq, dm_dsigma12, partials);
    F3DG_HIP_CHECK(hipGetLastError());
    return plane_sums ? tile_frame_sums<3>((hipStream_t)stream, n_planes, g, partials, plane_sums) : F3DG_OK;
}

extern "C" int f3dg_ssim_backward(void* stream, int n_planes, int W, int H, const float* img1, const float* img2, const float* dL_dmap,
                                  const float* plane_weights, const float* dm_dmu1, const float* dm_dsigma1_sq, const float* dm_dsigma12,
                                  float* dL_dimg1)
{
    if (n_planes <= 0 || W <= 0 || H <= 0 || !img1 || !img2 || !dm_dmu1 || !dm_dsigma1_sq || !dm_dsigma12 || !dL_dimg1)
        return F3DG_ERR_BAD_ARG;
    if (!dL_dmap && !plane_weights) return F3DG_ERR_BAD_ARG;
    TileGrid g;
    unsigned blocks;
    if (!tile_grid(n_planes, W, H, 0, g, blocks)) return F3DG_ERR_UNSUPPORTED;
    F3DG_KLAUNCH(ssim_bwd_kernel, dim3(blocks), dim3(F3DG_TILE_THREADS), 0, (hipStream_t)stream, g, W, H, img1, img2, dL_dmap,
                 plane_weights, dm_dmu1, dm_dsigma1_sq, dm_dsigma12, dL_dimg1);
    F3DG_HIP_CHECK(hipGetLastError());
    return F3DG_OK;
}
