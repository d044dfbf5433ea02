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
// Sums: every tile writes its three partial sums to its own slot of a caller-provided buffer (pairwise tree in LDS, fixed order), and
// ssim_plane_sums_kernel adds the slots of ONE plane in a fixed order: no float atomics, bit-reproducible, and no plane's sums ever see
// another plane's data.
#include "f3dg_common.h"
#include "f3dg_ssim_tile.h"

namespace {

struct SsimGrid { unsigned tiles_x, tiles_y; };

__device__ __forceinline__ SsimTile ssim_tile_of_block(unsigned block, SsimGrid grid, int W, int H, unsigned& plane, unsigned& tile)
{
    const unsigned per_plane = grid.tiles_x * grid.tiles_y;
    plane = block / per_plane;
    tile = block - plane * per_plane;
    SsimTile t;
    t.W = W; t.H = H;
    t.y0 = (int)(tile / grid.tiles_x) * F3DG_SSIM_TH;
    t.x0 = (int)(tile % grid.tiles_x) * F3DG_SSIM_TW;
    t.plane_off = (size_t)plane * (size_t)H * (size_t)W;
    return t;
}

__global__ void __launch_bounds__(F3DG_SSIM_THREADS)
ssim_fwd_kernel(SsimGrid grid, int W, int H, const float* __restrict__ img1, const float* __restrict__ img2, float* __restrict__ map,
                float* __restrict__ dm_dmu1, float* __restrict__ dm_dsigma1_sq, float* __restrict__ dm_dsigma12, float* __restrict__ partials)
{
    __shared__ float s_a[F3DG_SSIM_STAGE], s_b[F3DG_SSIM_STAGE];
    __shared__ float s_h[5 * F3DG_SSIM_HROWS];
    __shared__ float s_red[3 * F3DG_SSIM_THREADS];
    const int tid = threadIdx.x;
    unsigned plane, tile;
    const SsimTile t = ssim_tile_of_block(blockIdx.x, grid, W, H, plane, tile);
    ssim_fwd_stage(t, img1, img2, s_a, s_b, tid);
    __syncthreads();
    ssim_fwd_hpass(s_a, s_b, s_h, tid);
    __syncthreads();
    ssim_fwd_vpass(t, s_a, s_b, s_h, map, dm_dmu1, dm_dsigma1_sq, dm_dsigma12, s_red, tid);
    if (!partials) return;                      // (uniform: a kernel argument)
    for (int half = F3DG_SSIM_THREADS / 2; half >= 1; half >>= 1) {
        __syncthreads();
        ssim_reduce_level(s_red, half, tid);
    }
    if (tid == 0) {
        float* out = partials + 3 * (size_t)blockIdx.x;        // [plane][tile][3]
        out[0] = s_red[0];
        out[1] = s_red[F3DG_SSIM_THREADS];
        out[2] = s_red[2 * F3DG_SSIM_THREADS];
    }
}

// Second stage: one wave per plane adds that plane's tile slots -- lane l takes tiles l, l + 64, ... in ascending order, then a
// pairwise tree over the 64 lanes in LDS. plane_sums [n_planes][3] = sum of m, of |a - b|, of (a - b)^2.
__global__ void __launch_bounds__(64)
ssim_plane_sums_kernel(unsigned tiles_per_plane, const float* __restrict__ partials, float* __restrict__ plane_sums)
{
    __shared__ float s[3 * 64];
    const unsigned lane = threadIdx.x, plane = blockIdx.x;
    const float* p = partials + 3 * (size_t)plane * tiles_per_plane;
    float acc[3] = { 0.0f, 0.0f, 0.0f };
    for (unsigned i = lane; i < tiles_per_plane; i += 64u) {
        acc[0] = acc[0] + p[3 * (size_t)i];
        acc[1] = acc[1] + p[3 * (size_t)i + 1];
        acc[2] = acc[2] + p[3 * (size_t)i + 2];
    }
    for (int q = 0; q < 3; q++) s[q * 64 + lane] = acc[q];
    for (unsigned half = 32u; half >= 1u; half >>= 1) {
        __syncthreads();
        if (lane < half)
            for (int q = 0; q < 3; q++) s[q * 64 + lane] = s[q * 64 + lane] + s[q * 64 + lane + half];
    }
    if (lane == 0)
        for (int q = 0; q < 3; q++) plane_sums[3 * (size_t)plane + q] = s[q * 64];
}

__global__ void __launch_bounds__(F3DG_SSIM_THREADS)
ssim_bwd_kernel(SsimGrid grid, int W, int H, const float* __restrict__ img1, const float* __restrict__ img2,
                const float* __restrict__ dL_dmap, const float* __restrict__ plane_weights, const float* __restrict__ dm_dmu1,
                const float* __restrict__ dm_dsigma1_sq, const float* __restrict__ dm_dsigma12, float* __restrict__ dL_dimg1)
{
    __shared__ float s_x[3 * F3DG_SSIM_STAGE];
    __shared__ float s_h[3 * F3DG_SSIM_HROWS];
    const int tid = threadIdx.x;
    unsigned plane, tile;
    const SsimTile t = ssim_tile_of_block(blockIdx.x, grid, W, H, plane, tile);
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

// tiles of one plane and workgroups of the call; false when the sizes are not positive or the grid does not fit 31 bits
bool ssim_grid(int n_planes, int W, int H, SsimGrid& g, unsigned long long& blocks)
{
    if (n_planes <= 0 || W <= 0 || H <= 0) return false;
    g.tiles_x = ((unsigned)W + F3DG_SSIM_TW - 1u) / F3DG_SSIM_TW;
    g.tiles_y = ((unsigned)H + F3DG_SSIM_TH - 1u) / F3DG_SSIM_TH;
    blocks = (unsigned long long)g.tiles_x * g.tiles_y * (unsigned long long)n_planes;
    return blocks <= 0x7FFFFFFFull;
}

} // namespace

extern "C" size_t f3dg_ssim_partials_bytes(int n_planes, int W, int H)
{
    SsimGrid g;
    unsigned long long blocks;
    if (!ssim_grid(n_planes, W, H, g, blocks)) return 0;
    return (size_t)blocks * 3 * sizeof(float);
}

extern "C" int f3dg_ssim_forward(void* stream, int n_planes, int W, int H, const float* img1, const float* img2, float* map,
                                 float* dm_dmu1, float* dm_dsigma1_sq, float* dm_dsigma12, float* partials, size_t partials_bytes,
                                 float* plane_sums)
{
    if (n_planes <= 0 || W <= 0 || H <= 0 || !img1 || !img2) return F3DG_ERR_BAD_ARG;
    if (plane_sums && !partials) return F3DG_ERR_BAD_ARG;
    SsimGrid g;
    unsigned long long blocks;
    if (!ssim_grid(n_planes, W, H, g, blocks)) return F3DG_ERR_UNSUPPORTED;
    if (partials && partials_bytes < (size_t)blocks * 3 * sizeof(float)) return F3DG_ERR_WORKSPACE;
    if (!map && !dm_dmu1 && !dm_dsigma1_sq && !dm_dsigma12 && !partials) return F3DG_OK;
    F3DG_KLAUNCH(ssim_fwd_kernel, dim3((unsigned)blocks), dim3(F3DG_SSIM_THREADS), 0, (hipStream_t)stream, g, W, H, img1, img2, map,
                 dm_dmu1, dm_dsigma1_sq, dm_dsigma12, partials);
    F3DG_HIP_CHECK(hipGetLastError());
    if (plane_sums) {
        F3DG_KLAUNCH(ssim_plane_sums_kernel, dim3((unsigned)n_planes), dim3(64), 0, (hipStream_t)stream, g.tiles_x * g.tiles_y, partials,
                     plane_sums);
        F3DG_HIP_CHECK(hipGetLastError());
    }
    return F3DG_OK;
}

extern "C" int f3dg_ssim_backward(void* stream, int n_planes, int W, int H, const float* img1, const float* img2, const float* dL_dmap,
                                  const float* plane_weights, const float* dm_dmu1, const float* dm_dsigma1_sq, const float* dm_dsigma12,
                                  float* dL_dimg1)
{
    if (n_planes <= 0 || W <= 0 || H <= 0 || !img1 || !img2 || !dm_dmu1 || !dm_dsigma1_sq || !dm_dsigma12 || !dL_dimg1)
        return F3DG_ERR_BAD_ARG;
    if (!dL_dmap && !plane_weights) return F3DG_ERR_BAD_ARG;
    SsimGrid g;
    unsigned long long blocks;
    if (!ssim_grid(n_planes, W, H, g, blocks)) return F3DG_ERR_UNSUPPORTED;
    F3DG_KLAUNCH(ssim_bwd_kernel, dim3((unsigned)blocks), dim3(F3DG_SSIM_THREADS), 0, (hipStream_t)stream, g, W, H, img1, img2, dL_dmap,
                 plane_weights, dm_dmu1, dm_dsigma1_sq, dm_dsigma12, dL_dimg1);
    F3DG_HIP_CHECK(hipGetLastError());
    return F3DG_OK;
}
