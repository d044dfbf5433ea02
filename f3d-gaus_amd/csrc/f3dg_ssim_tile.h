// f3dg_ssim_tile.h -- the per-workgroup phases of the fused image loss (f3dg_ssim.hip): staging, horizontal pass, vertical pass of the
// forward and of the backward, each a function of the thread index that touches only the workgroup's LDS arrays and its own tile of
// global memory. The kernels call them with a workgroup barrier between two phases; nothing else is in between, so the phases can be
// read (and exercised on a host, one "thread" after the other) on their own.
//
// Definition (include/f3dg.h has the contract): G is the reference's 11-tap Gaussian window (utils/loss_utils.py:23-31, sigma 1.5) applied
// separably to the image zero-padded by 5; m = (2 mu1 mu2 + C1)(2 s12 + C2) / ((mu1^2 + mu2^2 + C1)(s1 + s2 + C2)), utils/loss_utils.py:43-58.
// Compiled with -ffp-contract=off like the rest of the library: every product and sum below is one float32 rounding.
#pragma once
#include "f3dg_tile_sums.h"                          // the tile: 32 wide (one LDS lane group per tile row), 16 high, 256 threads

#define F3DG_SSIM_R 5                                // window radius
#define F3DG_SSIM_SW (F3DG_TILE_W + 2 * F3DG_SSIM_R)    // 42 staged columns
#define F3DG_SSIM_SH (F3DG_TILE_H + 2 * F3DG_SSIM_R)    // 26 staged rows
#define F3DG_SSIM_STAGE (F3DG_SSIM_SH * F3DG_SSIM_SW)    // 1,092 floats per staged plane
#define F3DG_SSIM_HROWS (F3DG_SSIM_SH * F3DG_TILE_W)    // 832 floats per horizontally blurred plane

// The reference's taps: float32(exp(-(i - 5)^2 / 4.5)) over their float32 sum (torch.Tensor(...) / .sum()), i = 0..10.
#define F3DG_SSIM_TAPS { 0x1.0d956cp-10f, 0x1.f1fe02p-8f, 0x1.26eb18p-5f, 0x1.bff0fep-4f, 0x1.b43c3ep-3f, 0x1.10656p-2f, \
                         0x1.b43c3ep-3f, 0x1.bff0fep-4f, 0x1.26eb18p-5f, 0x1.f1fe02p-8f, 0x1.0d956cp-10f }
#define F3DG_SSIM_C1 0.0001f                         // float32(0.01 ** 2)
#define F3DG_SSIM_C2 0.0009f                         // float32(0.03 ** 2)

struct SsimTile {
    int W, H;                   // image size
    int x0, y0;                 // first pixel of the tile
    size_t plane_off;           // plane * H * W
};

// ------------------------------------------------------------------------------------------------ forward
// Phase 1: both images' (TH + 10) x (TW + 10) neighbourhood into LDS, zero outside the image (the reference's padding = 5).
__device__ __forceinline__ void ssim_fwd_stage(const SsimTile& t, const float* __restrict__ img1, const float* __restrict__ img2,
                                               float* s_a, float* s_b, int tid)
{
    for (int i = tid; i < F3DG_SSIM_STAGE; i += F3DG_TILE_THREADS) {
        const int r = i / F3DG_SSIM_SW, c = i - r * F3DG_SSIM_SW;
        const int y = t.y0 - F3DG_SSIM_R + r, x = t.x0 - F3DG_SSIM_R + c;
        float a = 0.0f, b = 0.0f;
        if (x >= 0 && x < t.W && y >= 0 && y < t.H) {
            const size_t idx = t.plane_off + (size_t)y * t.W + x;
            a = img1[idx];
            b = img2[idx];
        }
        s_a[i] = a;
        s_b[i] = b;
    }
}

// Phase 2: the 11 horizontal taps of a, b, a a, b b, a b for every staged row: s_h[q][row * TW + column].
__device__ __forceinline__ void ssim_fwd_hpass(const float* s_a, const float* s_b, float* s_h, int tid)
{
    const float g[11] = F3DG_SSIM_TAPS;
    for (int i = tid; i < F3DG_SSIM_HROWS; i += F3DG_TILE_THREADS) {
        const int r = i / F3DG_TILE_W, c = i - r * F3DG_TILE_W;
        const float* pa = s_a + r * F3DG_SSIM_SW + c;
        const float* pb = s_b + r * F3DG_SSIM_SW + c;
        float m1 = 0.0f, m2 = 0.0f, e11 = 0.0f, e22 = 0.0f, e12 = 0.0f;
#pragma unroll
        for (int k = 0; k < 11; k++) {
            const float a = pa[k], b = pb[k];
            m1 = m1 + g[k] * a;
            m2 = m2 + g[k] * b;
            e11 = e11 + g[k] * (a * a);
            e22 = e22 + g[k] * (b * b);
            e12 = e12 + g[k] * (a * b);
        }
        s_h[0 * F3DG_SSIM_HROWS + i] = m1;
        s_h[1 * F3DG_SSIM_HROWS + i] = m2;
        s_h[2 * F3DG_SSIM_HROWS + i] = e11;
        s_h[3 * F3DG_SSIM_HROWS + i] = e22;
        s_h[4 * F3DG_SSIM_HROWS + i] = e12;
    }
}

// The map and its three partial derivatives from the five windowed moments. dm_dmu1 is the derivative with G*(a a) and G*(a b) held
// fixed (it carries the -2 mu1 of sigma1^2 and the -mu2 of sigma12), which is what the backward's three blurs need.
struct SsimPoint { float m, dm_dmu1, dm_dsigma1_sq, dm_dsigma12; };
__device__ __forceinline__ SsimPoint ssim_point(float mu1, float mu2, float e11, float e22, float e12)
{
    const float mu1_sq = mu1 * mu1, mu2_sq = mu2 * mu2, mu1_mu2 = mu1 * mu2;
    const float s1 = e11 - mu1_sq, s2 = e22 - mu2_sq, s12 = e12 - mu1_mu2;
    const float A1 = 2.0f * mu1_mu2 + F3DG_SSIM_C1, A2 = 2.0f * s12 + F3DG_SSIM_C2;
    const float B1 = (mu1_sq + mu2_sq) + F3DG_SSIM_C1, B2 = (s1 + s2) + F3DG_SSIM_C2;
    const float den = B1 * B2;
    SsimPoint p;
    p.m = (A1 * A2) / den;
    p.dm_dmu1 = (2.0f * mu2 * (A2 - A1) - 2.0f * mu1 * p.m * (B2 - B1)) / den;
    p.dm_dsigma1_sq = -p.m / B2;
    p.dm_dsigma12 = (2.0f * A1) / den;
    return p;
}

// Phase 3: the 11 vertical taps, the map, the derivative planes (each pointer may be null) and this thread's share of the tile sums:
// red[0 / 1 / 2][tid] = sum of m, |a - b|, (a - b)^2 over its (up to two) pixels inside the image, in row order.
__device__ __forceinline__ void ssim_fwd_vpass(const SsimTile& t, const float* s_a, const float* s_b, const float* s_h,
                                               float* __restrict__ map, float* __restrict__ dm_dmu1, float* __restrict__ dm_dsigma1_sq,
                                               float* __restrict__ dm_dsigma12, float* red, int tid)
{
    const float g[11] = F3DG_SSIM_TAPS;
    int tx, ty0;
    tile_thread(tid, tx, ty0);
    float sum_m = 0.0f, sum_l1 = 0.0f, sum_l2 = 0.0f;
#pragma unroll
    for (int j = 0; j < F3DG_TILE_H / F3DG_TILE_ROWS; j++) {
        const int ty = ty0 + j * F3DG_TILE_ROWS;
        float v[5];
#pragma unroll
        for (int q = 0; q < 5; q++) {
            const float* p = s_h + q * F3DG_SSIM_HROWS + ty * F3DG_TILE_W + tx;
            float acc = 0.0f;
#pragma unroll
            for (int k = 0; k < 11; k++) acc = acc + g[k] * p[k * F3DG_TILE_W];
            v[q] = acc;
        }
        const int x = t.x0 + tx, y = t.y0 + ty;
        if (x < t.W && y < t.H) {
            const SsimPoint p = ssim_point(v[0], v[1], v[2], v[3], v[4]);
            const size_t idx = t.plane_off + (size_t)y * t.W + x;
            if (map) map[idx] = p.m;
            if (dm_dmu1) dm_dmu1[idx] = p.dm_dmu1;
            if (dm_dsigma1_sq) dm_dsigma1_sq[idx] = p.dm_dsigma1_sq;
            if (dm_dsigma12) dm_dsigma12[idx] = p.dm_dsigma12;
            const int c = (ty + F3DG_SSIM_R) * F3DG_SSIM_SW + tx + F3DG_SSIM_R;
            const float d = s_a[c] - s_b[c];
            sum_m = sum_m + p.m;
            sum_l1 = sum_l1 + fabsf(d);
            sum_l2 = sum_l2 + d * d;
        }
    }
    red[0 * F3DG_TILE_THREADS + tid] = sum_m;
    red[1 * F3DG_TILE_THREADS + tid] = sum_l1;
    red[2 * F3DG_TILE_THREADS + tid] = sum_l2;
}

// ------------------------------------------------------------------------------------------------ backward
// dL/da(p) = sum_q g(q - p) [ w(q) dm_dmu1(q) + 2 a(p) w(q) dm_dsigma1_sq(q) + b(p) w(q) dm_dsigma12(q) ]
//            + w_l1 sign(a - b)(p) + 2 w_l2 (a - b)(p),       w(q) = dL_dmap(q) + w_ssim of the plane
// Phase 1: the three products over the tile's neighbourhood into LDS, zero outside the image (no pixel there has a map value).
__device__ __forceinline__ void ssim_bwd_stage(const SsimTile& t, const float* __restrict__ dL_dmap, float w_ssim,
                                               const float* __restrict__ dm_dmu1, const float* __restrict__ dm_dsigma1_sq,
                                               const float* __restrict__ dm_dsigma12, float* s_x, int tid)
{
    for (int i = tid; i < F3DG_SSIM_STAGE; i += F3DG_TILE_THREADS) {
        const int r = i / F3DG_SSIM_SW, c = i - r * F3DG_SSIM_SW;
        const int y = t.y0 - F3DG_SSIM_R + r, x = t.x0 - F3DG_SSIM_R + c;
        float x1 = 0.0f, x2 = 0.0f, x3 = 0.0f;
        if (x >= 0 && x < t.W && y >= 0 && y < t.H) {
            const size_t idx = t.plane_off + (size_t)y * t.W + x;
            const float w = dL_dmap ? dL_dmap[idx] + w_ssim : w_ssim;
            x1 = w * dm_dmu1[idx];
            x2 = w * dm_dsigma1_sq[idx];
            x3 = w * dm_dsigma12[idx];
        }
        s_x[0 * F3DG_SSIM_STAGE + i] = x1;
        s_x[1 * F3DG_SSIM_STAGE + i] = x2;
        s_x[2 * F3DG_SSIM_STAGE + i] = x3;
    }
}

// Phase 2: the horizontal taps of the three products.
__device__ __forceinline__ void ssim_bwd_hpass(const float* s_x, float* s_h, int tid)
{
    const float g[11] = F3DG_SSIM_TAPS;
    for (int i = tid; i < F3DG_SSIM_HROWS; i += F3DG_TILE_THREADS) {
        const int r = i / F3DG_TILE_W, c = i - r * F3DG_TILE_W;
#pragma unroll
        for (int q = 0; q < 3; q++) {
            const float* p = s_x + q * F3DG_SSIM_STAGE + r * F3DG_SSIM_SW + c;
            float acc = 0.0f;
#pragma unroll
            for (int k = 0; k < 11; k++) acc = acc + g[k] * p[k];
            s_h[q * F3DG_SSIM_HROWS + i] = acc;
        }
    }
}

// Phase 3: the vertical taps, the chain rule through a a and a b at the pixel itself, and the L1 / L2 terms (sign(0) = 0, as
// torch.abs's gradient).
__device__ __forceinline__ void ssim_bwd_vpass(const SsimTile& t, const float* s_h, const float* __restrict__ img1,
                                               const float* __restrict__ img2, float w_l1, float w_l2, float* __restrict__ dL_dimg1, int tid)
{
    const float g[11] = F3DG_SSIM_TAPS;
    int tx, ty0;
    tile_thread(tid, tx, ty0);
#pragma unroll
    for (int j = 0; j < F3DG_TILE_H / F3DG_TILE_ROWS; j++) {
        const int ty = ty0 + j * F3DG_TILE_ROWS;
        const int x = t.x0 + tx, y = t.y0 + ty;
        if (!(x < t.W && y < t.H)) continue;
        float v[3];
#pragma unroll
        for (int q = 0; q < 3; q++) {
            const float* p = s_h + q * F3DG_SSIM_HROWS + ty * F3DG_TILE_W + tx;
            float acc = 0.0f;
#pragma unroll
            for (int k = 0; k < 11; k++) acc = acc + g[k] * p[k * F3DG_TILE_W];
            v[q] = acc;
        }
        const size_t idx = t.plane_off + (size_t)y * t.W + x;
        const float a = img1[idx], b = img2[idx];
        const float d = a - b;
        const float sgn = d > 0.0f ? 1.0f : (d < 0.0f ? -1.0f : 0.0f);
        float grad = (v[0] + (2.0f * a) * v[1]) + b * v[2];
        grad = grad + w_l1 * sgn;
        grad = grad + (2.0f * w_l2) * d;
        dL_dimg1[idx] = grad;
    }
}
