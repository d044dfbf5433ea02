// f3dg_backward.hip -- backward of the compositing stage and of the per-Gaussian projection stage.
//
// Replaces (reference RAST/cuda_rasterizer/backward.cu):
//   renderCUDA<3> (bwd)              :634-955   -> render3_bwd_kernel (and render5_bwd_kernel, f3dg_backward5.hip)
//   preprocessCUDA<3> (bwd)          :593-631   -> preprocess_bwd_kernel, with
//   computeView2Gaussian_backward    :381-587
//   computeColorFromSH (bwd)         :20-139
// The reference's computeCov2DCUDA / computeCov3D backward are commented out there (:992-1007, :627-630), so
// dL_dconic and dL_dcov3D are identically zero; they are left untouched here as well.
//
// MI355X shape of render3_bwd_kernel (option bwd_dense 0; the default is render5_bwd_kernel). The reference issues 17 float atomicAdds per
// contributing (pixel, Gaussian) pair. Here all 64 lanes of a wave walk the tile list in lock-step, so the 17 partial derivatives of one
// Gaussian (f3dg_bwd_pair.h) are first summed across the wave in float32: permlane swaps pair the values two by two (pair32, pair16) until
// every 16-lane row holds the partial sums of different values, four DPP steps finish a row (row_total), and the four row-end lanes add
// neighbouring elements to memory -- five atomic instructions per (wave, Gaussian) instead of 17 per (pixel, Gaussian), and nothing at
// all for the (wave, Gaussian) pairs no lane contributes to (a ballot). Only the accumulation of the 10 dL/dview2gaussian entries is
// float64 (global_atomic_add_f64): the per-Gaussian stage below amplifies a 5e-7 ordering perturbation of them into tens of percent on
// dL/dscale (SURVEY 0.9 -- the reference's own run-to-run spread), so float64 sums keep the order of the waves out of the result.
#include "f3dg_common.h"
#include "f3dg_ellipse.h"
#include "f3dg_quad.h"
#include "f3dg_bwd_pair.h"

namespace {

// Row-local sums on the VALU with DPP (no LDS traffic): inclusive row scans (row_shr 1, 2, 4, 8 with zero fill)
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ float dpp_f32(float v)
{
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, ROW_MASK, 0xF, true));
}
#define F3DG_DPP_ROW_SHR(n) (0x110 + (n))

// ---- transposed wave reduction of several values at once -------------------------------------------------------------
// v_permlane32_swap / v_permlane16_swap (gfx950) exchange half-waves / 16-lane rows between two registers, so ONE add
// halves the lane span of TWO values: after both, every 16-lane row holds the partial sums of a different value and only
// ceil(n/4) registers are left for the four row-local DPP steps. 17 values: 34 adds instead of 102.
//   pair32(X, Y): lanes 0..31 = X[i] + X[i+32], lanes 32..63 = Y[i-32] + Y[i]
//   pair16(P, Q): row 0 = P.row0 + P.row1, row 1 = Q.row0 + Q.row1, row 2 = P.row2 + P.row3, row 3 = Q.row2 + Q.row3
typedef unsigned __attribute__((ext_vector_type(2))) f3dg_u2;
__device__ __forceinline__ float pair32(float x, float y)
{
    const f3dg_u2 r = __builtin_amdgcn_permlane32_swap(__float_as_uint(x), __float_as_uint(y), false, false);
    return __uint_as_float(r.x) + __uint_as_float(r.y);
}
__device__ __forceinline__ float pair16(float x, float y)
{
    const f3dg_u2 r = __builtin_amdgcn_permlane16_swap(__float_as_uint(x), __float_as_uint(y), false, false);
    return __uint_as_float(r.x) + __uint_as_float(r.y);
}
// total of each 16-lane row in its lane 15
__device__ __forceinline__ float row_total(float v)
{
    v += dpp_f32<F3DG_DPP_ROW_SHR(1), 0xF>(v);
    v += dpp_f32<F3DG_DPP_ROW_SHR(2), 0xF>(v);
    v += dpp_f32<F3DG_DPP_ROW_SHR(4), 0xF>(v);
    v += dpp_f32<F3DG_DPP_ROW_SHR(8), 0xF>(v);
    return v;
}

// ---- render3's counterpart: ONE wave64 per 8x8 quadrant, no workgroup barriers ------------------------------------------------------
// The reference's arithmetic per contributing (pixel, Gaussian) pair, followed by a transposed wave reduction. Around it, as in the
// forward (f3dg_render.hip, render3s_fwd_kernel):
//   * a workgroup is one wave that owns a quadrant from its deepest last contributor back to the first list entry; nothing is
//     shared with the other quadrants of the tile and nothing waits at a barrier;
//   * the wave scans the tile's list BACKWARDS 64 ids at a time and keeps the entries whose quadrant bit is set (F3DG_ID_BITS); a window
//     of 64 kept entries is staged and tested against the conservative ellipse: every pixel gets its pass mask and the wave the mask of
//     entries that can reach ANY of its pixels -- the others are never looked at (F3dgBwdWindow, f3dg_quad.h, shared with
//     render5_bwd_kernel);
//   * the surviving entries are walked in lock-step, back to front, because the 17 partials of a Gaussian are reduced across the
//     wave before they touch memory.
// Of a pair's arithmetic the kernel keeps what makes it the independent cross-check of render5_bwd_kernel: backward.cu's six per-pixel
// recurrences in registers, T rebuilt by the reference's division, its rounding of the background term. The rest is f3dg_bwd_pair.h.
template <int OCC>
__global__ void __launch_bounds__(64, OCC)
render3_bwd_kernel(const F3dgBwdLaunch::Args a, float* __restrict__ dL_dmean2D, float* __restrict__ dL_dopacity, float* __restrict__ dL_dcolors)
{
    const F3dgQuad qd = f3dg_quad(a.V, a.T, a.tiles_x);
    const unsigned lane = threadIdx.x;
    const auto [pix_x, pix_y, inside, pix_id, ray_x, ray_y] = f3dg_quad_pixel(qd, lane, a.W, a.H, a.focal_x, a.focal_y);

    __shared__ float4 sR[4][64];          // records of the window, [16-byte chunk][entry] (global_load_lds image)
    __shared__ float4 sC[64];             // 2D conic + opacity * coef
    __shared__ float2 sX[64];             // projected centre
    __shared__ uint2 sQ[F3DG_QUAD_RING];  // (list position, Gaussian id) of the kept entries, ring

    F3dgBwdWindow<false> w(a, sR, sC, sX, nullptr, sQ, qd, inside, pix_id, lane);
    const size_t vP = w.vP;
    const F3dgBwdPixel px = { ray_x, ray_y, (float)pix_x, (float)pix_y, { w.dpx0, w.dpx1, w.dpx2 }, { w.dn0, w.dn1, w.dn2 },
                              w.dL_dmax_depth, w.dL_dreg, w.final_A, w.final_D, w.max_contributor };
    float Tr = w.T_final;
    float accum_rec0 = 0, accum_rec1 = 0, accum_rec2 = 0;
    float last_alpha = 0;
    float last_c0 = 0, last_c1 = 0, last_c2 = 0;
    float last_n0 = 0, last_n1 = 0, last_n2 = 0;
    float acc_n0 = 0, acc_n1 = 0, acc_n2 = 0;
    unsigned n_pairs = 0;                 // contributing (pixel, Gaussian) pairs of this wave

    // Where lane 15 of row r adds its totals (see the reduction below): everything but the Gaussian id is fixed per lane, so the
    // address of an atomic is one multiply-add -- base + id * stride -- instead of per-row selects among four arrays.
    const unsigned row = lane >> 4;
    char* const add0 = row < 3 ? reinterpret_cast<char*>(dL_dcolors + vP * 3 + row) : reinterpret_cast<char*>(dL_dmean2D + vP * 3);   // stride 12
    char* const add1 = row < 2 ? reinterpret_cast<char*>(dL_dmean2D + vP * 3 + 1 + row) : reinterpret_cast<char*>(dL_dopacity);
    const unsigned stride1 = row < 2 ? 12u : 4u;
    char* const addD = reinterpret_cast<char*>(a.dL_dv2g_acc + vP * 10 + row);                                                         // stride 80

    while (w.next()) {
        // ---- lock-step walk over the entries that reach at least one pixel, back to front (window slot order)
        unsigned long long todo = w.any;
        while (todo != 0ull) {
            const int j = __builtin_ctzll(todo);
            todo &= todo - 1ull;
            const uint2 pe = w.entry((unsigned)j);
            const int contributor = (int)pe.x;                             // 0-based position from the front
            const bool reached = inside && ((w.pass >> j) & 1ull) != 0ull && contributor < w.last_contributor;
            if (__ballot(reached) == 0)
                continue;

            const F3dgBwdPair pr = f3dg_bwd_pair_eval(sR[0][j], sR[1][j], sR[2][j], ray_x, ray_y, w.alpha_fast, reached);
            {
                const unsigned long long act = __ballot(pr.live);
                if (act == 0)
                    continue;
                n_pairs += (unsigned)__popcll(act);
            }

            float g[17];
#pragma unroll
            for (int c = 0; c < 17; c++) g[c] = 0.0f;
            if (pr.live) {
                // gradient terms only from here: float32 with one reciprocal each, FMA contraction allowed
#pragma clang fp contract(fast)
                const float4 q3 = sR[3][j];
                const float alpha = pr.alpha;
                float nn0, nn1, nn2;
                f3dg_bwd_pair_normal(pr, nn0, nn1, nn2);

                // T is rebuilt by the reference's own IEEE division (backward.cu:803): a reciprocal + Newton step (<= 1 ulp per layer)
                // keeps the compositing-stage gradients within 1e-5, but the per-Gaussian stage amplifies even that on ill-conditioned
                // anisotropic scenes (dL/dscale of tests/test_raster_backward_gpu.py B2 moved from 2x to 3x the oracle's own error)
                const float oma = 1.f - alpha;
                Tr = Tr / oma;
                const float inv_oma = __builtin_amdgcn_rcpf(oma);      // background term only

                // backward.cu's recurrences: the colour / normal blended behind the entry, channel by channel
                float dL_dalpha = 0.0f;
                const float c0 = q3.x, c1 = q3.y, c2 = q3.z;
                accum_rec0 = last_alpha * last_c0 + (1.f - last_alpha) * accum_rec0; last_c0 = c0;
                dL_dalpha += (c0 - accum_rec0) * px.dpx[0];
                accum_rec1 = last_alpha * last_c1 + (1.f - last_alpha) * accum_rec1; last_c1 = c1;
                dL_dalpha += (c1 - accum_rec1) * px.dpx[1];
                accum_rec2 = last_alpha * last_c2 + (1.f - last_alpha) * accum_rec2; last_c2 = c2;
                dL_dalpha += (c2 - accum_rec2) * px.dpx[2];
                acc_n0 = last_alpha * last_n0 + (1.f - last_alpha) * acc_n0; last_n0 = nn0;
                dL_dalpha += (nn0 - acc_n0) * px.dn[0];
                acc_n1 = last_alpha * last_n1 + (1.f - last_alpha) * acc_n1; last_n1 = nn1;
                dL_dalpha += (nn1 - acc_n1) * px.dn[1];
                acc_n2 = last_alpha * last_n2 + (1.f - last_alpha) * acc_n2; last_n2 = nn2;
                dL_dalpha += (nn2 - acc_n2) * px.dn[2];
                dL_dalpha *= Tr;
                last_alpha = alpha;
                dL_dalpha += (-w.T_final * inv_oma) * w.bg_dot_dpixel;

                f3dg_bwd_pair_partials<true>(g, px, pr, sC[j], sX[j], w.ddelx_dx, w.ddely_dy, contributor, Tr, dL_dalpha);
            }

            // the 17 partials summed over the wave's 64 pixels (pair32 / pair16, then row-local DPP); the values are paired so that
            // lane 15 of row r holds element r of each target array:
            //                     row 0          row 1          row 2          row 3
            const float f0 = row_total(pair16(pair32(g[0], g[2]), pair32(g[1], g[3])));           // col0   col1   col2   mean2D.x
            const float f1 = row_total(pair16(pair32(g[4], g[6]), pair32(g[5], 0.0f)));           // m2D.y  m2D.z  opacity  -
            const float d0 = row_total(pair16(pair32(g[7], g[9]), pair32(g[8], g[10])));          // v0 v1 v2 v3
            const float d1 = row_total(pair16(pair32(g[11], g[13]), pair32(g[12], g[14])));       // v4 v5 v6 v7
            const float d2 = row_total(pair16(pair32(g[15], 0.0f), pair32(g[16], 0.0f)));         // v8 v9 -  -
            if ((lane & 15u) == 15u) {
                const size_t id = pe.y;
                unsafeAtomicAdd(reinterpret_cast<float*>(add0 + id * 12u), f0);
                if (row < 3) unsafeAtomicAdd(reinterpret_cast<float*>(add1 + id * stride1), f1);
                double* acc = reinterpret_cast<double*>(addD + id * 80u);
                unsafeAtomicAdd(acc, (double)d0);
                unsafeAtomicAdd(acc + 4, (double)d1);
                if (row < 2) unsafeAtomicAdd(acc + 8, (double)d2);
            }
        }
        w.retire();
    }
    if (lane == 0 && n_pairs)
        atomicAdd(&a.hdr->bwd_pairs, (unsigned long long)n_pairs);
}

struct M3 { float m[3][3]; };
struct M4 { float m[4][4]; };
__device__ __forceinline__ M3 mul(const M3& a, const M3& b)
{
    M3 r;
#pragma unroll
    for (int c = 0; c < 3; c++)
#pragma unroll
        for (int q = 0; q < 3; q++)
            r.m[c][q] = a.m[0][q] * b.m[c][0] + a.m[1][q] * b.m[c][1] + a.m[2][q] * b.m[c][2];
    return r;
}
__device__ __forceinline__ M3 transpose(const M3& a)
{
    M3 r;
#pragma unroll
    for (int c = 0; c < 3; c++)
#pragma unroll
        for (int q = 0; q < 3; q++)
            r.m[c][q] = a.m[q][c];
    return r;
}
__device__ __forceinline__ M4 mul(const M4& a, const M4& b)
{
    M4 r;
#pragma unroll
    for (int c = 0; c < 4; c++)
#pragma unroll
        for (int q = 0; q < 4; q++)
            r.m[c][q] = a.m[0][q] * b.m[c][0] + a.m[1][q] * b.m[c][1] + a.m[2][q] * b.m[c][2] + a.m[3][q] * b.m[c][3];
    return r;
}

__device__ __constant__ float B_SH_C0 = 0.28209479177387814f;
__device__ __constant__ float B_SH_C1 = 0.4886025119029199f;
__device__ __constant__ float B_SH_C2[5] = { 1.0925484305920792f, -1.0925484305920792f, 0.31539156525252005f,
                                             -1.0925484305920792f, 0.5462742152960396f };
__device__ __constant__ float B_SH_C3[7] = { -0.5900435899266435f, 2.890611442640554f, -0.4570457994644658f,
                                             0.3731763325901154f, -0.4570457994644658f, 1.445305721320277f,
                                             -0.5900435899266435f };

// One thread per GAUSSIAN (blockIdx.y: its set), looping over the views of its set: view2gaussian backward + SH backward. The per-Gaussian
// parameter gradients (mean, scale, rotation, SH) are summed over the views in registers and added to the caller's
// zero-filled outputs once, by their single writer: no atomics (a (view, Gaussian) grid with 22+ float atomics per
// thread measured 4.4 ms at 1 M Gaussians x 8 views, all of it contention), and a deterministic view order.
// Several sets (f3dg_backward_sets): the Gaussian inputs and the per-Gaussian sums are [n_sets, P, ...] and are indexed at set * P + g,
// the per-view planes at view * P + g with view in [set * V, (set + 1) * V) -- a set's sums never see another set's views.
__global__ void __launch_bounds__(F3DG_BLOCK)
preprocess_bwd_kernel(int P, int D, int M, const float* __restrict__ means3D, const int* __restrict__ radii,
                      const float* __restrict__ shs, const unsigned char* __restrict__ clamped,
                      const float* __restrict__ scales, const float* __restrict__ rotations,
                      const float* __restrict__ viewmatrices, const float* __restrict__ cam_positions,
                      const double* __restrict__ dL_dv2g_acc, float* __restrict__ dL_dv2g_out,
                      float* __restrict__ dL_dcolor, float* __restrict__ dL_dmeans, float* __restrict__ dL_dsh,
                      float* __restrict__ dL_dscale, float* __restrict__ dL_drot, int V /* views per set */,
                      int acc_stride /* doubles per (view, Gaussian) of dL_dv2g_acc: 10, or 16 = the packed records of the dense compositing backward */,
                      float* __restrict__ dL_dmean2D, float* __restrict__ dL_dopacity)
{
    const int g = blockIdx.x * F3DG_BLOCK + threadIdx.x;
    if (g >= P) return;
    const int set = blockIdx.y;
    const size_t gs = (size_t)set * P + g;
    float sum_mean[3] = { 0, 0, 0 }, sum_scale[3] = { 0, 0, 0 }, sum_rot[4] = { 0, 0, 0, 0 };
    float sum_sh[48];
#pragma unroll
    for (int i = 0; i < 48; i++) sum_sh[i] = 0.0f;
    bool any = false;
    float op_sum = 0.0f;

    for (int v = set * V; v < (set + 1) * V; v++) {
    const size_t idx = (size_t)v * P + g;

    float dv[10];
    const double* arec = dL_dv2g_acc + idx * (size_t)acc_stride;
    if (acc_stride == 16) {
        // the dense compositing backward (f3dg_backward5.hip) adds colour, mean2D and opacity into the same 128-byte record as the ten
        // float64 sums (one line per atomic event instead of four arrays): the record is read as seven 16-byte words, its float32 sums
        // leave for the caller's arrays here, the opacity summed over the views by its single writer
        const double2* a2 = reinterpret_cast<const double2*>(arec);
        const double2 d0 = a2[0], d1 = a2[1], d2 = a2[2], d3 = a2[3], d4 = a2[4];
        const float4 f0 = reinterpret_cast<const float4*>(arec)[5], f1 = reinterpret_cast<const float4*>(arec)[6];
        dv[0] = (float)d0.x; dv[1] = (float)d0.y; dv[2] = (float)d1.x; dv[3] = (float)d1.y; dv[4] = (float)d2.x;
        dv[5] = (float)d2.y; dv[6] = (float)d3.x; dv[7] = (float)d3.y; dv[8] = (float)d4.x; dv[9] = (float)d4.y;
        dL_dcolor[idx * 3] = f0.x; dL_dcolor[idx * 3 + 1] = f0.y; dL_dcolor[idx * 3 + 2] = f0.z;
        dL_dmean2D[idx * 3] = f0.w; dL_dmean2D[idx * 3 + 1] = f1.x; dL_dmean2D[idx * 3 + 2] = f1.y;
        op_sum += f1.z;
    } else {
#pragma unroll
        for (int i = 0; i < 10; i++) dv[i] = (float)arec[i];
    }
#pragma unroll
    for (int i = 0; i < 10; i++) dL_dv2g_out[idx * 10 + i] = dv[i];
    if (!(radii[idx] > 0)) continue;
    any = true;
    const float* view = viewmatrices + 16 * v;

    float dmean[3] = { 0, 0, 0 };
    if (scales && rotations) {
        const float sx = scales[3 * gs], sy = scales[3 * gs + 1], sz = scales[3 * gs + 2];
        const float4 rot = reinterpret_cast<const float4*>(rotations)[gs];
        const float mx = means3D[3 * gs], my = means3D[3 * gs + 1], mz = means3D[3 * gs + 2];
        const float r = rot.x, x = rot.y, y = rot.z, z = rot.w;
        M3 R;
        R.m[0][0] = 1.f - 2.f * (y * y + z * z); R.m[0][1] = 2.f * (x * y - r * z);       R.m[0][2] = 2.f * (x * z + r * y);
        R.m[1][0] = 2.f * (x * y + r * z);       R.m[1][1] = 1.f - 2.f * (x * x + z * z); R.m[1][2] = 2.f * (y * z - r * x);
        R.m[2][0] = 2.f * (x * z - r * y);       R.m[2][1] = 2.f * (y * z + r * x);       R.m[2][2] = 1.f - 2.f * (x * x + y * y);

        M4 G2W, W2V;
#pragma unroll
        for (int c = 0; c < 3; c++) {
            G2W.m[c][0] = R.m[0][c]; G2W.m[c][1] = R.m[1][c]; G2W.m[c][2] = R.m[2][c]; G2W.m[c][3] = 0.0f;
        }
        G2W.m[3][0] = mx; G2W.m[3][1] = my; G2W.m[3][2] = mz; G2W.m[3][3] = 1.0f;
#pragma unroll
        for (int c = 0; c < 4; c++)
#pragma unroll
            for (int q = 0; q < 4; q++)
                W2V.m[c][q] = view[4 * c + q];
        const M4 G2V = mul(W2V, G2W);

        M3 Rt;
#pragma unroll
        for (int c = 0; c < 3; c++) { Rt.m[c][0] = G2V.m[0][c]; Rt.m[c][1] = G2V.m[1][c]; Rt.m[c][2] = G2V.m[2][c]; }
        const float tx = G2V.m[3][0], ty = G2V.m[3][1], tz = G2V.m[3][2];
        float t2[3];
        t2[0] = (-Rt.m[0][0]) * tx + (-Rt.m[1][0]) * ty + (-Rt.m[2][0]) * tz;
        t2[1] = (-Rt.m[0][1]) * tx + (-Rt.m[1][1]) * ty + (-Rt.m[2][1]) * tz;
        t2[2] = (-Rt.m[0][2]) * tx + (-Rt.m[1][2]) * ty + (-Rt.m[2][2]) * tz;

        const double S[3] = { 1.0f / ((double)sx * sx + 1e-7), 1.0f / ((double)sy * sy + 1e-7), 1.0f / ((double)sz * sz + 1e-7) };
        M3 SR;
#pragma unroll
        for (int c = 0; c < 3; c++)
#pragma unroll
            for (int q = 0; q < 3; q++)
                SR.m[c][q] = (float)(S[q] * Rt.m[c][q]);

        M3 dSig;
        dSig.m[0][0] = dv[0];        dSig.m[0][1] = 0.5f * dv[1]; dSig.m[0][2] = 0.5f * dv[2];
        dSig.m[1][0] = 0.5f * dv[1]; dSig.m[1][1] = dv[3];        dSig.m[1][2] = 0.5f * dv[4];
        dSig.m[2][0] = 0.5f * dv[2]; dSig.m[2][1] = 0.5f * dv[4]; dSig.m[2][2] = dv[5];
        const float dB[3] = { dv[6], dv[7], dv[8] };
        const float dC = dv[9];

        M3 Dm = mul(Rt, dSig);
#pragma unroll
        for (int i = 0; i < 3; i++)
#pragma unroll
            for (int j = 0; j < 3; j++)
                Dm.m[i][j] = Dm.m[i][j] + t2[j] * dB[i];
        M3 dRt = transpose(mul(dSig, transpose(SR)));
#pragma unroll
        for (int c = 0; c < 3; c++)
#pragma unroll
            for (int q = 0; q < 3; q++)
                dRt.m[c][q] = dRt.m[c][q] + (float)(S[q] * Dm.m[c][q]);

        float dS[3], dt2[3];
#pragma unroll
        for (int q = 0; q < 3; q++)
            dS[q] = Dm.m[0][q] * Rt.m[0][q] + Dm.m[1][q] * Rt.m[1][q] + Dm.m[2][q] * Rt.m[2][q];
#pragma unroll
        for (int q = 0; q < 3; q++)
            dt2[q] = (float)(2 * t2[q] * S[q] * dC + dB[0] * SR.m[0][q] + dB[1] * SR.m[1][q] + dB[2] * SR.m[2][q]);
#pragma unroll
        for (int q = 0; q < 3; q++)
            dS[q] += dC * t2[q] * t2[q];
        const float sc[3] = { sx, sy, sz };
#pragma unroll
        for (int q = 0; q < 3; q++)
            sum_scale[q] += (float)(-2 / sc[q] * S[q] * dS[q]);

        const M3 dV2G_R_t = transpose(dRt);
        M3 dG2V_R;
        const float tv[3] = { tx, ty, tz };
#pragma unroll
        for (int c = 0; c < 3; c++)
#pragma unroll
            for (int q = 0; q < 3; q++)
                dG2V_R.m[c][q] = dV2G_R_t.m[c][q] + (-dt2[c] * tv[q]);
        const float nd[3] = { -dt2[0], -dt2[1], -dt2[2] };
        float dG2V_t[3];
#pragma unroll
        for (int c = 0; c < 3; c++)
            dG2V_t[c] = Rt.m[c][0] * nd[0] + Rt.m[c][1] * nd[1] + Rt.m[c][2] * nd[2];

        M4 dG2V, W2Vt;
#pragma unroll
        for (int c = 0; c < 3; c++) {
            dG2V.m[c][0] = dG2V_R.m[c][0]; dG2V.m[c][1] = dG2V_R.m[c][1]; dG2V.m[c][2] = dG2V_R.m[c][2]; dG2V.m[c][3] = 0.0f;
        }
        dG2V.m[3][0] = dG2V_t[0]; dG2V.m[3][1] = dG2V_t[1]; dG2V.m[3][2] = dG2V_t[2]; dG2V.m[3][3] = 0.0f;
#pragma unroll
        for (int c = 0; c < 4; c++)
#pragma unroll
            for (int q = 0; q < 4; q++)
                W2Vt.m[c][q] = W2V.m[q][c];
        const M4 dG2W = mul(W2Vt, dG2V);

        dmean[0] = dG2W.m[3][0]; dmean[1] = dG2W.m[3][1]; dmean[2] = dG2W.m[3][2];
        float Mt[3][3];
#pragma unroll
        for (int c = 0; c < 3; c++)
#pragma unroll
            for (int q = 0; q < 3; q++)
                Mt[c][q] = dG2W.m[c][q];
        const float q0 = 2 * z * (Mt[0][1] - Mt[1][0]) + 2 * y * (Mt[2][0] - Mt[0][2]) + 2 * x * (Mt[1][2] - Mt[2][1]);
        const float q1 = 2 * y * (Mt[1][0] + Mt[0][1]) + 2 * z * (Mt[2][0] + Mt[0][2]) + 2 * r * (Mt[1][2] - Mt[2][1]) - 4 * x * (Mt[2][2] + Mt[1][1]);
        const float q2 = 2 * x * (Mt[1][0] + Mt[0][1]) + 2 * r * (Mt[2][0] - Mt[0][2]) + 2 * z * (Mt[1][2] + Mt[2][1]) - 4 * y * (Mt[2][2] + Mt[0][0]);
        const float q3 = 2 * r * (Mt[0][1] - Mt[1][0]) + 2 * x * (Mt[2][0] + Mt[0][2]) + 2 * y * (Mt[1][2] + Mt[2][1]) - 4 * z * (Mt[1][1] + Mt[0][0]);
        sum_rot[0] += q0; sum_rot[1] += q1; sum_rot[2] += q2; sum_rot[3] += q3;
    }

    if (shs) {
        const float* campos = cam_positions + 3 * v;
        const float o0 = means3D[3 * gs] - campos[0], o1 = means3D[3 * gs + 1] - campos[1], o2 = means3D[3 * gs + 2] - campos[2];
        const float len = sqrtf(o0 * o0 + o1 * o1 + o2 * o2);
        const float x = o0 / len, y = o1 / len, z = o2 / len;
        const float* sh = shs + gs * M * 3;
        const unsigned char cl = clamped[idx];
        float dRGB[3];
#pragma unroll
        for (int ch = 0; ch < 3; ch++)
            dRGB[ch] = dL_dcolor[idx * 3 + ch] * ((cl >> ch) & 1 ? 0 : 1);
        float ddx[3] = { 0, 0, 0 }, ddy[3] = { 0, 0, 0 }, ddz[3] = { 0, 0, 0 };
#define F3DG_DSH(k, val) do { const float _w = (val); _Pragma("unroll") for (int ch = 0; ch < 3; ch++) sum_sh[(k) * 3 + ch] += _w * dRGB[ch]; } while (0)
#define F3DG_SH(k, ch) sh[(k) * 3 + (ch)]
        F3DG_DSH(0, B_SH_C0);
        if (D > 0) {
            F3DG_DSH(1, -B_SH_C1 * y);
            F3DG_DSH(2, B_SH_C1 * z);
            F3DG_DSH(3, -B_SH_C1 * x);
            for (int ch = 0; ch < 3; ch++) {
                ddx[ch] = -B_SH_C1 * F3DG_SH(3, ch);
                ddy[ch] = -B_SH_C1 * F3DG_SH(1, ch);
                ddz[ch] = B_SH_C1 * F3DG_SH(2, ch);
            }
            if (D > 1) {
                const float xx = x * x, yy = y * y, zz = z * z;
                const float xy = x * y, yz = y * z, xz = x * z;
                F3DG_DSH(4, B_SH_C2[0] * xy);
                F3DG_DSH(5, B_SH_C2[1] * yz);
                F3DG_DSH(6, B_SH_C2[2] * (2.f * zz - xx - yy));
                F3DG_DSH(7, B_SH_C2[3] * xz);
                F3DG_DSH(8, B_SH_C2[4] * (xx - yy));
                for (int ch = 0; ch < 3; ch++) {
                    ddx[ch] += B_SH_C2[0] * y * F3DG_SH(4, ch) + B_SH_C2[2] * 2.f * -x * F3DG_SH(6, ch) + B_SH_C2[3] * z * F3DG_SH(7, ch) + B_SH_C2[4] * 2.f * x * F3DG_SH(8, ch);
                    ddy[ch] += B_SH_C2[0] * x * F3DG_SH(4, ch) + B_SH_C2[1] * z * F3DG_SH(5, ch) + B_SH_C2[2] * 2.f * -y * F3DG_SH(6, ch) + B_SH_C2[4] * 2.f * -y * F3DG_SH(8, ch);
                    ddz[ch] += B_SH_C2[1] * y * F3DG_SH(5, ch) + B_SH_C2[2] * 2.f * 2.f * z * F3DG_SH(6, ch) + B_SH_C2[3] * x * F3DG_SH(7, ch);
                }
                if (D > 2) {
                    F3DG_DSH(9, B_SH_C3[0] * y * (3.f * xx - yy));
                    F3DG_DSH(10, B_SH_C3[1] * xy * z);
                    F3DG_DSH(11, B_SH_C3[2] * y * (4.f * zz - xx - yy));
                    F3DG_DSH(12, B_SH_C3[3] * z * (2.f * zz - 3.f * xx - 3.f * yy));
                    F3DG_DSH(13, B_SH_C3[4] * x * (4.f * zz - xx - yy));
                    F3DG_DSH(14, B_SH_C3[5] * z * (xx - yy));
                    F3DG_DSH(15, B_SH_C3[6] * x * (xx - 3.f * yy));
                    for (int ch = 0; ch < 3; ch++) {
                        ddx[ch] += (
                            B_SH_C3[0] * F3DG_SH(9, ch) * 3.f * 2.f * xy +
                            B_SH_C3[1] * F3DG_SH(10, ch) * yz +
                            B_SH_C3[2] * F3DG_SH(11, ch) * -2.f * xy +
                            B_SH_C3[3] * F3DG_SH(12, ch) * -3.f * 2.f * xz +
                            B_SH_C3[4] * F3DG_SH(13, ch) * (-3.f * xx + 4.f * zz - yy) +
                            B_SH_C3[5] * F3DG_SH(14, ch) * 2.f * xz +
                            B_SH_C3[6] * F3DG_SH(15, ch) * 3.f * (xx - yy));
                        ddy[ch] += (
                            B_SH_C3[0] * F3DG_SH(9, ch) * 3.f * (xx - yy) +
                            B_SH_C3[1] * F3DG_SH(10, ch) * xz +
                            B_SH_C3[2] * F3DG_SH(11, ch) * (-3.f * yy + 4.f * zz - xx) +
                            B_SH_C3[3] * F3DG_SH(12, ch) * -3.f * 2.f * yz +
                            B_SH_C3[4] * F3DG_SH(13, ch) * -2.f * xy +
                            B_SH_C3[5] * F3DG_SH(14, ch) * -2.f * yz +
                            B_SH_C3[6] * F3DG_SH(15, ch) * -3.f * 2.f * xy);
                        ddz[ch] += (
                            B_SH_C3[1] * F3DG_SH(10, ch) * xy +
                            B_SH_C3[2] * F3DG_SH(11, ch) * 4.f * 2.f * yz +
                            B_SH_C3[3] * F3DG_SH(12, ch) * 3.f * (2.f * zz - xx - yy) +
                            B_SH_C3[4] * F3DG_SH(13, ch) * 4.f * 2.f * xz +
                            B_SH_C3[5] * F3DG_SH(14, ch) * (xx - yy));
                    }
                }
            }
        }
#undef F3DG_DSH
#undef F3DG_SH
        const float dd0 = ddx[0] * dRGB[0] + ddx[1] * dRGB[1] + ddx[2] * dRGB[2];
        const float dd1 = ddy[0] * dRGB[0] + ddy[1] * dRGB[1] + ddy[2] * dRGB[2];
        const float dd2 = ddz[0] * dRGB[0] + ddz[1] * dRGB[1] + ddz[2] * dRGB[2];
        // dnormvdv (auxiliary.h:145-155)
        const float sum2 = o0 * o0 + o1 * o1 + o2 * o2;
        const float invsum32 = 1.0f / sqrtf(sum2 * sum2 * sum2);
        dmean[0] += ((+sum2 - o0 * o0) * dd0 - o1 * o0 * dd1 - o2 * o0 * dd2) * invsum32;
        dmean[1] += (-o0 * o1 * dd0 + (sum2 - o1 * o1) * dd1 - o2 * o1 * dd2) * invsum32;
        dmean[2] += (-o0 * o2 * dd0 - o1 * o2 * dd1 + (sum2 - o2 * o2) * dd2) * invsum32;
    }
    sum_mean[0] += dmean[0]; sum_mean[1] += dmean[1]; sum_mean[2] += dmean[2];
    }   // views

    if (acc_stride == 16) dL_dopacity[gs] += op_sum;
    if (!any) return;
#pragma unroll
    for (int q = 0; q < 3; q++) dL_dmeans[3 * gs + q] += sum_mean[q];
    if (scales && rotations) {
#pragma unroll
        for (int q = 0; q < 3; q++) dL_dscale[3 * gs + q] += sum_scale[q];
#pragma unroll
        for (int q = 0; q < 4; q++) dL_drot[4 * gs + q] += sum_rot[q];
    }
    if (shs) {
        float* dsh = dL_dsh + gs * M * 3;
        const int ncoef = (D + 1) * (D + 1);
#pragma unroll
        for (int i = 0; i < 48; i++)
            if (i < ncoef * 3) dsh[i] += sum_sh[i];
    }
}

// the lock-step walk compiled for OCC waves per SIMD (option bwd_occ)
template <int OCC>
void launch_render3_bwd(const F3dgBwdLaunch& a)
{
    F3DG_KLAUNCH((render3_bwd_kernel<OCC>), a.quadrants(), dim3(64), 0, a.s, a.k, a.dL_dmean2D, a.dL_dopacity, a.dL_dcolors);
}

int backward_sets(void* stream, void* workspace, size_t workspace_bytes, long long max_rendered,
                  int n_sets, int views_per_set, int P, int D, int M, const float* background, int W, int H,
                  const float* means3D, const float* shs, const float* scales, const float* rotations,
                  const float* viewmatrix, const float* cam_pos, float tan_fovx, float tan_fovy,
                  const int* radii, const float* dL_dpix,
                  float* dL_dmean2D, float* dL_dopacity, float* dL_dcolor,
                  float* dL_dmean3D, float* dL_dsh, float* dL_dscale, float* dL_drot,
                  float* dL_dview2gaussian, unsigned flags)
{
    hipStream_t s = (hipStream_t)stream;
    if (n_sets <= 0 || views_per_set <= 0 || (long long)n_sets * views_per_set > 0x7FFFFFF0ll) return F3DG_ERR_BAD_ARG;
    const int n_views = n_sets * views_per_set;
    if (P < 0 || W <= 0 || H <= 0 || !workspace || !dL_dpix || !background) return F3DG_ERR_BAD_ARG;
    if ((long long)n_views * P > 0xFFFFFFF0ll || n_sets > 65535) return F3DG_ERR_BAD_ARG;      // 32-bit (view, Gaussian) indices; the set is a grid's y
    if (P == 0) return F3DG_OK;
    if (!means3D || !viewmatrix || !cam_pos || !dL_dmean2D || !dL_dopacity || !dL_dcolor || !dL_dmean3D ||
        !dL_dview2gaussian)
        return F3DG_ERR_BAD_ARG;
    if ((scales != nullptr) != (rotations != nullptr)) return F3DG_ERR_BAD_ARG;
    if (scales && (!dL_dscale || !dL_drot)) return F3DG_ERR_BAD_ARG;
    if (shs && !dL_dsh) return F3DG_ERR_BAD_ARG;
    const F3dgLayout L = f3dg_layout(P, W, H, n_views, max_rendered);
    if (workspace_bytes < L.total) return F3DG_ERR_WORKSPACE;
    char* ws = static_cast<char*>(workspace);
    F3dgHeader* hdr = reinterpret_cast<F3dgHeader*>(ws + L.header);
    const int tiles_x = (W + F3DG_TILE - 1) / F3DG_TILE, tiles_y = (H + F3DG_TILE - 1) / F3DG_TILE;
    const int T = tiles_x * tiles_y;
    const float focal_y = H / (2.0f * tan_fovy);
    const float focal_x = W / (2.0f * tan_fovx);
    const int* radii_used = radii ? radii : reinterpret_cast<const int*>(ws + L.radii);

    // float64 accumulator of dL/dview2gaussian (its own region of the workspace)
    double* acc = reinterpret_cast<double*>(ws + L.bwd_acc);
    // (the lock-step walk adds dL/dopacity at the bare Gaussian id, which is right for one set only: several sets always take the dense
    // kernel, whose opacity sums stay in the per-(view, Gaussian) records until the per-Gaussian stage folds them set by set)
    const bool dense = g_f3dg_bwd_dense != 0 || n_sets > 1;
    const int acc_stride = dense ? 16 : 10;           // the dense kernel's 128-byte records (ten float64 + seven float32 sums) or [V*P][10]
    F3DG_HIP_CHECK(hipMemsetAsync(acc, 0, sizeof(double) * (size_t)acc_stride * (size_t)n_views * P, s));
    F3DG_HIP_CHECK(hipMemsetAsync(&hdr->bwd_pairs, 0, sizeof(hdr->bwd_pairs), s));
    if (!dense) {
        // the per-view outputs need no zero-fill by the caller: the dense path writes every element of them from its records
        // (preprocess_bwd_kernel); render3_bwd_kernel adds into these two
        F3DG_HIP_CHECK(hipMemsetAsync(dL_dmean2D, 0, sizeof(float) * 3 * (size_t)n_views * P, s));
        F3DG_HIP_CHECK(hipMemsetAsync(dL_dcolor, 0, sizeof(float) * 3 * (size_t)n_views * P, s));
    }
    const int prof = f3dg_prof_bwd_begin(s);

    const F3dgBwdLaunch launch = { s, { n_views, P, W, H, tiles_x, T, focal_x, focal_y, hdr, reinterpret_cast<const uint2*>(ws + L.ranges),
                                        reinterpret_cast<const unsigned*>(ws + L.vals[0]), reinterpret_cast<const unsigned*>(ws + L.small_list),
                                        reinterpret_cast<const F3dgRec*>(ws + L.rec), reinterpret_cast<const float4*>(ws + L.cull),
                                        reinterpret_cast<const float2*>(ws + L.means2D), reinterpret_cast<const float4*>(ws + L.conic), background,
                                        (flags & F3DG_FLAG_BG_PER_VIEW) ? 1 : 0, reinterpret_cast<const float*>(ws + L.final_T),
                                        reinterpret_cast<const unsigned*>(ws + L.n_contrib), dL_dpix, acc },
                                   dL_dmean2D, dL_dopacity, dL_dcolor };
    if (dense) {
        const int rc5 = f3dg_launch_render5_bwd(launch);
        if (rc5 != F3DG_OK) return rc5;
    } else {
        switch (g_f3dg_bwd_occ) {
        case 2: launch_render3_bwd<2>(launch); break;
        case 3: launch_render3_bwd<3>(launch); break;
        case 4: launch_render3_bwd<4>(launch); break;
        case 6: launch_render3_bwd<6>(launch); break;
        default: launch_render3_bwd<5>(launch); break;
        }
    }
    f3dg_prof_bwd_mark(prof, 0, s);
    F3DG_KLAUNCH(preprocess_bwd_kernel, dim3((P + F3DG_BLOCK - 1) / F3DG_BLOCK, (unsigned)n_sets), dim3(F3DG_BLOCK), 0, s, P,
                       D, M, means3D, radii_used, shs, reinterpret_cast<const unsigned char*>(ws + L.clamped), scales,
                       rotations, viewmatrix, cam_pos, acc, dL_dview2gaussian, dL_dcolor, dL_dmean3D, dL_dsh, dL_dscale,
                       dL_drot, views_per_set, acc_stride, dL_dmean2D, dL_dopacity);
    f3dg_prof_bwd_mark(prof, 1, s);
    F3DG_HIP_CHECK(hipGetLastError());
    return F3DG_OK;
}

} // namespace

extern "C" int f3dg_backward(void* stream, void* workspace, size_t workspace_bytes, long long max_rendered,
                             int n_views, int P, int D, int M, const float* background, int W, int H,
                             const float* means3D, const float* shs, const float* colors_precomp,
                             const float* scales, float scale_modifier, const float* rotations,
                             const float* cov3D_precomp, const float* view2gaussian_precomp,
                             const float* viewmatrix, const float* projmatrix, const float* cam_pos,
                             float tan_fovx, float tan_fovy, float kernel_size,
                             const int* radii, const float* dL_dpix,
                             float* dL_dmean2D, float* dL_dconic, float* dL_dopacity, float* dL_dcolor,
                             float* dL_dmean3D, float* dL_dcov3D, float* dL_dsh, float* dL_dscale, float* dL_drot,
                             float* dL_dview2gaussian, unsigned flags)
{
    (void)scale_modifier; (void)projmatrix; (void)kernel_size; (void)dL_dconic; (void)dL_dcov3D;
    (void)cov3D_precomp; (void)colors_precomp; (void)view2gaussian_precomp;
    return backward_sets(stream, workspace, workspace_bytes, max_rendered, 1, n_views, P, D, M, background, W, H, means3D, shs, scales,
                         rotations, viewmatrix, cam_pos, tan_fovx, tan_fovy, radii, dL_dpix, dL_dmean2D, dL_dopacity, dL_dcolor,
                         dL_dmean3D, dL_dsh, dL_dscale, dL_drot, dL_dview2gaussian, flags);
}

extern "C" int f3dg_backward_sets(void* stream, void* workspace, size_t workspace_bytes, long long max_rendered,
                                  int n_sets, int views_per_set, int P, int D, int M, const float* background, int W, int H,
                                  const float* means3D, const float* shs, const float* colors_precomp,
                                  const float* scales, float scale_modifier, const float* rotations,
                                  const float* cov3D_precomp, const float* view2gaussian_precomp,
                                  const float* viewmatrix, const float* projmatrix, const float* cam_pos,
                                  float tan_fovx, float tan_fovy, float kernel_size,
                                  const int* radii, const float* dL_dpix,
                                  float* dL_dmean2D, float* dL_dconic, float* dL_dopacity, float* dL_dcolor,
                                  float* dL_dmean3D, float* dL_dcov3D, float* dL_dsh, float* dL_dscale, float* dL_drot,
                                  float* dL_dview2gaussian, unsigned flags)
{
    (void)scale_modifier; (void)projmatrix; (void)kernel_size; (void)dL_dconic; (void)dL_dcov3D;
    (void)cov3D_precomp; (void)colors_precomp;
    if (n_sets > 1 && view2gaussian_precomp != nullptr) return F3DG_ERR_BAD_ARG;       // [n_views, P, 10] of ONE set, as in the forward
    return backward_sets(stream, workspace, workspace_bytes, max_rendered, n_sets, views_per_set, P, D, M, background, W, H, means3D, shs,
                         scales, rotations, viewmatrix, cam_pos, tan_fovx, tan_fovy, radii, dL_dpix, dL_dmean2D, dL_dopacity, dL_dcolor,
                         dL_dmean3D, dL_dsh, dL_dscale, dL_drot, dL_dview2gaussian, flags);
}
