// f3dg_bwd_pair.h -- the per-(pixel, Gaussian) arithmetic of the compositing backward (reference RAST/cuda_rasterizer/backward.cu:745-950).
//
// The ONE copy that render3_bwd_kernel (f3dg_backward.hip, the lock-step walk) and render5_bwd_kernel (f3dg_backward5.hip, dense
// batches) share: a fix to a derivative is made here, once. A pair is handled in three steps:
//   f3dg_bwd_pair_eval      t, G and alpha again, exactly as the workspace's forward computed them, and the reference's rejections;
//   the kernel's own part   dL/dalpha. The lock-step kernel keeps backward.cu's six per-pixel recurrences in registers, divides T by
//                           1 - alpha and rounds the background term as (-T_final / (1 - alpha)) (bg . dL/dC); the dense kernel keeps one
//                           folded recurrence in LDS, multiplies T by a correctly rounded reciprocal and rounds the background term as
//                           (-1 / (1 - alpha)) (T_final (bg . dL/dC)). Those three differences ARE the two kernels -- the lock-step one
//                           is the independent cross-check of the dense one (tests/test_raster_backward_gpu.py) -- and stay in them;
//   f3dg_bwd_pair_partials  from the finished dL/dalpha and T to the 17 partial derivatives that leave for memory (one switch, WALK, for
//                           three sums that the two kernels round in a different order: see there).
// The files are built with -ffp-contract=off: the evaluation keeps the reference's separate roundings, the gradient terms allow FMA
// contraction by a pragma of their own (float32 sums with one hardware reciprocal each, <= 1 ulp).
#pragma once
#include "f3dg_common.h"

// The pixel's constants as a pair sees them. The lock-step kernel fills it once from its lane's F3dgBwdWindow, the dense kernel per
// batch by ds_bpermute from the lane that owns the pair's pixel.
struct F3dgBwdPixel {
    float ray_x, ray_y;
    float pix_x, pix_y;               // the pixel's coordinates (its centre minus 0.5)
    float dpx[3], dn[3];              // dL/dcolour, dL/dnormal
    float dL_dmax_depth, dL_dreg;
    float final_A, final_D;
    int max_contributor;
};

struct F3dgBwdPair {
    float n0, n1, n2, aaf;            // the ray's normal in the Gaussian's frame (not normalised), a = r' Sigma' r
    float t, G, alpha;
    bool live;                        // the pair was blended by the forward as far as its own tests say (the caller knows the pixel's range)
};

// q0 = (v0 v1 v2 v3), q1 = (v4 v5 v6 v7), q2 = (v8 v9 opacity*coef K): the first three 16-byte chunks of the Gaussian's record.
// `candidate`: false for a lane that holds no pair, which only computes the quadric terms.
__device__ __forceinline__ F3dgBwdPair f3dg_bwd_pair_eval(const float4& q0, const float4& q1, const float4& q2, float ray_x, float ray_y,
                                                          bool alpha_fast, bool candidate)
{
    F3dgBwdPair pr;
    pr.n0 = q0.x * ray_x + q0.y * ray_y + q0.z;
    pr.n1 = q0.y * ray_x + q0.w * ray_y + q1.x;
    pr.n2 = q0.z * ray_x + q1.x * ray_y + q1.y;
    pr.aaf = ray_x * pr.n0 + ray_y * pr.n1 + pr.n2;
    const float bhalf = q1.z * ray_x + q1.w * ray_y + q2.x;
    const float CC = q2.y;
    pr.t = 1.0f; pr.G = 0; pr.alpha = 0;
    pr.live = candidate;
    if (pr.live) {
        if (alpha_fast) {
            // the forward of this workspace took the fast arithmetic: the same function, to the bit
            f3dg_fast_t_G(pr.aaf, bhalf, CC, pr.t, pr.G);
            if (pr.t < 0.2f) pr.live = false;
            pr.alpha = fminf(0.99f, q2.z * pr.G);
        } else {
            const double AA = pr.aaf;
            const double BB = 2 * bhalf;
            const double q = BB / AA;                          // one division: -BB / (2 * AA) == -0.5 * (BB / AA) exactly
            pr.t = (float)(-0.5 * q);
            if (pr.t <= F3DG_NEAR_PLANE) pr.live = false;
            const double min_value = -q * (BB / 4.) + CC;
            float power = (float)(-0.5f * min_value);
            if (power > 0.0f) power = 0.0f;
            pr.G = expf(power);
            pr.alpha = fminf(0.99f, q2.z * pr.G);
        }
        if (pr.alpha < 1.0f / 255.0f) pr.live = false;
    }
    return pr;
}

// 1 / |n| (hardware reciprocal square root, <= 1 ulp) and the unit normal the forward blended, already negated: what the kernels'
// recurrences accumulate
__device__ __forceinline__ float f3dg_bwd_pair_inv_len(const F3dgBwdPair& pr)
{
#pragma clang fp contract(fast)
    return __builtin_amdgcn_rsqf(pr.n0 * pr.n0 + pr.n1 * pr.n1 + pr.n2 * pr.n2 + 1e-7f);
}
__device__ __forceinline__ void f3dg_bwd_pair_normal(const F3dgBwdPair& pr, float& nn0, float& nn1, float& nn2)
{
#pragma clang fp contract(fast)
    const float inv_len = f3dg_bwd_pair_inv_len(pr);
    nn0 = -pr.n0 * inv_len; nn1 = -pr.n1 * inv_len; nn2 = -pr.n2 * inv_len;
}

// The 17 partials of a live pair in the order of the dense kernel's record: colour 0..2, mean2D 3..5, opacity 6, view2gaussian 7..16.
// con: the 2D conic with opacity * coef in .w; xy: the projected centre; contributor: the entry's 0-based list position; Tr: the
// transmittance in front of the entry; dL_dalpha: finished, background term included.
// WALK: where dL/dt joins the partials, the two kernels round differently, and each keeps its rounding (its results are bit for bit what
// they were when each had a copy of this text). A sum of two products under fp contract(fast) leaves to the compiler which product
// joins the FMA and which is rounded first; the two copies had come out differently for dL/dA and dL/dB, and render3_bwd_kernel wrote
// the distortion term as 0 + product, which keeps it out of the FMA with the max-depth cotangent. The three sums are written out:
//   true  (render3_bwd_kernel)  the source order: the term of the minimum is rounded, the term of dL/dt joins it in an FMA;
//   false (render5_bwd_kernel)  the other way round, and the distortion term's last product joins the max-depth cotangent in an FMA.
template <bool WALK>
__device__ __forceinline__ void f3dg_bwd_pair_partials(float* g, const F3dgBwdPixel& px, const F3dgBwdPair& pr, const float4& con, const float2& xy,
                                                       float ddelx_dx, float ddely_dy, int contributor, float Tr, float dL_dalpha)
{
    // gradient terms only: float32 with one reciprocal each, FMA contraction allowed
#pragma clang fp contract(fast)
    const float n0 = pr.n0, n1 = pr.n1, n2 = pr.n2, t = pr.t, G = pr.G, alpha = pr.alpha;
    const float d_x = xy.x - px.pix_x, d_y = xy.y - px.pix_y;

    // (hardware reciprocals / reciprocal square root, <= 1 ulp: these feed float32 gradient sums only)
    const float inv_t = __builtin_amdgcn_rcpf(t);
    const float mapped_max_t = fmaf(-0.20040080160320642f, inv_t, 1.0020040080160322f);
    const float dmax_t_dd = 0.20040080160320642f * inv_t * inv_t;
    const float inv_len = f3dg_bwd_pair_inv_len(pr);

    const float dchannel_dcolor = alpha * Tr;
    g[0] = dchannel_dcolor * px.dpx[0];
    g[1] = dchannel_dcolor * px.dpx[1];
    g[2] = dchannel_dcolor * px.dpx[2];

    float dL_dmax_t = 2.0f * (Tr * alpha) * (mapped_max_t * px.final_A - px.final_D) * px.dL_dreg * dmax_t_dd;
    if (WALK) dL_dmax_t = 0.0f + dL_dmax_t;     // takes the product's contraction: the sum with dL_dmax_depth below stays a sum
    const float dnn0 = alpha * Tr * px.dn[0], dnn1 = alpha * Tr * px.dn[1], dnn2 = alpha * Tr * px.dn[2];
    float dL_dlength = (dnn0 * n0 + dnn1 * n1 + dnn2 * n2);
    dL_dlength *= inv_len * inv_len;
    float dLn0 = (-dnn0 + dL_dlength * n0) * inv_len;
    float dLn1 = (-dnn1 + dL_dlength * n1) * inv_len;
    float dLn2 = (-dnn2 + dL_dlength * n2) * inv_len;

    float dL_dt = dL_dmax_t;
    if (contributor == px.max_contributor - 1)
        dL_dt += px.dL_dmax_depth;

    const float dL_dG = con.w * dL_dalpha;
    const float gdx = G * d_x;
    const float gdy = G * d_y;
    const float dG_ddelx = -gdx * con.x - gdy * con.y;
    const float dG_ddely = -gdy * con.z - gdx * con.y;
    g[3] = dL_dG * dG_ddelx * ddelx_dx;
    g[4] = dL_dG * dG_ddely * ddely_dy;
    g[5] = fabsf(dL_dG * dG_ddelx * ddelx_dx) + fabsf(dL_dG * dG_ddely * ddely_dy);
    g[6] = G * dL_dalpha;

    const float dL_dpower = dL_dG * G;
    const float dL_dmin_value = dL_dpower * -0.5f;
    const float qf = -2.0f * t, inv_a = __builtin_amdgcn_rcpf(pr.aaf);
    const float dL_dA = WALK ? fmaf(dL_dt, 0.5f * qf * inv_a, dL_dmin_value * qf * qf * 0.25f)
                             : fmaf(dL_dmin_value * qf * qf, 0.25f, dL_dt * (0.5f * qf * inv_a));
    const float dL_dB = WALK ? fmaf(dL_dt, -0.5f * inv_a, dL_dmin_value * (-0.5f * qf))
                             : fmaf(dL_dmin_value, -0.5f * qf, dL_dt * (-0.5f * inv_a));
    const float dL_dC = dL_dmin_value;
    dLn0 += dL_dA * px.ray_x;
    dLn1 += dL_dA * px.ray_y;
    dLn2 += dL_dA;

    g[7] = dLn0 * px.ray_x;
    g[8] = dLn0 * px.ray_y + dLn1 * px.ray_x;
    g[9] = dLn0 + dLn2 * px.ray_x;
    g[10] = dLn1 * px.ray_y;
    g[11] = dLn1 + dLn2 * px.ray_y;
    g[12] = dLn2;
    g[13] = dL_dB * 2 * px.ray_x;
    g[14] = dL_dB * 2 * px.ray_y;
    g[15] = dL_dB * 2;
    g[16] = dL_dC;
}
