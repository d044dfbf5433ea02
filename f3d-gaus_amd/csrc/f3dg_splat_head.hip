// f3dg_splat_head.hip -- cycle-aggregative projection ("splat head") and the render epilogue.
//
// splat_head_kernel fuses everything GaussianSplatPredictor_gtunet.forward does after the U-Net
// (reference src/gaussian_predictor.py): get_pos_from_network_output :857-881 (pos = ray_dirs * depth + offset),
// the [pos,1] @ view_to_world bmm and perspective divide :961-970, sigmoid / exp / F.normalize activations
// :976-979, transform_rotations = quaternion_raw_multiply(cam_quat, q) :839-855 / :45-64, transform_SHs
// :821-837 with the constant sh<->v permutation matrices :649-655, flatten_vector :788-791 (NCHW -> N x C), and
// writes straight into the aggregated per-image Gaussian buffers at `n_offset`, which replaces the torch.cat
// chain of the cycle loop (visualize.py:336-340) -- ~15 small torch kernels + permutes + 9 reallocations become
// one bandwidth-bound pass: 96 B read + 96 B written per Gaussian.
//
// splat_head_backward_kernel is its vector-Jacobian product with respect to net_out and depth (what torch.autograd derives from those
// same reference lines): the same grid, the forward's intermediates recomputed through shared __device__ helpers, no saved state, no atomics.
//
// epilogue_kernel fuses the post-processing of render_predicted_more_v2_gof
// (src/gaussian_renderer/__init__.py:1043-1053 world normals, :881-909 depth_to_normal).
//
// epilogue_backward_kernel is its vector-Jacobian product with respect to the raster: the same grid, the forward's points and cross
// products recomputed through the shared __device__ helpers, the depth channel as a gather over the pixel's axial neighbours.
#include "f3dg_common.h"
#include "f3dg_epilogue.h"

namespace {

// ---- per-pixel arithmetic shared by splat_head_kernel and splat_head_backward_kernel: the backward saves nothing and recomputes the
// forward's intermediates with these very float32 expressions
struct SplatPos { float den, X, Y, Z; };       // perspective divide, BEFORE the squre_clip clamp

__device__ __forceinline__ SplatPos splat_position(const float* __restrict__ net, const float* __restrict__ ray_dirs,
                                                   const float* __restrict__ M, int HW, int n, float d)
{
    // pos = ray_dirs * depth + offset  (two roundings, as torch evaluates it)
    const float p0 = ray_dirs[n] * d + net[0 * HW];
    const float p1 = ray_dirs[HW + n] * d + net[1 * HW];
    const float p2 = ray_dirs[2 * HW + n] * d + net[2 * HW];
    // [p,1] @ M
    const float w0 = p0 * M[0] + p1 * M[4] + p2 * M[8] + M[12];
    const float w1 = p0 * M[1] + p1 * M[5] + p2 * M[9] + M[13];
    const float w2 = p0 * M[2] + p1 * M[6] + p2 * M[10] + M[14];
    const float w3 = p0 * M[3] + p1 * M[7] + p2 * M[11] + M[15];
    SplatPos r;
    r.den = w3 + 1e-10f;
    r.X = w0 / r.den; r.Y = w1 / r.den; r.Z = w2 / r.den;
    return r;
}

__device__ __forceinline__ float splat_sigmoid(float x) { return 1.0f / (1.0f + expf(-x)); }

// |q| before F.normalize's clamp_min(1e-12)
__device__ __forceinline__ float splat_quat_norm(float bw, float bx, float by, float bz)
{
    return sqrtf(bw * bw + bx * bx + by * by + bz * bz);
}

// T = sh_to_v @ R @ v_to_sh with R = M[:3,:3]; the two constant matrices are signed permutations:
//   X = sh_to_v @ R : rows (-R[1], R[2], -R[0]);   T[i] = (-X[i][1], X[i][2], -X[i][0])
__device__ __forceinline__ void splat_sh_matrix(const float* __restrict__ M, float Tm[3][3])
{
    const float Xr[3][3] = { { -M[4], -M[5], -M[6] }, { M[8], M[9], M[10] }, { -M[0], -M[1], -M[2] } };
#pragma unroll
    for (int i = 0; i < 3; i++) { Tm[i][0] = -Xr[i][1]; Tm[i][1] = Xr[i][2]; Tm[i][2] = -Xr[i][0]; }
}

__global__ void __launch_bounds__(F3DG_BLOCK)
splat_head_kernel(int HW, const float* __restrict__ net_out, const float* __restrict__ depth,
                  const float* __restrict__ ray_dirs, const float* __restrict__ view_to_world,
                  const float* __restrict__ cam_quat, float squre_clip, long long n_total, long long n_offset,
                  float* __restrict__ xyz, float* __restrict__ opacity, float* __restrict__ scaling,
                  float* __restrict__ rotation, float* __restrict__ features_dc, float* __restrict__ features_rest,
                  float* __restrict__ unet_depth)
{
    const int n = blockIdx.x * F3DG_BLOCK + threadIdx.x;
    const int b = blockIdx.y;
    if (n >= HW) return;
    const float* net = net_out + (size_t)b * 23 * HW + n;       // channel c at net[c * HW]
    const float* M = view_to_world + 16 * b;                     // row-major 4x4, row-vector convention (uniform)
    const float* qc = cam_quat + 4 * b;

    const float d = depth[(size_t)b * HW + n];
    const SplatPos pos = splat_position(net, ray_dirs, M, HW, n, d);
    float X = pos.X, Y = pos.Y;
    const float Z = pos.Z;
    if (squre_clip < 10.0f) {       // clamp_(-c, c): NaN stays NaN as in torch (fminf / fmaxf would return the bound for it)
        X = X < -squre_clip ? -squre_clip : (X > squre_clip ? squre_clip : X);
        Y = Y < -squre_clip ? -squre_clip : (Y > squre_clip ? squre_clip : Y);
    }

    const size_t o = (size_t)b * (size_t)n_total + (size_t)n_offset + n;
    xyz[3 * o + 0] = X; xyz[3 * o + 1] = Y; xyz[3 * o + 2] = Z;

    opacity[o] = splat_sigmoid(net[3 * HW]);
    scaling[3 * o + 0] = expf(net[4 * HW]);
    scaling[3 * o + 1] = expf(net[5 * HW]);
    scaling[3 * o + 2] = expf(net[6 * HW]);

    // F.normalize(dim=channel, eps=1e-12) then Hamilton product cam_quat (x) q, real part first
    float bw = net[7 * HW], bx = net[8 * HW], by = net[9 * HW], bz = net[10 * HW];
    const float nrm = fmaxf(splat_quat_norm(bw, bx, by, bz), 1e-12f);
    bw /= nrm; bx /= nrm; by /= nrm; bz /= nrm;
    const float aw = qc[0], ax = qc[1], ay = qc[2], az = qc[3];
    rotation[4 * o + 0] = aw * bw - ax * bx - ay * by - az * bz;
    rotation[4 * o + 1] = aw * bx + ax * bw + ay * bz - az * by;
    rotation[4 * o + 2] = aw * by - ax * bz + ay * bw + az * bx;
    rotation[4 * o + 3] = aw * bz + ax * by - ay * bx + az * bw;

    features_dc[3 * o + 0] = net[11 * HW];
    features_dc[3 * o + 1] = net[12 * HW];
    features_dc[3 * o + 2] = net[13 * HW];

    float Tm[3][3];
    splat_sh_matrix(M, Tm);
    // rest'[t][c] = sum_s rest[s][c] * T[s][t], rest channel index = 14 + 3*s + c
#pragma unroll
    for (int c = 0; c < 3; c++) {
        const float s0 = net[(14 + c) * HW], s1 = net[(17 + c) * HW], s2 = net[(20 + c) * HW];
#pragma unroll
        for (int t = 0; t < 3; t++)
            features_rest[9 * o + 3 * t + c] = s0 * Tm[0][t] + s1 * Tm[1][t] + s2 * Tm[2][t];
    }
    unet_depth[o] = d;
}

// Backward of splat_head_kernel with respect to net_out and depth (the cameras and ray_dirs are data): one thread per (image, pixel),
// the same grid. A Gaussian's seven outputs depend on that pixel's 23 + 1 inputs only, so there is nothing to reduce: no atomics, no
// LDS, no saved state -- the forward's intermediates are recomputed from net_out / depth through the helpers above. A NULL g_* counts as
// all-zero upstream gradient; every element of d_net_out (and of d_depth unless NULL) is written.
__global__ void __launch_bounds__(F3DG_BLOCK)
splat_head_backward_kernel(int HW, const float* __restrict__ net_out, const float* __restrict__ depth,
                           const float* __restrict__ ray_dirs, const float* __restrict__ view_to_world,
                           const float* __restrict__ cam_quat, float squre_clip, long long n_total, long long n_offset,
                           const float* __restrict__ g_xyz, const float* __restrict__ g_opacity, const float* __restrict__ g_scaling,
                           const float* __restrict__ g_rotation, const float* __restrict__ g_features_dc,
                           const float* __restrict__ g_features_rest, const float* __restrict__ g_unet_depth,
                           float* __restrict__ d_net_out, float* __restrict__ d_depth)
{
    const int n = blockIdx.x * F3DG_BLOCK + threadIdx.x;
    const int b = blockIdx.y;
    if (n >= HW) return;
    const float* net = net_out + (size_t)b * 23 * HW + n;
    float* dnet = d_net_out + (size_t)b * 23 * HW + n;
    const float* M = view_to_world + 16 * b;
    const float* qc = cam_quat + 4 * b;
    const size_t o = (size_t)b * (size_t)n_total + (size_t)n_offset + n;

    // ---- position (gaussian_predictor.py:879, :961-970)
    float dp0 = 0.0f, dp1 = 0.0f, dp2 = 0.0f;
    if (g_xyz) {
        const SplatPos pos = splat_position(net, ray_dirs, M, HW, n, depth[(size_t)b * HW + n]);
        float gX = g_xyz[3 * o + 0], gY = g_xyz[3 * o + 1];
        const float gZ = g_xyz[3 * o + 2];
        if (squre_clip < 10.0f) {       // clamp_ passes the gradient where -c <= x <= c
            if (!(pos.X >= -squre_clip && pos.X <= squre_clip)) gX = 0.0f;
            if (!(pos.Y >= -squre_clip && pos.Y <= squre_clip)) gY = 0.0f;
        }
        const float dw0 = gX / pos.den, dw1 = gY / pos.den, dw2 = gZ / pos.den;
        const float dw3 = -(gX * pos.X + gY * pos.Y + gZ * pos.Z) / pos.den;
        dp0 = M[0] * dw0 + M[1] * dw1 + M[2] * dw2 + M[3] * dw3;
        dp1 = M[4] * dw0 + M[5] * dw1 + M[6] * dw2 + M[7] * dw3;
        dp2 = M[8] * dw0 + M[9] * dw1 + M[10] * dw2 + M[11] * dw3;
    }
    dnet[0 * HW] = dp0; dnet[1 * HW] = dp1; dnet[2 * HW] = dp2;
    if (d_depth) {
        const float gd = g_unet_depth ? g_unet_depth[o] : 0.0f;
        d_depth[(size_t)b * HW + n] = ray_dirs[n] * dp0 + ray_dirs[HW + n] * dp1 + ray_dirs[2 * HW + n] * dp2 + gd;
    }

    // ---- opacity: sigmoid (:975)
    float dop = 0.0f;
    if (g_opacity) {
        const float s = splat_sigmoid(net[3 * HW]);
        dop = g_opacity[o] * s * (1.0f - s);
    }
    dnet[3 * HW] = dop;

    // ---- scaling: exp (:976)
#pragma unroll
    for (int c = 0; c < 3; c++)
        dnet[(4 + c) * HW] = g_scaling ? g_scaling[3 * o + c] * expf(net[(4 + c) * HW]) : 0.0f;

    // ---- rotation: transpose of the Hamilton product cam_quat (x) q (:45-64, :839-855), then F.normalize (:977)
    float d0 = 0.0f, d1 = 0.0f, d2 = 0.0f, d3 = 0.0f;
    if (g_rotation) {
        const float g0 = g_rotation[4 * o + 0], g1 = g_rotation[4 * o + 1], g2 = g_rotation[4 * o + 2], g3 = g_rotation[4 * o + 3];
        const float aw = qc[0], ax = qc[1], ay = qc[2], az = qc[3];
        const float q0 = g0 * aw + g1 * ax + g2 * ay + g3 * az;
        const float q1 = -g0 * ax + g1 * aw + g2 * az - g3 * ay;
        const float q2 = -g0 * ay - g1 * az + g2 * aw + g3 * ax;
        const float q3 = -g0 * az + g1 * ay - g2 * ax + g3 * aw;
        const float bw = net[7 * HW], bx = net[8 * HW], by = net[9 * HW], bz = net[10 * HW];
        const float raw = splat_quat_norm(bw, bx, by, bz);
        if (raw >= 1e-12f) {
            const float hw = bw / raw, hx = bx / raw, hy = by / raw, hz = bz / raw;
            const float dot = hw * q0 + hx * q1 + hy * q2 + hz * q3;
            d0 = (q0 - hw * dot) / raw; d1 = (q1 - hx * dot) / raw; d2 = (q2 - hy * dot) / raw; d3 = (q3 - hz * dot) / raw;
        } else {                        // clamp_min(1e-12) is active: the norm gets no gradient
            d0 = q0 / 1e-12f; d1 = q1 / 1e-12f; d2 = q2 / 1e-12f; d3 = q3 / 1e-12f;
        }
    }
    dnet[7 * HW] = d0; dnet[8 * HW] = d1; dnet[9 * HW] = d2; dnet[10 * HW] = d3;

    // ---- features_dc: pass-through (:978)
#pragma unroll
    for (int c = 0; c < 3; c++)
        dnet[(11 + c) * HW] = g_features_dc ? g_features_dc[3 * o + c] : 0.0f;

    // ---- features_rest (:821-837): d_rest[s][c] = sum_t g[t][c] * T[s][t]
    if (g_features_rest) {
        float Tm[3][3];
        splat_sh_matrix(M, Tm);
#pragma unroll
        for (int c = 0; c < 3; c++) {
            const float t0 = g_features_rest[9 * o + 0 + c], t1 = g_features_rest[9 * o + 3 + c], t2 = g_features_rest[9 * o + 6 + c];
#pragma unroll
            for (int s = 0; s < 3; s++)
                dnet[(14 + 3 * s + c) * HW] = t0 * Tm[s][0] + t1 * Tm[s][1] + t2 * Tm[s][2];
        }
    } else {
#pragma unroll
        for (int c = 0; c < 9; c++) dnet[(14 + c) * HW] = 0.0f;
    }
}

// The epilogue's per-pixel arithmetic (invert4x4, epilogue_ray / _point / _cross, normalize3_backward) is in f3dg_epilogue.h.
// from_view: `c2w` holds the world_view matrices (row-vector convention, as the renderer receives them) and the kernel inverts their
// transposes itself -- the caller saves a torch.linalg.inv (a solver call and several launches per one-view call)
template <bool FROM_VIEW>
__global__ void __launch_bounds__(F3DG_BLOCK)
epilogue_kernel(int H, int W, const float* __restrict__ raster, const float* __restrict__ c2w, float fx, float fy,
                float* __restrict__ normal_world, float* __restrict__ depth_normal)
{
    const int HW = H * W;
    const int n = blockIdx.x * F3DG_BLOCK + threadIdx.x;
    const int v = blockIdx.y;
    __shared__ float s_c2w[16];
    if (FROM_VIEW) {
        if (threadIdx.x == 0) {
            float t[16];
            for (int r = 0; r < 4; r++)
                for (int c = 0; c < 4; c++) t[4 * r + c] = c2w[16 * v + 4 * c + r];      // world_view^T
            invert4x4(t, s_c2w);
        }
        __syncthreads();
    }
    if (n >= HW) return;
    const int y = n / W, x = n % W;
    const float* ras = raster + (size_t)v * F3DG_OUT_CHANNELS * HW;
    const float* Cw = FROM_VIEW ? s_c2w : c2w + 16 * v;     // row-major 4x4

    if (normal_world) {
        const float a = ras[3 * HW + n], b = ras[4 * HW + n], c = ras[5 * HW + n];
        const float nrm = fmaxf(sqrtf(a * a + b * b + c * c), 1e-12f);
        const float na = a / nrm, nb = b / nrm, nc = c / nrm;
        float* o = normal_world + (size_t)v * 3 * HW;
        o[n] = Cw[0] * na + Cw[1] * nb + Cw[2] * nc;
        o[HW + n] = Cw[4] * na + Cw[5] * nb + Cw[6] * nc;
        o[2 * HW + n] = Cw[8] * na + Cw[9] * nb + Cw[10] * nc;
    }
    if (depth_normal) {
        float* o = depth_normal + (size_t)v * 3 * HW;
        float r0 = 0, r1 = 0, r2 = 0;
        if (x >= 1 && x < W - 1 && y >= 1 && y < H - 1) {
            const float* dep = ras + 6 * HW;
            const float ax = 1.0f / fx, bx = -(W / 2.0f) / fx, ay = 1.0f / fy, by = -(H / 2.0f) / fy;
            const EpilogueCross k = epilogue_cross(dep, Cw, W, ax, bx, ay, by, y, x);
            const float nrm = fmaxf(sqrtf(k.cx * k.cx + k.cy * k.cy + k.cz * k.cz), 1e-12f);
            r0 = k.cx / nrm; r1 = k.cy / nrm; r2 = k.cz / nrm;
        }
        o[n] = r0; o[HW + n] = r1; o[2 * HW + n] = r2;
    }
}

// Adjoint of epilogue_kernel<true>: one thread per (view, pixel), the same grid. Channels 3..5 depend on this pixel's normal only.
// Channel 6 in GATHER form: the depth of pixel (y, x) is read by the depth normals of its axial neighbours that are interior pixels --
// as the "y + 1" point of centre (y - 1, x), the "y - 1" point of (y + 1, x), the "x + 1" point of (y, x - 1) and the "x - 1" point of
// (y, x + 1). For each such centre the thread recomputes the forward's two difference vectors and cross product from `raster`, takes the
// centre's cotangent through the normalisation and through c = e x g (dL/de = g x w, dL/dg = w x e), and dots the result with its own
// ray: d point / d depth. The up to four terms are summed in that order. No atomics, no LDS beyond the matrix, nothing saved by the
// forward; the kernel ADDS into channels 3..5 and 6 of dL_dpix and touches no other channel.
__global__ void __launch_bounds__(F3DG_BLOCK)
epilogue_backward_kernel(int H, int W, const float* __restrict__ raster, const float* __restrict__ world_view, float fx, float fy,
                         const float* __restrict__ g_normal_world, const float* __restrict__ g_depth_normal, float* __restrict__ dL_dpix)
{
    const int HW = H * W;
    const int n = blockIdx.x * F3DG_BLOCK + threadIdx.x;
    const int v = blockIdx.y;
    __shared__ float s_c2w[16];
    if (threadIdx.x == 0) {         // c2w = inverse(world_view^T), as epilogue_kernel<true> forms it
        float t[16];
        for (int r = 0; r < 4; r++)
            for (int c = 0; c < 4; c++) t[4 * r + c] = world_view[16 * v + 4 * c + r];
        invert4x4(t, s_c2w);
    }
    __syncthreads();
    if (n >= HW) return;
    const int y = n / W, x = n % W;
    const float* ras = raster + (size_t)v * F3DG_OUT_CHANNELS * HW;
    float* dpix = dL_dpix + (size_t)v * F3DG_OUT_CHANNELS * HW;
    const float* Cw = s_c2w;

    if (g_normal_world) {
        const float* gw = g_normal_world + (size_t)v * 3 * HW;
        const float w0 = gw[n], w1 = gw[HW + n], w2 = gw[2 * HW + n];
        // c2w[:3,:3]^T applied to the cotangent, then the normalisation
        float g0 = Cw[0] * w0 + Cw[4] * w1 + Cw[8] * w2;
        float g1 = Cw[1] * w0 + Cw[5] * w1 + Cw[9] * w2;
        float g2 = Cw[2] * w0 + Cw[6] * w1 + Cw[10] * w2;
        normalize3_backward(ras[3 * HW + n], ras[4 * HW + n], ras[5 * HW + n], g0, g1, g2);
        dpix[3 * HW + n] += g0; dpix[4 * HW + n] += g1; dpix[5 * HW + n] += g2;
    }
    if (g_depth_normal) {
        const float* gd = g_depth_normal + (size_t)v * 3 * HW;
        const float* dep = ras + 6 * HW;
        const float ax = 1.0f / fx, bx = -(W / 2.0f) / fx, ay = 1.0f / fy, by = -(H / 2.0f) / fy;
        float rx, ry, rz;
        epilogue_ray(Cw, ax, bx, ay, by, y, x, rx, ry, rz);
        // the cotangent of centre (cy, cx) taken back to its difference vectors: along_rows selects dL/de (else dL/dg), dotted with this ray
        auto term = [&](int cy, int cx, bool along_rows) -> float {
            if (!(cx >= 1 && cx < W - 1 && cy >= 1 && cy < H - 1)) return 0.0f;
            const EpilogueCross k = epilogue_cross(dep, Cw, W, ax, bx, ay, by, cy, cx);
            const int m = cy * W + cx;
            float w0 = gd[m], w1 = gd[HW + m], w2 = gd[2 * HW + m];
            normalize3_backward(k.cx, k.cy, k.cz, w0, w1, w2);
            float p0, p1, p2;
            if (along_rows) { p0 = k.gy * w2 - k.gz * w1; p1 = k.gz * w0 - k.gx * w2; p2 = k.gx * w1 - k.gy * w0; }      // g x w
            else            { p0 = w1 * k.ez - w2 * k.ey; p1 = w2 * k.ex - w0 * k.ez; p2 = w0 * k.ey - w1 * k.ex; }      // w x e
            return rx * p0 + ry * p1 + rz * p2;
        };
        float sum = term(y - 1, x, true);
        sum -= term(y + 1, x, true);
        sum += term(y, x - 1, false);
        sum -= term(y, x + 1, false);
        dpix[6 * HW + n] += sum;
    }
}

// 8-bit RGB frames for the video writer / the multi-GPU gather: dst[n][y][x][c] = (uint8)(255 * clamp(src[n][c][y][x], 0, 1))
// exactly as visualize.py:407,416 does on the host ((255 * np.clip(x, 0, 1)).astype(np.uint8): float32 product, truncation).
// src is planar with `src_channels` planes per frame (9 for the rasterizer output) of which the first three are read.
__global__ void __launch_bounds__(F3DG_BLOCK)
pack_frames_kernel(size_t HW, int src_channels, const float* __restrict__ src, unsigned char* __restrict__ dst)
{
    const size_t q = (size_t)blockIdx.x * F3DG_BLOCK + threadIdx.x;      // group of 4 pixels
    const size_t n = blockIdx.y;
    const float* s = src + n * (size_t)src_channels * HW;
    unsigned char* d = dst + n * 3 * HW;
    auto cv = [](float v) -> unsigned { return (unsigned)(255.0f * fminf(fmaxf(v, 0.0f), 1.0f)); };
    if (q * 4 + 4 <= HW && (HW & 3) == 0) {
        const float4 r = reinterpret_cast<const float4*>(s)[q];
        const float4 g = reinterpret_cast<const float4*>(s + HW)[q];
        const float4 b = reinterpret_cast<const float4*>(s + 2 * HW)[q];
        const unsigned w0 = cv(r.x) | (cv(g.x) << 8) | (cv(b.x) << 16) | (cv(r.y) << 24);
        const unsigned w1 = cv(g.y) | (cv(b.y) << 8) | (cv(r.z) << 16) | (cv(g.z) << 24);
        const unsigned w2 = cv(b.z) | (cv(r.w) << 8) | (cv(g.w) << 16) | (cv(b.w) << 24);
        unsigned* o = reinterpret_cast<unsigned*>(d + q * 12);
        o[0] = w0; o[1] = w1; o[2] = w2;
    } else {
        for (size_t p = q * 4; p < q * 4 + 4 && p < HW; p++) {
            d[3 * p] = (unsigned char)cv(s[p]);
            d[3 * p + 1] = (unsigned char)cv(s[HW + p]);
            d[3 * p + 2] = (unsigned char)cv(s[2 * HW + p]);
        }
    }
}

// The same frames written STRAIGHT into pinned host memory (device-accessible: hipHostMalloc / torch pin_memory): no staging copy in
// HBM and no copy command. HIP runs a device -> pinned-host hipMemcpyAsync as a shader copy over the whole chip
// (__amd_rocclr_copyBuffer, 0.43 ms per 23.6 MB on this box: tools/micro/d2h_engine.py) which takes wave slots from the next step's
// rendering; this kernel is PCIe-bound all the same, so a FEW workgroups (max_workgroups) move it in the same time and leave the
// rest of the chip alone. A lane produces one 16-byte chunk of the byte stream -- 5 1/3 pixels: byte B of a frame is channel B % 3 of
// pixel B / 3 -- so that a store instruction of a wave writes 1 KB of contiguous host memory (the fabric forwards partial lines as
// small PCIe writes); the 16 float reads of a lane are shared with its neighbours through L1 / L2.
__global__ void __launch_bounds__(F3DG_BLOCK)
pack_frames_host_kernel(size_t n_bytes, size_t HW, int src_channels, const float* __restrict__ src, unsigned char* __restrict__ dst)
{
    auto cv = [](float v) -> unsigned { return (unsigned)(255.0f * fminf(fmaxf(v, 0.0f), 1.0f)); };
    const size_t frame_bytes = 3 * HW, n_chunks = (n_bytes + 15) / 16;
    for (size_t c = (size_t)blockIdx.x * F3DG_BLOCK + threadIdx.x; c < n_chunks; c += (size_t)gridDim.x * F3DG_BLOCK) {
        const size_t b0 = 16 * c;
        size_t n = b0 / frame_bytes;
        unsigned rem = (unsigned)(b0 - n * frame_bytes);           // (a frame is < 4 GB)
        const float* s = src + n * (size_t)src_channels * HW;
        unsigned p = rem / 3u, ch = rem - 3u * p;
        unsigned w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
        for (int j = 0; j < 16; j++) {
            if (b0 + j < n_bytes)
                w[j >> 2] |= cv(s[(size_t)ch * HW + p]) << (8 * (j & 3));
            if (++ch == 3u) {
                ch = 0u;
                if (++p == (unsigned)HW) { p = 0u; s += (size_t)src_channels * HW; }       // the chunk runs into the next frame
            }
        }
        if (b0 + 16 <= n_bytes) {
            *reinterpret_cast<uint4*>(dst + b0) = make_uint4(w[0], w[1], w[2], w[3]);
        } else {
            for (int j = 0; b0 + j < n_bytes; j++) dst[b0 + j] = (unsigned char)(w[j >> 2] >> (8 * (j & 3)));
        }
    }
}

} // namespace

extern "C" int f3dg_splat_head(void* stream, int B, int H, int W, const float* net_out, const float* depth,
                               const float* ray_dirs, const float* view_to_world, const float* cam_quat,
                               float squre_clip, long long n_total, long long n_offset,
                               float* xyz, float* opacity, float* scaling, float* rotation,
                               float* features_dc, float* features_rest, float* unet_depth)
{
    if (B <= 0 || H <= 0 || W <= 0 || !net_out || !depth || !ray_dirs || !view_to_world || !cam_quat || !xyz ||
        !opacity || !scaling || !rotation || !features_dc || !features_rest || !unet_depth)
        return F3DG_ERR_BAD_ARG;
    const long long HW = (long long)H * W;
    if (n_offset < 0 || n_total < n_offset + HW) return F3DG_ERR_BAD_ARG;
    dim3 grid((unsigned)((HW + F3DG_BLOCK - 1) / F3DG_BLOCK), (unsigned)B);
    F3DG_KLAUNCH(splat_head_kernel, grid, dim3(F3DG_BLOCK), 0, (hipStream_t)stream, (int)HW, net_out, depth,
                       ray_dirs, view_to_world, cam_quat, squre_clip, n_total, n_offset, xyz, opacity, scaling,
                       rotation, features_dc, features_rest, unet_depth);
    F3DG_HIP_CHECK(hipGetLastError());
    return F3DG_OK;
}

extern "C" int f3dg_splat_head_backward(void* stream, int B, int H, int W, const float* net_out, const float* depth,
                                        const float* ray_dirs, const float* view_to_world, const float* cam_quat,
                                        float squre_clip, long long n_total, long long n_offset,
                                        const float* g_xyz, const float* g_opacity, const float* g_scaling, const float* g_rotation,
                                        const float* g_features_dc, const float* g_features_rest, const float* g_unet_depth,
                                        float* d_net_out, float* d_depth)
{
    if (B <= 0 || H <= 0 || W <= 0 || !net_out || !depth || !ray_dirs || !view_to_world || !cam_quat || !d_net_out)
        return F3DG_ERR_BAD_ARG;
    const long long HW = (long long)H * W;
    if (n_offset < 0 || n_total < n_offset + HW) return F3DG_ERR_BAD_ARG;
    dim3 grid((unsigned)((HW + F3DG_BLOCK - 1) / F3DG_BLOCK), (unsigned)B);
    F3DG_KLAUNCH(splat_head_backward_kernel, grid, dim3(F3DG_BLOCK), 0, (hipStream_t)stream, (int)HW, net_out, depth,
                       ray_dirs, view_to_world, cam_quat, squre_clip, n_total, n_offset, g_xyz, g_opacity, g_scaling,
                       g_rotation, g_features_dc, g_features_rest, g_unet_depth, d_net_out, d_depth);
    F3DG_HIP_CHECK(hipGetLastError());
    return F3DG_OK;
}

extern "C" int f3dg_render_epilogue(void* stream, int n_views, int H, int W, const float* raster,
                                    const float* c2w, float fx, float fy,
                                    float* normal_world, float* depth_normal)
{
    if (n_views <= 0 || H <= 0 || W <= 0 || !raster || !c2w) return F3DG_ERR_BAD_ARG;
    if (!normal_world && !depth_normal) return F3DG_OK;
    dim3 grid((unsigned)(((long long)H * W + F3DG_BLOCK - 1) / F3DG_BLOCK), (unsigned)n_views);
    F3DG_KLAUNCH(epilogue_kernel<false>, grid, dim3(F3DG_BLOCK), 0, (hipStream_t)stream, H, W, raster, c2w, fx, fy,
                       normal_world, depth_normal);
    F3DG_HIP_CHECK(hipGetLastError());
    return F3DG_OK;
}

extern "C" int f3dg_render_epilogue_view(void* stream, int n_views, int H, int W, const float* raster,
                                         const float* world_view, float fx, float fy,
                                         float* normal_world, float* depth_normal)
{
    if (n_views <= 0 || H <= 0 || W <= 0 || !raster || !world_view) return F3DG_ERR_BAD_ARG;
    if (!normal_world && !depth_normal) return F3DG_OK;
    dim3 grid((unsigned)(((long long)H * W + F3DG_BLOCK - 1) / F3DG_BLOCK), (unsigned)n_views);
    F3DG_KLAUNCH(epilogue_kernel<true>, grid, dim3(F3DG_BLOCK), 0, (hipStream_t)stream, H, W, raster, world_view, fx, fy,
                       normal_world, depth_normal);
    F3DG_HIP_CHECK(hipGetLastError());
    return F3DG_OK;
}

extern "C" int f3dg_render_epilogue_backward(void* stream, int n_views, int H, int W, const float* raster,
                                             const float* world_view, float fx, float fy,
                                             const float* dL_dnormal_world, const float* dL_ddepth_normal, float* dL_dpix)
{
    // (the kernel forms channel * HW + pixel, channel < 9, in int)
    if (n_views <= 0 || H <= 0 || W <= 0 || 9ll * H * W > 0x7FFFFFF0ll || !raster || !world_view || !dL_dpix) return F3DG_ERR_BAD_ARG;
    if (!dL_dnormal_world && !dL_ddepth_normal) return F3DG_OK;
    dim3 grid((unsigned)(((long long)H * W + F3DG_BLOCK - 1) / F3DG_BLOCK), (unsigned)n_views);
    F3DG_KLAUNCH(epilogue_backward_kernel, grid, dim3(F3DG_BLOCK), 0, (hipStream_t)stream, H, W, raster, world_view, fx, fy,
                       dL_dnormal_world, dL_ddepth_normal, dL_dpix);
    F3DG_HIP_CHECK(hipGetLastError());
    return F3DG_OK;
}

extern "C" int f3dg_pack_frames(void* stream, int n_frames, int H, int W, int src_channels, const float* src,
                                unsigned char* dst)
{
    if (n_frames < 0 || H <= 0 || W <= 0 || src_channels < 3 || !src || !dst) return F3DG_ERR_BAD_ARG;
    if (n_frames == 0) return F3DG_OK;
    const size_t HW = (size_t)H * W;
    if (((uintptr_t)src & 15u) || ((uintptr_t)dst & 3u)) return F3DG_ERR_BAD_ARG;
    F3DG_KLAUNCH(pack_frames_kernel, dim3((unsigned)((HW / 4 + F3DG_BLOCK) / F3DG_BLOCK), (unsigned)n_frames), dim3(F3DG_BLOCK), 0,
                       (hipStream_t)stream, HW, src_channels, src, dst);
    F3DG_HIP_CHECK(hipGetLastError());
    return F3DG_OK;
}

extern "C" int f3dg_pack_frames_host(void* stream, int n_frames, int H, int W, int src_channels, const float* src,
                                     unsigned char* dst_host, int max_workgroups)
{
    if (n_frames < 0 || H <= 0 || W <= 0 || src_channels < 3 || !src || !dst_host) return F3DG_ERR_BAD_ARG;
    if (n_frames == 0) return F3DG_OK;
    if ((uintptr_t)dst_host & 15u) return F3DG_ERR_BAD_ARG;
    const size_t HW = (size_t)H * W, n_bytes = 3 * HW * (size_t)n_frames;
    if (3 * HW >= ((size_t)1 << 32)) return F3DG_ERR_BAD_ARG;
    hipPointerAttribute_t at;
    if (hipPointerGetAttributes(&at, dst_host) != hipSuccess || at.type != hipMemoryTypeHost) {      // pinned, device-accessible host memory only
        (void)hipGetLastError();
        return F3DG_ERR_BAD_ARG;
    }
    const size_t need = ((n_bytes + 15) / 16 + F3DG_BLOCK - 1) / F3DG_BLOCK;
    size_t grid = max_workgroups > 0 ? (size_t)max_workgroups : 64;
    if (grid > need) grid = need;
    F3DG_KLAUNCH(pack_frames_host_kernel, dim3((unsigned)grid), dim3(F3DG_BLOCK), 0, (hipStream_t)stream, n_bytes, HW, src_channels, src,
                 dst_host);
    F3DG_HIP_CHECK(hipGetLastError());
    return F3DG_OK;
}

// ------------------------------------------------------------------------------------------------ cycle inputs
// Hand-off of the cycle aggregation (reference visualize.py:311, 331-333): every rendered view becomes the next predictor
// input  cat(clamp(rgb, 0, 1), alpha)  [4, H, W]  with its median depth [1, H, W] as unet_depth. One pass over the 9-channel
// raster instead of clamp + two slices + cat (and the .cpu() round trips of the reference). Frame n = b * V + v of the raster is
// written to slot v * B + b, so that the B inputs of one novel view are one contiguous predictor batch.
namespace {
__global__ void __launch_bounds__(F3DG_BLOCK)
cycle_inputs_kernel(size_t HW, int B, int V, const float* __restrict__ raster, float* __restrict__ xin, float* __restrict__ depth)
{
    const size_t i = ((size_t)blockIdx.x * F3DG_BLOCK + threadIdx.x) * 4;
    if (i >= HW) return;
    const unsigned n = blockIdx.y, b = n / (unsigned)V, v = n % (unsigned)V;
    const float* src = raster + (size_t)n * F3DG_OUT_CHANNELS * HW;
    const size_t slot = (size_t)v * B + b;
    float* x = xin + slot * 4 * HW;
    auto clamp4 = [](float4 q) {      // torch.clamp(x, 0, 1): NaN stays NaN
        q.x = q.x < 0.0f ? 0.0f : (q.x > 1.0f ? 1.0f : q.x); q.y = q.y < 0.0f ? 0.0f : (q.y > 1.0f ? 1.0f : q.y);
        q.z = q.z < 0.0f ? 0.0f : (q.z > 1.0f ? 1.0f : q.z); q.w = q.w < 0.0f ? 0.0f : (q.w > 1.0f ? 1.0f : q.w);
        return q;
    };
    if (i + 4 <= HW) {
        *reinterpret_cast<float4*>(x + 0 * HW + i) = clamp4(*reinterpret_cast<const float4*>(src + 0 * HW + i));
        *reinterpret_cast<float4*>(x + 1 * HW + i) = clamp4(*reinterpret_cast<const float4*>(src + 1 * HW + i));
        *reinterpret_cast<float4*>(x + 2 * HW + i) = clamp4(*reinterpret_cast<const float4*>(src + 2 * HW + i));
        *reinterpret_cast<float4*>(x + 3 * HW + i) = *reinterpret_cast<const float4*>(src + 7 * HW + i);
        *reinterpret_cast<float4*>(depth + slot * HW + i) = *reinterpret_cast<const float4*>(src + 6 * HW + i);
    } else {
        for (size_t k = i; k < HW; k++) {
            for (int c = 0; c < 3; c++) { const float q = src[c * HW + k]; x[c * HW + k] = q < 0.0f ? 0.0f : (q > 1.0f ? 1.0f : q); }
            x[3 * HW + k] = src[7 * HW + k];
            depth[slot * HW + k] = src[6 * HW + k];
        }
    }
}
} // namespace

extern "C" int f3dg_cycle_inputs(void* stream, int B, int V, int H, int W, const float* raster, float* xin, float* depth)
{
    if (B < 0 || V <= 0 || H <= 0 || W <= 0 || !raster || !xin || !depth) return F3DG_ERR_BAD_ARG;
    if (B == 0) return F3DG_OK;
    const size_t HW = (size_t)H * W;
    if ((HW & 3u) || ((uintptr_t)raster & 15u) || ((uintptr_t)xin & 15u) || ((uintptr_t)depth & 15u)) return F3DG_ERR_BAD_ARG;
    F3DG_KLAUNCH(cycle_inputs_kernel, dim3((unsigned)((HW / 4 + F3DG_BLOCK - 1) / F3DG_BLOCK), (unsigned)(B * V)), dim3(F3DG_BLOCK), 0,
                       (hipStream_t)stream, HW, B, V, raster, xin, depth);
    F3DG_HIP_CHECK(hipGetLastError());
    return F3DG_OK;
}

// Adjoint of cycle_inputs_kernel (what torch.autograd derives from visualize.py:311, 331-333): the same launch shape, one thread per four
// pixels of frame n = b * V + v, which takes its cotangents from slot v * B + b and writes all nine planes of d_raster. The clamp passes
// the cotangent where 0 <= raster <= 1 (both ends and -0.0 included; NaN and +-Inf fail both comparisons); elsewhere +0.0 is SELECTED,
// never g * 0, so a non-finite cotangent under the mask cannot leak. A NULL g_xin / g_depth counts as all-zero.
namespace {
__global__ void __launch_bounds__(F3DG_BLOCK)
cycle_inputs_backward_kernel(size_t HW, int B, int V, const float* __restrict__ raster, const float* __restrict__ g_xin,
                             const float* __restrict__ g_depth, float* __restrict__ d_raster)
{
    const size_t i = ((size_t)blockIdx.x * F3DG_BLOCK + threadIdx.x) * 4;
    if (i >= HW) return;             // (HW is a multiple of 4: a thread's four pixels are all inside or all outside)
    const unsigned n = blockIdx.y, b = n / (unsigned)V, v = n % (unsigned)V;
    const float* src = raster + (size_t)n * F3DG_OUT_CHANNELS * HW + i;
    float* dst = d_raster + (size_t)n * F3DG_OUT_CHANNELS * HW + i;
    const size_t slot = (size_t)v * B + b;
    auto gate = [](float r, float g) { return (r >= 0.0f && r <= 1.0f) ? g : 0.0f; };
    auto put = [](float* p, float x, float y, float z, float w) { *reinterpret_cast<float4*>(p) = make_float4(x, y, z, w); };
    if (g_xin) {
        const float* gx = g_xin + slot * 4 * HW + i;
#pragma unroll
        for (int c = 0; c < 3; c++) {
            const float4 r = *reinterpret_cast<const float4*>(src + c * HW);
            const float4 g = *reinterpret_cast<const float4*>(gx + c * HW);
            put(dst + c * HW, gate(r.x, g.x), gate(r.y, g.y), gate(r.z, g.z), gate(r.w, g.w));
        }
        const float4 a = *reinterpret_cast<const float4*>(gx + 3 * HW);
        put(dst + 7 * HW, a.x, a.y, a.z, a.w);
    } else {
#pragma unroll
        for (int c = 0; c < 3; c++) put(dst + c * HW, 0.0f, 0.0f, 0.0f, 0.0f);
        put(dst + 7 * HW, 0.0f, 0.0f, 0.0f, 0.0f);
    }
    put(dst + 3 * HW, 0.0f, 0.0f, 0.0f, 0.0f);
    put(dst + 4 * HW, 0.0f, 0.0f, 0.0f, 0.0f);
    put(dst + 5 * HW, 0.0f, 0.0f, 0.0f, 0.0f);
    if (g_depth) {
        const float4 d = *reinterpret_cast<const float4*>(g_depth + slot * HW + i);
        put(dst + 6 * HW, d.x, d.y, d.z, d.w);
    } else {
        put(dst + 6 * HW, 0.0f, 0.0f, 0.0f, 0.0f);
    }
    put(dst + 8 * HW, 0.0f, 0.0f, 0.0f, 0.0f);
}
} // namespace

extern "C" int f3dg_cycle_inputs_backward(void* stream, int B, int V, int H, int W, const float* raster,
                                          const float* g_xin, const float* g_depth, float* d_raster)
{
    if (B < 0 || V <= 0 || H <= 0 || W <= 0 || !raster || !d_raster) return F3DG_ERR_BAD_ARG;
    if (B == 0) return F3DG_OK;
    const size_t HW = (size_t)H * W;
    if ((HW & 3u) || ((uintptr_t)raster & 15u) || ((uintptr_t)d_raster & 15u) || ((uintptr_t)g_xin & 15u) || ((uintptr_t)g_depth & 15u))
        return F3DG_ERR_BAD_ARG;
    if ((long long)B * V > 65535) return F3DG_ERR_BAD_ARG;          // grid.y
    F3DG_KLAUNCH(cycle_inputs_backward_kernel, dim3((unsigned)((HW / 4 + F3DG_BLOCK - 1) / F3DG_BLOCK), (unsigned)(B * V)),
                 dim3(F3DG_BLOCK), 0, (hipStream_t)stream, HW, B, V, raster, g_xin, g_depth, d_raster);
    F3DG_HIP_CHECK(hipGetLastError());
    return F3DG_OK;
}
