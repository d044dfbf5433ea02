// f3dg_geometry_loss.hip -- the trainer's geometry terms on the nine raster planes of a batch of frames: depth-normal consistency,
// distortion, depth, normal and alpha (the reference's w_depth_normal / w_distortion / w_depth / w_normal / w_alpha,
// config/imagenetgs_256x256_v1.yaml:50-66) as ONE forward kernel plus a tiny fixed-order second-stage sum, and dL/draster of all five
// as ONE backward kernel. include/f3dg.h has the contract.
//
// Written as torch operations on the maps render_views returns, the same terms materialise normal_world and depth_normal
// ([F,3,H,W] each), run about fifteen elementwise kernels with their autograd graph and then f3dg_render_epilogue_backward on two
// full-size cotangent maps. Here the two derived maps exist in registers only: N = normal_world and D = depth_normal of a pixel are
// formed with the epilogue's own expressions (f3dg_epilogue.h), so the terms are those of the maps f3dg_render_epilogue_view writes.
//
// forward   the two-stage, fixed-order sums of f3dg_tile_sums.h with TERMS = 5: a workgroup per 32 x 16 pixel tile of one frame, two
//           pixels per thread.
// backward  one thread per (frame, pixel), 256 consecutive pixels of a frame per workgroup, as epilogue_backward_kernel: channels 3..5
//           from this pixel's own N, D and target; channel 6 as the gather over the up to four interior axial neighbours whose depth
//           normal reads this pixel's depth, each neighbour's cotangent -W0 w(q) N(q) recomputed from the raster. Nothing is saved by
//           the forward, no atomics, every element of dL_draster is assigned.
#include "f3dg_common.h"
#include "f3dg_epilogue.h"
#include "f3dg_tile_sums.h"

#define F3DG_GEOM_TERMS 5

namespace {

// what both kernels read (by value)
struct GeomArgs {
    int H, W;
    const float* raster;            // [F,9,H,W]
    const float* world_view;        // [F,16]
    float fx, fy;
    int flags;
    const float* depth_target;      // [F,H,W] or null
    const float* normal_target;     // [F,3,H,W] or null
    const float* alpha_target;      // [F,H,W] or null
    const float* mask;              // [F,H,W] or null (= 1)
};

// c2w = inverse(world_view^T) of frame f, as epilogue_kernel<true> forms it (one thread)
__device__ void geom_camera(const float* __restrict__ world_view, size_t f, float* c2w)
{
    float t[16];
    for (int r = 0; r < 4; r++)
        for (int c = 0; c < 4; c++) t[4 * r + c] = world_view[16 * f + 4 * c + r];
    invert4x4(t, c2w);
}

// n^ = normalize(raster[3:6]) of pixel n (camera frame) and N = c2w[:3,:3] n^ (normal_world), as epilogue_kernel writes it
struct GeomNormal { float na, nb, nc, N0, N1, N2; };
__device__ __forceinline__ GeomNormal geom_normal(const float* __restrict__ ras, const float* Cw, int HW, int n)
{
    const float a = ras[3 * HW + n], b = ras[4 * HW + n], c = ras[5 * HW + n];
    const float nrm = fmaxf(sqrtf(a * a + b * b + c * c), 1e-12f);
    GeomNormal r;
    r.na = a / nrm; r.nb = b / nrm; r.nc = c / nrm;
    r.N0 = Cw[0] * r.na + Cw[1] * r.nb + Cw[2] * r.nc;
    r.N1 = Cw[4] * r.na + Cw[5] * r.nb + Cw[6] * r.nc;
    r.N2 = Cw[8] * r.na + Cw[9] * r.nb + Cw[10] * r.nc;
    return r;
}

__device__ __forceinline__ bool geom_interior(int H, int W, int y, int x) { return x >= 1 && x < W - 1 && y >= 1 && y < H - 1; }

// D = depth_normal of pixel (y, x), as epilogue_kernel writes it: 0 on the border
__device__ __forceinline__ void geom_depth_normal(const float* __restrict__ dep, const float* Cw, int H, int W, float ax, float bx, float ay,
                                                  float by, int y, int x, float& D0, float& D1, float& D2)
{
    D0 = 0.0f; D1 = 0.0f; D2 = 0.0f;
    if (geom_interior(H, W, y, x)) {
        const EpilogueCross k = epilogue_cross(dep, Cw, W, ax, bx, ay, by, y, x);
        const float nrm = fmaxf(sqrtf(k.cx * k.cx + k.cy * k.cy + k.cz * k.cz), 1e-12f);
        D0 = k.cx / nrm; D1 = k.cy / nrm; D2 = k.cz / nrm;
    }
}

__device__ __forceinline__ float geom_sign(float d) { return d > 0.0f ? 1.0f : (d < 0.0f ? -1.0f : 0.0f); }

__global__ void __launch_bounds__(F3DG_TILE_THREADS)
geom_fwd_kernel(TileGrid grid, GeomArgs a, float* __restrict__ partials)
{
    __shared__ float s_c2w[16];
    __shared__ float s_red[F3DG_GEOM_TERMS * F3DG_TILE_THREADS];
    const int tid = threadIdx.x;
    const TileOfBlock t = tile_of_block(grid);
    const unsigned f = t.frame;
    if (tid == 0) geom_camera(a.world_view, f, s_c2w);
    __syncthreads();
    const int H = a.H, W = a.W, HW = H * W;
    const float* ras = a.raster + (size_t)f * F3DG_OUT_CHANNELS * HW;
    const float* dep = ras + 6 * HW;
    const float* Cw = s_c2w;
    const float ax = 1.0f / a.fx, bx = -(W / 2.0f) / a.fx, ay = 1.0f / a.fy, by = -(H / 2.0f) / a.fy;
    int tx, ty;
    tile_thread(tid, tx, ty);
    const int x = t.x0 + tx, y0 = t.y0 + ty;
    float acc[F3DG_GEOM_TERMS] = { 0.0f, 0.0f, 0.0f, 0.0f, 0.0f };
#pragma unroll
    for (int j = 0; j < F3DG_TILE_H / F3DG_TILE_ROWS; j++) {
        const int y = y0 + j * F3DG_TILE_ROWS;
        if (!(x < W && y < H)) continue;
        const int n = y * W + x;
        const size_t fn = (size_t)f * HW + n;
        const GeomNormal nn = geom_normal(ras, Cw, HW, n);
        float D0, D1, D2;
        geom_depth_normal(dep, Cw, H, W, ax, bx, ay, by, y, x, D0, D1, D2);
        const float alpha = ras[7 * HW + n];
        const float w = (a.flags & F3DG_GEOM_ALPHA_WEIGHT) ? alpha : 1.0f;
        const float m = a.mask ? a.mask[fn] : 1.0f;
        acc[0] = acc[0] + w * (1.0f - (nn.N0 * D0 + nn.N1 * D1 + nn.N2 * D2));
        acc[1] = acc[1] + ras[8 * HW + n];
        if (a.depth_target) acc[2] = acc[2] + m * fabsf(dep[n] - a.depth_target[fn]);
        if (a.normal_target) {
            const float* nt = a.normal_target + (size_t)f * 3 * HW + n;
            acc[3] = acc[3] + m * (1.0f - (nn.na * nt[0] + nn.nb * nt[HW] + nn.nc * nt[2 * HW]));
        }
        if (a.alpha_target) acc[4] = acc[4] + fabsf(alpha - a.alpha_target[fn]);
    }
    tile_sums_put(s_red, acc, tid);
    tile_sums_reduce<F3DG_GEOM_TERMS>(s_red, tid, partials);
}

// dL/draster for L = sum_f sum_k frame_weights[f,k] frame_sums[f,k]. A term whose weight is exactly 0 is not evaluated (its data
// cannot reach the gradient, whatever it holds), as a term whose target is null.
__global__ void __launch_bounds__(F3DG_BLOCK)
geom_bwd_kernel(unsigned blocks_per_frame, GeomArgs a, const float* __restrict__ frame_weights, float* __restrict__ dL_draster)
{
    __shared__ float s_c2w[16];
    unsigned f;
    int n;
    frame_pixel_of_block(blocks_per_frame, f, n);
    const int H = a.H, W = a.W, HW = H * W;
    if (threadIdx.x == 0) geom_camera(a.world_view, f, s_c2w);
    __syncthreads();
    if (n >= HW) return;
    const int y = n / W, x = n % W;
    const float* ras = a.raster + (size_t)f * F3DG_OUT_CHANNELS * HW;
    const float* dep = ras + 6 * HW;
    float* dpix = dL_draster + (size_t)f * F3DG_OUT_CHANNELS * HW;
    const float* Cw = s_c2w;
    const float* fw = frame_weights + F3DG_GEOM_TERMS * (size_t)f;
    const float W0 = fw[0], W1 = fw[1], W2 = fw[2], W3 = fw[3], W4 = fw[4];
    const bool by_alpha = (a.flags & F3DG_GEOM_ALPHA_WEIGHT) != 0;
    const size_t fn = (size_t)f * HW + n;
    const float m = a.mask ? a.mask[fn] : 1.0f;
    const float alpha = ras[7 * HW + n];
    const float ax = 1.0f / a.fx, bx = -(W / 2.0f) / a.fx, ay = 1.0f / a.fy, by = -(H / 2.0f) / a.fy;

    // channels 3..5: the cotangent of n^ from terms 0 (through N = c2w[:3,:3] n^) and 3, then the normalisation
    float g0 = 0.0f, g1 = 0.0f, g2 = 0.0f;
    if (W0 != 0.0f) {
        float D0, D1, D2;
        geom_depth_normal(dep, Cw, H, W, ax, bx, ay, by, y, x, D0, D1, D2);
        const float c = -(W0 * (by_alpha ? alpha : 1.0f));
        const float w0 = c * D0, w1 = c * D1, w2 = c * D2;              // dL/dN
        g0 = Cw[0] * w0 + Cw[4] * w1 + Cw[8] * w2;
        g1 = Cw[1] * w0 + Cw[5] * w1 + Cw[9] * w2;
        g2 = Cw[2] * w0 + Cw[6] * w1 + Cw[10] * w2;
    }
    if (a.normal_target && W3 != 0.0f) {
        const float* nt = a.normal_target + (size_t)f * 3 * HW + n;
        const float c = W3 * m;
        g0 = g0 - c * nt[0]; g1 = g1 - c * nt[HW]; g2 = g2 - c * nt[2 * HW];
    }
    normalize3_backward(ras[3 * HW + n], ras[4 * HW + n], ras[5 * HW + n], g0, g1, g2);

    // channel 6: the gather of term 0 (epilogue_backward_kernel's, with the centre's cotangent -W0 w(q) N(q) formed here), then term 2
    float gd = 0.0f;
    if (W0 != 0.0f) {
        float rx, ry, rz;
        epilogue_ray(Cw, ax, bx, ay, by, y, x, rx, ry, rz);
        // the cotangent of centre (cy, cx) taken back to its difference vectors: along_rows selects dL/de (else dL/dg), dotted with this ray
        auto term = [&](int cy, int cx, bool along_rows) -> float {
            if (!geom_interior(H, W, cy, cx)) return 0.0f;
            const EpilogueCross k = epilogue_cross(dep, Cw, W, ax, bx, ay, by, cy, cx);
            const int q = cy * W + cx;
            const GeomNormal nq = geom_normal(ras, Cw, HW, q);
            const float c = -(W0 * (by_alpha ? ras[7 * HW + q] : 1.0f));
            float w0 = c * nq.N0, w1 = c * nq.N1, w2 = c * nq.N2;      // dL/dD(q)
            normalize3_backward(k.cx, k.cy, k.cz, w0, w1, w2);
            float p0, p1, p2;
            if (along_rows) { p0 = k.gy * w2 - k.gz * w1; p1 = k.gz * w0 - k.gx * w2; p2 = k.gx * w1 - k.gy * w0; }      // g x w
            else            { p0 = w1 * k.ez - w2 * k.ey; p1 = w2 * k.ex - w0 * k.ez; p2 = w0 * k.ey - w1 * k.ex; }      // w x e
            return rx * p0 + ry * p1 + rz * p2;
        };
        gd = term(y - 1, x, true);
        gd -= term(y + 1, x, true);
        gd += term(y, x - 1, false);
        gd -= term(y, x + 1, false);
    }
    if (a.depth_target && W2 != 0.0f) gd = (W2 * m) * geom_sign(dep[n] - a.depth_target[fn]) + gd;

    dpix[n] = 0.0f; dpix[HW + n] = 0.0f; dpix[2 * HW + n] = 0.0f;
    dpix[3 * HW + n] = g0; dpix[4 * HW + n] = g1; dpix[5 * HW + n] = g2;
    dpix[6 * HW + n] = gd;
    dpix[7 * HW + n] = (a.alpha_target && W4 != 0.0f) ? W4 * geom_sign(alpha - a.alpha_target[fn]) : 0.0f;
    dpix[8 * HW + n] = W1;
}

} // namespace

extern "C" size_t f3dg_geometry_loss_partials_bytes(int n_frames, int W, int H)
{
    return tile_partials_bytes<F3DG_GEOM_TERMS>(n_frames, W, H, 9ll * H * W);
}

extern "C" int f3dg_geometry_loss_forward(void* stream, int n_frames, int H, int W, const float* raster, const float* world_view,
                                          float fx, float fy, int flags, const float* depth_target, const float* normal_target,
                                          const float* alpha_target, const float* mask, float* partials, size_t partials_bytes,
                                          float* frame_sums)
{
    if (n_frames <= 0 || H <= 0 || W <= 0 || !raster || !world_view || !frame_sums || !partials) return F3DG_ERR_BAD_ARG;
    if (flags & ~F3DG_GEOM_ALPHA_WEIGHT) return F3DG_ERR_BAD_ARG;
    TileGrid g;
    unsigned blocks;
    if (!tile_grid(n_frames, W, H, 9ll * H * W, g, blocks)) return F3DG_ERR_UNSUPPORTED;
    if (partials_bytes < tile_partials_bytes<F3DG_GEOM_TERMS>(blocks)) return F3DG_ERR_WORKSPACE;
    const GeomArgs a = { H, W, raster, world_view, fx, fy, flags, depth_target, normal_target, alpha_target, mask };
    F3DG_KLAUNCH(geom_fwd_kernel, dim3(blocks), dim3(F3DG_TILE_THREADS), 0, (hipStream_t)stream, g, a, partials);
    F3DG_HIP_CHECK(hipGetLastError());
    return tile_frame_sums<F3DG_GEOM_TERMS>((hipStream_t)stream, n_frames, g, partials, frame_sums);
}

extern "C" int f3dg_geometry_loss_backward(void* stream, int n_frames, int H, int W, const float* raster, const float* world_view,
                                           float fx, float fy, int flags, const float* depth_target, const float* normal_target,
                                           const float* alpha_target, const float* mask, const float* frame_weights, float* dL_draster)
{
    if (n_frames <= 0 || H <= 0 || W <= 0 || !raster || !world_view || !frame_weights || !dL_draster) return F3DG_ERR_BAD_ARG;
    if (flags & ~F3DG_GEOM_ALPHA_WEIGHT) return F3DG_ERR_BAD_ARG;
    TileGrid g;
    unsigned blocks;
    if (!tile_grid(n_frames, W, H, 9ll * H * W, g, blocks)) return F3DG_ERR_UNSUPPORTED;
    unsigned per_frame;
    if (!frame_pixel_grid(n_frames, H, W, per_frame, blocks)) return F3DG_ERR_UNSUPPORTED;
    const GeomArgs a = { H, W, raster, world_view, fx, fy, flags, depth_target, normal_target, alpha_target, mask };
    F3DG_KLAUNCH(geom_bwd_kernel, dim3(blocks), dim3(F3DG_BLOCK), 0, (hipStream_t)stream, per_frame, a, frame_weights, dL_draster);
    F3DG_HIP_CHECK(hipGetLastError());
    return F3DG_OK;
}
