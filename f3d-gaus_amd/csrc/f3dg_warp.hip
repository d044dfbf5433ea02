// f3dg_warp.hip -- depth-based forward warp of source frames into new cameras (the pseudo-target of the settings' w_warping / w_prop,
// config/imagenetgs_256x256_v1.yaml:50-66: threshold, erode_kernel_size, erode_pad_size) and the masked L1 that compares a render with
// it. The reference's release holds no trainer and no warp: the semantics are this project's, stated in include/f3dg.h and DESIGN.md.
//
// forward warp   every (source frame, target camera) pair of a call in ONE launch sequence:
//   warp_fill_kernel      z-buffer = bits of +inf, accumulators = 0
//   warp_zbuffer_kernel   one thread per (pair, source pixel): project, atomicMin of the bits of z (a positive float orders as its bit
//                         pattern) into the up to four target pixels whose bilinear weight reaches the occlusion floor
//   warp_splat_kernel     the same thread, the same projection: a neighbour with z <= zmin + tolerance adds w, w c and w z to the target
//                         pixel's accumulators -- 64-bit integers in units of F3DG_WARP_Q = 2^-24, native atomicAdd on unsigned long long
//                         (two's complement: a negative term wraps to the right sum). Integer sums do not depend on arrival order, so
//                         the outputs are bit-reproducible. Accumulators are plane-major, [pair][C + 2][H W] = (W, C_0.., Z): neighbouring
//                         source pixels land on neighbouring target pixels, so each of the C + 2 atomic wave-instructions of a
//                         contribution covers a few contiguous runs of 8-byte words. The pixel-major layout ([pair][H W][C + 2], one
//                         contribution's atomics in 40 consecutive bytes, every lane on its own 40-byte stride) was measured too:
//                         the launch sequence takes 1.44-1.54 ms with it against 0.67-0.69 ms at 8 x 4 pairs of 256 x 256
//                         (profiles/warp.md).
//   warp_resolve_kernel   one thread per (pair, target pixel): weight, warped, warped_depth, mask (every element assigned)
//   warp_erode_kernel     only with erode >= 3: the k x k minimum of the mask, out-of-image neighbours ignored
//
// The projection runs in float64 on the float32 inputs. Both scatter passes wait on their atomics, not on arithmetic, and float64 puts
// the kernel on the definition's side of the two depth tests and of the floor wherever float32 rounding could flip them; the
// definition itself does not need it (tests/warp_truth.py: its float32 and float64 restatements agree outside a sub-percent margin).
// Target coordinates are range-checked as floating-point numbers before any conversion to int: NaN, +-Inf and +-huge fail the check.
//
// Fixed-point range: a contribution is round-to-nearest(w v / q) with |w v| clamped to F3DG_WARP_VMAX = 2^15 (saturation: |image| and
// depth up to 32768 are exact to q / 2 per contribution; beyond, a contribution saturates). A target pixel receives at most H W
// contributions (one per source pixel), so with H W <= 2^23 (F3DG_ERR_UNSUPPORTED beyond) a sum stays below 2^15 2^24 2^23 = 2^62.
//
// masked L1      masked_l1_fwd_kernel, the two-stage, fixed-order sums of f3dg_tile_sums.h with TERMS = 2; masked_l1_bwd_kernel assigns
//                g m sign(a - b) -- the mould of f3dg_geometry_loss.hip.
#include "f3dg_common.h"
#include "f3dg_tile_sums.h"

#define F3DG_WARP_Q_INV 16777216.0        // 1 / q, q = 2^-24
#define F3DG_WARP_Q (1.0 / F3DG_WARP_Q_INV)
#define F3DG_WARP_VMAX 32768.0
#define F3DG_WARP_MAX_PIXELS (1ll << 23)
#define F3DG_WARP_MAX_C 16
#define F3DG_WARP_MAX_ERODE 15

namespace {

typedef unsigned long long u64;

struct WarpArgs {
    int n_views, C, H, W;
    const float* image;     // [n_src,C,H,W]
    const float* depth;     // [n_src,H,W]
    const float* valid;     // [n_src,H,W] or null
    const float* rel;       // [n_src,n_views,16]
    double fx, fy, z_near, depth_tolerance, occlusion_min_weight;
    unsigned* zbuf;         // [pairs][H W]
    u64* acc;               // [pairs][C + 2][H W]
};

// the footprint of one source pixel in one target camera
struct WarpFoot {
    int x0, y0;             // floor(u), floor(v): in [-1, W - 1] x [-1, H - 1]
    double a, b, z;
};

// Thread (pair, source pixel n) -> its footprint; false when the pixel is not live. `b_src` receives the source frame.
__device__ __forceinline__ bool warp_project(const WarpArgs& A, unsigned pair, int n, unsigned& b_src, WarpFoot& f)
{
    const int HW = A.H * A.W;
    b_src = pair / (unsigned)A.n_views;
    const size_t sn = (size_t)b_src * HW + n;
    if (A.valid && !(A.valid[sn] > 0.0f)) return false;
    const float df = A.depth[sn];
    if (!(df > 0.0f && df <= 3.402823466e+38f)) return false;            // NaN, +Inf, zero and negative depths
    const int i = n % A.W, j = n / A.W;
    const double d = (double)df;
    const double X = ((double)i + 0.5 - A.W / 2.0) / A.fx * d;
    const double Y = ((double)j + 0.5 - A.H / 2.0) / A.fy * d;
    const float* R = A.rel + 16 * (size_t)pair;
    const double x = X * (double)R[0] + Y * (double)R[4] + d * (double)R[8] + (double)R[12];
    const double y = X * (double)R[1] + Y * (double)R[5] + d * (double)R[9] + (double)R[13];
    const double z = X * (double)R[2] + Y * (double)R[6] + d * (double)R[10] + (double)R[14];
    if (!(z > A.z_near)) return false;
    const double u = A.fx * x / z + A.W / 2.0 - 0.5;
    const double v = A.fy * y / z + A.H / 2.0 - 0.5;
    if (!(u > -1.0 && u < (double)A.W && v > -1.0 && v < (double)A.H)) return false;      // (NaN fails every comparison)
    const double fu = floor(u), fv = floor(v);
    f.x0 = (int)fu; f.y0 = (int)fv;
    f.a = u - fu; f.b = v - fv;
    f.z = z;
    return true;
}

// target pixel and bilinear weight of neighbour k = 2 dy + dx; false outside the image or at weight 0
__device__ __forceinline__ bool warp_neighbour(const WarpArgs& A, const WarpFoot& f, int k, int& t, double& w)
{
    const int dx = k & 1, dy = k >> 1;
    const int tx = f.x0 + dx, ty = f.y0 + dy;
    if (tx < 0 || tx >= A.W || ty < 0 || ty >= A.H) return false;
    w = (dx ? f.a : 1.0 - f.a) * (dy ? f.b : 1.0 - f.b);
    t = ty * A.W + tx;
    return w > 0.0;
}

__global__ void __launch_bounds__(F3DG_BLOCK)
warp_fill_kernel(u64 n_acc, u64 n_z, u64* __restrict__ acc, unsigned* __restrict__ zbuf)
{
    const u64 i = (u64)blockIdx.x * F3DG_BLOCK + threadIdx.x;
    if (i < n_acc) acc[i] = 0ull;
    if (i < n_z) zbuf[i] = 0x7F800000u;
}

__global__ void __launch_bounds__(F3DG_BLOCK)
warp_zbuffer_kernel(unsigned blocks_per_pair, WarpArgs A)
{
    const unsigned pair = blockIdx.x / blocks_per_pair;
    const int HW = A.H * A.W;
    const int n = (int)(blockIdx.x - pair * blocks_per_pair) * F3DG_BLOCK + (int)threadIdx.x;
    if (n >= HW) return;
    unsigned b_src;
    WarpFoot f;
    if (!warp_project(A, pair, n, b_src, f)) return;
    const unsigned zbits = __float_as_uint((float)f.z);         // z > z_near >= 0: the bits of a positive float order as the float
    unsigned* zb = A.zbuf + (size_t)pair * HW;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        int t;
        double w;
        if (warp_neighbour(A, f, k, t, w) && w >= A.occlusion_min_weight) atomicMin(zb + t, zbits);
    }
}

// accumulator k (0: W, 1 .. C: colour, C + 1: Z) of target pixel t inside a pair's block: plane-major (see the head of the file)
__device__ __forceinline__ size_t warp_slot(int t, int k, int HW) { return (size_t)k * HW + t; }

// round-to-nearest(v / q) as the two's complement addend of a 64-bit sum; |v| saturates at F3DG_WARP_VMAX
__device__ __forceinline__ u64 warp_fixed(double v)
{
    v = fmin(fmax(v, -F3DG_WARP_VMAX), F3DG_WARP_VMAX);
    return (u64)__double2ll_rn(v * F3DG_WARP_Q_INV);
}

__global__ void __launch_bounds__(F3DG_BLOCK)
warp_splat_kernel(unsigned blocks_per_pair, WarpArgs A)
{
    const unsigned pair = blockIdx.x / blocks_per_pair;
    const int HW = A.H * A.W;
    const int n = (int)(blockIdx.x - pair * blocks_per_pair) * F3DG_BLOCK + (int)threadIdx.x;
    if (n >= HW) return;
    unsigned b_src;
    WarpFoot f;
    if (!warp_project(A, pair, n, b_src, f)) return;
    // the z-buffer holds float32 values: the test compares the float32 z the first pass offered, so the owner of zmin always passes it
    const double zf = (double)(float)f.z;
    const unsigned* zb = A.zbuf + (size_t)pair * HW;
    const int S = A.C + 2;
    u64* acc = A.acc + (size_t)pair * HW * S;
    const float* img = A.image + (size_t)b_src * A.C * HW + n;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        int t;
        double w;
        if (!warp_neighbour(A, f, k, t, w)) continue;
        const double zmin = (double)__uint_as_float(zb[t]);
        if (!(zf <= zmin + A.depth_tolerance)) continue;
        atomicAdd(acc + warp_slot(t, 0, HW), warp_fixed(w));
        for (int c = 0; c < A.C; c++) atomicAdd(acc + warp_slot(t, 1 + c, HW), warp_fixed(w * (double)img[(size_t)c * HW]));
        atomicAdd(acc + warp_slot(t, 1 + A.C, HW), warp_fixed(w * f.z));
    }
}

__global__ void __launch_bounds__(F3DG_BLOCK)
warp_resolve_kernel(unsigned blocks_per_pair, int C, int HW, double threshold, const u64* __restrict__ acc, float* __restrict__ warped,
                    float* __restrict__ mask, float* __restrict__ warped_depth, float* __restrict__ weight)
{
    const unsigned pair = blockIdx.x / blocks_per_pair;
    const int t = (int)(blockIdx.x - pair * blocks_per_pair) * F3DG_BLOCK + (int)threadIdx.x;
    if (t >= HW) return;
    const int S = C + 2;
    const u64* pa = acc + (size_t)pair * HW * S;
    const long long wq = (long long)pa[warp_slot(t, 0, HW)];
    const double ws = (double)wq * F3DG_WARP_Q;
    const bool covered = wq > 0;
    const size_t pt = (size_t)pair * HW + t;
    float* wp = warped + (size_t)pair * C * HW + t;
    for (int c = 0; c < C; c++) wp[(size_t)c * HW] = covered ? (float)((double)(long long)pa[warp_slot(t, 1 + c, HW)] / (double)wq) : 0.0f;
    mask[pt] = ws >= threshold ? 1.0f : 0.0f;
    if (warped_depth) warped_depth[pt] = covered ? (float)((double)(long long)pa[warp_slot(t, 1 + C, HW)] / (double)wq) : 0.0f;
    if (weight) weight[pt] = (float)ws;
}

__global__ void __launch_bounds__(F3DG_BLOCK)
warp_erode_kernel(unsigned blocks_per_pair, int H, int W, int radius, const float* __restrict__ mask_in, float* __restrict__ mask_out)
{
    const unsigned pair = blockIdx.x / blocks_per_pair;
    const int HW = H * W;
    const int t = (int)(blockIdx.x - pair * blocks_per_pair) * F3DG_BLOCK + (int)threadIdx.x;
    if (t >= HW) return;
    const int y = t / W, x = t % W;
    const float* m = mask_in + (size_t)pair * HW;
    const int y0 = max(y - radius, 0), y1 = min(y + radius, H - 1), x0 = max(x - radius, 0), x1 = min(x + radius, W - 1);
    float r = 1.0f;
    for (int yy = y0; yy <= y1; yy++)
        for (int xx = x0; xx <= x1; xx++) r = fminf(r, m[yy * W + xx]);
    mask_out[(size_t)pair * HW + t] = r;
}

// byte offsets of the workspace: accumulators, z-buffer, the mask before erosion
struct WarpLayout {
    size_t acc, zbuf, mask0, total;
    unsigned long long pairs, blocks_per_pair;
};

// false when a size is out of range; `unsupported` then tells a shape the kernels do not cover from a bad argument
bool warp_layout(int n_src, int n_views, int C, int W, int H, WarpLayout& L, bool& unsupported)
{
    unsupported = false;
    if (n_src <= 0 || n_views <= 0 || C <= 0 || W <= 0 || H <= 0) return false;
    const long long HW = (long long)H * W;
    L.pairs = (unsigned long long)n_src * (unsigned long long)n_views;
    L.blocks_per_pair = ((unsigned long long)HW + F3DG_BLOCK - 1) / F3DG_BLOCK;
    // more channels or pixels than the fixed point covers, or a grid (one thread per pixel of a pair; per accumulator word in the fill)
    // beyond 31 bits
    if (C > F3DG_WARP_MAX_C || HW > F3DG_WARP_MAX_PIXELS || L.pairs > 0x7FFFFFFFull || L.pairs * L.blocks_per_pair > 0x7FFFFFFFull ||
        (L.pairs * (unsigned long long)HW * (C + 2) + F3DG_BLOCK - 1) / F3DG_BLOCK > 0x7FFFFFFFull) {
        unsupported = true;
        return false;
    }
    const size_t px = (size_t)L.pairs * (size_t)HW;
    L.acc = 0;
    L.zbuf = px * (size_t)(C + 2) * sizeof(u64);
    L.mask0 = L.zbuf + px * sizeof(unsigned);
    L.total = L.mask0 + px * sizeof(float);
    return true;
}

// ------------------------------------------------------------------------------------------------ masked L1
__global__ void __launch_bounds__(F3DG_TILE_THREADS)
masked_l1_fwd_kernel(TileGrid grid, int C, int H, int W, const float* __restrict__ a, const float* __restrict__ b, const float* __restrict__ mask,
                     float* __restrict__ partials)
{
    __shared__ float s_red[2 * F3DG_TILE_THREADS];
    const int tid = threadIdx.x;
    const TileOfBlock t = tile_of_block(grid);
    const unsigned f = t.frame;
    const int HW = H * W;
    int tx, ty;
    tile_thread(tid, tx, ty);
    const int x = t.x0 + tx, y0 = t.y0 + ty;
    const float* af = a + (size_t)f * C * HW;
    const float* bf = b + (size_t)f * C * HW;
    float acc[2] = { 0.0f, 0.0f };
#pragma unroll
    for (int j = 0; j < F3DG_TILE_H / F3DG_TILE_ROWS; j++) {
        const int y = y0 + j * F3DG_TILE_ROWS;
        if (!(x < W && y < H)) continue;
        const int n = y * W + x;
        const float m = mask[(size_t)f * HW + n];
        for (int c = 0; c < C; c++) acc[0] = acc[0] + m * fabsf(af[(size_t)c * HW + n] - bf[(size_t)c * HW + n]);
        acc[1] = acc[1] + m;
    }
    tile_sums_put(s_red, acc, tid);
    tile_sums_reduce<2>(s_red, tid, partials);
}

__global__ void __launch_bounds__(F3DG_BLOCK)
masked_l1_bwd_kernel(unsigned blocks_per_frame, int C, int HW, const float* __restrict__ a, const float* __restrict__ b,
                     const float* __restrict__ mask, const float* __restrict__ frame_weights, float* __restrict__ dL_da)
{
    unsigned f;
    int n;
    frame_pixel_of_block(blocks_per_frame, f, n);
    if (n >= HW) return;
    const float gm = frame_weights[2 * (size_t)f] * mask[(size_t)f * HW + n];
    const size_t base = (size_t)f * C * HW + n;
    for (int c = 0; c < C; c++) {
        const float d = a[base + (size_t)c * HW] - b[base + (size_t)c * HW];
        dL_da[base + (size_t)c * HW] = gm * (d > 0.0f ? 1.0f : (d < 0.0f ? -1.0f : 0.0f));
    }
}

} // namespace

extern "C" size_t f3dg_forward_warp_workspace_bytes(int n_src, int n_views, int C, int W, int H)
{
    WarpLayout L;
    bool unsupported;
    return warp_layout(n_src, n_views, C, W, H, L, unsupported) ? L.total : 0;
}

extern "C" int f3dg_forward_warp(void* stream, int n_src, int n_views, int C, int H, int W, const float* image, const float* depth,
                                 const float* valid, const float* rel, float fx, float fy, float z_near, float depth_tolerance,
                                 float occlusion_min_weight, float threshold, int erode, void* workspace, size_t workspace_bytes,
                                 float* warped, float* mask, float* warped_depth, float* weight)
{
    if (!image || !depth || !rel || !workspace || !warped || !mask || ((uintptr_t)workspace & 7u)) return F3DG_ERR_BAD_ARG;
    if (!(fx > 0.0f && fx <= 3.402823466e+38f && fy > 0.0f && fy <= 3.402823466e+38f)) return F3DG_ERR_BAD_ARG;
    if (!(z_near >= 0.0f && z_near <= 3.402823466e+38f) || !(depth_tolerance >= 0.0f) || !(occlusion_min_weight >= 0.0f && occlusion_min_weight <= 1.0f) ||
        !(threshold == threshold))
        return F3DG_ERR_BAD_ARG;
    if (erode < 0 || erode > F3DG_WARP_MAX_ERODE || (erode > 0 && !(erode & 1))) return F3DG_ERR_BAD_ARG;
    WarpLayout L;
    bool unsupported;
    if (!warp_layout(n_src, n_views, C, W, H, L, unsupported)) return unsupported ? F3DG_ERR_UNSUPPORTED : F3DG_ERR_BAD_ARG;
    if (workspace_bytes < L.total) return F3DG_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    char* ws = (char*)workspace;
    const int HW = H * W;
    u64* acc = (u64*)(ws + L.acc);
    unsigned* zbuf = (unsigned*)(ws + L.zbuf);
    float* mask0 = (float*)(ws + L.mask0);
    const u64 n_z = L.pairs * (u64)HW, n_acc = n_z * (u64)(C + 2);
    const unsigned bpp = (unsigned)L.blocks_per_pair;
    const unsigned grid = (unsigned)(L.pairs * L.blocks_per_pair);       // 31 bits: warp_layout
    const WarpArgs A = { n_views, C, H, W, image, depth, valid, rel, (double)fx, (double)fy, (double)z_near, (double)depth_tolerance,
                         (double)occlusion_min_weight, zbuf, acc };
    F3DG_KLAUNCH(warp_fill_kernel, dim3((unsigned)((n_acc + F3DG_BLOCK - 1) / F3DG_BLOCK)), dim3(F3DG_BLOCK), 0, s, n_acc, n_z, acc, zbuf);
    F3DG_HIP_CHECK(hipGetLastError());
    F3DG_KLAUNCH(warp_zbuffer_kernel, dim3(grid), dim3(F3DG_BLOCK), 0, s, bpp, A);
    F3DG_HIP_CHECK(hipGetLastError());
    F3DG_KLAUNCH(warp_splat_kernel, dim3(grid), dim3(F3DG_BLOCK), 0, s, bpp, A);
    F3DG_HIP_CHECK(hipGetLastError());
    const bool eroding = erode >= 3;
    F3DG_KLAUNCH(warp_resolve_kernel, dim3(grid), dim3(F3DG_BLOCK), 0, s, bpp, C, HW, (double)threshold, (const u64*)acc, warped,
                 eroding ? mask0 : mask, warped_depth, weight);
    F3DG_HIP_CHECK(hipGetLastError());
    if (eroding) {
        F3DG_KLAUNCH(warp_erode_kernel, dim3(grid), dim3(F3DG_BLOCK), 0, s, bpp, H, W, erode / 2, (const float*)mask0, mask);
        F3DG_HIP_CHECK(hipGetLastError());
    }
    return F3DG_OK;
}

extern "C" size_t f3dg_masked_l1_partials_bytes(int n_frames, int C, int W, int H)
{
    return C > 0 ? tile_partials_bytes<2>(n_frames, W, H, (long long)C * H * W) : 0;
}

extern "C" int f3dg_masked_l1_forward(void* stream, int n_frames, int C, int H, int W, const float* a, const float* b, const float* mask,
                                      float* partials, size_t partials_bytes, float* frame_sums)
{
    if (n_frames <= 0 || C <= 0 || H <= 0 || W <= 0 || !a || !b || !mask || !partials || !frame_sums) return F3DG_ERR_BAD_ARG;
    TileGrid g;
    unsigned blocks;
    if (!tile_grid(n_frames, W, H, (long long)C * H * W, g, blocks)) return F3DG_ERR_UNSUPPORTED;
    if (partials_bytes < tile_partials_bytes<2>(blocks)) return F3DG_ERR_WORKSPACE;
    F3DG_KLAUNCH(masked_l1_fwd_kernel, dim3(blocks), dim3(F3DG_TILE_THREADS), 0, (hipStream_t)stream, g, C, H, W, a, b, mask, partials);
    F3DG_HIP_CHECK(hipGetLastError());
    return tile_frame_sums<2>((hipStream_t)stream, n_frames, g, partials, frame_sums);
}

extern "C" int f3dg_masked_l1_backward(void* stream, int n_frames, int C, int H, int W, const float* a, const float* b, const float* mask,
                                       const float* frame_weights, float* dL_da)
{
    if (n_frames <= 0 || C <= 0 || H <= 0 || W <= 0 || !a || !b || !mask || !frame_weights || !dL_da) return F3DG_ERR_BAD_ARG;
    TileGrid g;
    unsigned blocks;
    if (!tile_grid(n_frames, W, H, (long long)C * H * W, g, blocks)) return F3DG_ERR_UNSUPPORTED;
    unsigned per_frame;
    if (!frame_pixel_grid(n_frames, H, W, per_frame, blocks)) return F3DG_ERR_UNSUPPORTED;
    F3DG_KLAUNCH(masked_l1_bwd_kernel, dim3(blocks), dim3(F3DG_BLOCK), 0, (hipStream_t)stream, per_frame, C, H * W, a, b, mask, frame_weights,
                 dL_da);
    F3DG_HIP_CHECK(hipGetLastError());
    return F3DG_OK;
}
