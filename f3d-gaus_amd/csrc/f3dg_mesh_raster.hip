// f3dg_mesh_raster.hip -- a triangle mesh drawn from the renderer's cameras: exact integer coverage on a 1/256-pixel lattice, a 64-bit
// z-buffer (bits(depth) << 32 | face under an unsigned atomicMin), perspective-correct weights in float64. The semantics are this
// project's, stated in include/f3dg.h and DESIGN.md section 3g-quinquies; tests/mesh_raster_truth.py restates them in float64 numpy.
// Integer atomics only, no float atomics: every output is a function of the input alone. No thread waits for another thread's write,
// and every loop is bounded by a box of pixel centres or by the queue's length.
//   raster_fill_kernel     the keys to all ones (empty), the header to zero
//   raster_small_kernel    one thread per (view, face): the range check of its ids BEFORE anything is indexed with them, projection,
//                          snapping, the class of the pair, the box of pixel centres; an empty box ends there, a box of at most 64
//                          centres is walked by the thread, a larger one is queued (an integer atomicAdd hands out the slot; the
//                          atomicMin on the keys erases the arrival order)
//   raster_large_kernel    a fixed grid that reads the queue's length from the header: the 64 lanes of a wave stride over every queued
//                          box of at most 512 centres, the 256 threads of a workgroup over every larger one (bit 31 of the queue entry
//                          says which), each lane setting the triangle up for itself
//   raster_resolve_kernel  one thread per pixel: the winner's weights again by raster_setup / raster_eval, the functions the scatter
//                          used, and every output
// A face with an id out of range sets hdr->bad in raster_small_kernel; the later kernels return at once then, so a refused mesh writes
// no output.
#include "f3dg_common.h"
#include "f3dg_mesh_project.h"

namespace {

typedef unsigned int u32;
typedef unsigned long long u64;
typedef long long i64;

#define RAST_SMALL 64u              // most pixel centres of a box that one thread walks
#define RAST_WAVE 512u              // most pixel centres of a box that one wave walks; a workgroup beyond
#define RAST_LARGE_GRID 1024u       // workgroups of raster_large_kernel
#define RAST_WG_FLAG 0x80000000u    // queue entry: the box is a workgroup's
#define RAST_GUARD 16384.0
#define RAST_MAX_C 8
#define RAST_EMPTY 0xFFFFFFFFFFFFFFFFull

enum { RAST_OK = 0, RAST_NEAR = 1, RAST_GUARDED = 2, RAST_DEGENERATE = 3, RAST_CULLED = 4, RAST_BAD = 5 };

struct RasterHeader {               // first 256 bytes of the workspace
    u32 bad;                        // 1: a face holds an id outside [0, N)
    u32 n_large;                    // queued pairs
    u32 cls[5];                     // pairs per class: rasterised, near / non-finite, guard band, degenerate, culled
    u32 covered;                    // pixels with a face
    u32 reserved[56];
};
static_assert(sizeof(RasterHeader) == 256, "the header is the first 256 bytes");

struct RasterLayout { size_t header, keys, queue, total; };

inline size_t rast_align256(size_t b) { return (b + 255) / 256 * 256; }

RasterLayout raster_layout(i64 V, i64 F, i64 H, i64 W)
{
    RasterLayout L;
    L.header = 0;
    L.keys = sizeof(RasterHeader);
    L.queue = L.keys + rast_align256((size_t)(V * H * W) * 8);
    L.total = L.queue + rast_align256((size_t)(V * F) * 4);
    return L;
}

// F3DG_OK, or why the sizes are refused
int raster_check_sizes(i64 V, i64 F, i64 H, i64 W)
{
    if (V <= 0 || F < 0 || H <= 0 || W <= 0) return F3DG_ERR_BAD_ARG;
    if (H > 16384 || W > 16384 || F >= (1ll << 31) || V >= (1ll << 31)) return F3DG_ERR_UNSUPPORTED;
    if (V * H * W >= (1ll << 31) || V * F >= (1ll << 31)) return F3DG_ERR_UNSUPPORTED;       // (each product is below 2^62)
    return F3DG_OK;
}

struct RasterArgs {                 // by value to every kernel
    const float* vertices;
    const void* faces;
    const float* world_views;
    const float* attrs;
    double fx, fy, z_near, half_w, half_h;      // half_w = (double)W / 2
    u32 N, F, V, H, W;
    int cull, C, faces_int32;
};

struct RasterTri {                  // a rasterised pair, set up
    int U[3], Vv[3];                // the snapped corners in the ORIENTED order o
    double q[3];                    // 1 / z of the face's OWN corners
    double absA;
    u32 id[3];                      // the face's own ids
    int swapped;                    // o = (0, 2, 1)
    int i0, i1, j0, j1;             // the box of pixel centres, cut to the image (empty when i1 < i0 or j1 < j0)
};

__device__ __forceinline__ int rast_ceil256(int a) { return (a + 255) >> 8; }       // ceil(a / 256), a of either sign
__device__ __forceinline__ int rast_floor256(int a) { return a >> 8; }              // floor(a / 256)

// The class of pair (view, f) and, for RAST_OK, its set-up triangle. Nothing is indexed with an id before all three are in range.
__device__ int raster_setup(const RasterArgs& A, u32 view, u32 f, RasterTri& T)
{
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const i64 id = A.faces_int32 ? (i64)((const int*)A.faces)[3 * (size_t)f + k] : ((const i64*)A.faces)[3 * (size_t)f + k];
        ok = ok && id >= 0 && id < (i64)A.N;
        T.id[k] = (u32)id;
    }
    if (!ok) return RAST_BAD;
    if (T.id[0] == T.id[1] || T.id[1] == T.id[2] || T.id[0] == T.id[2]) return RAST_DEGENERATE;
    const float* m = A.world_views + 16 * (size_t)view;
    double u[3], v[3];
    bool near = false, guard = false;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const float* p = A.vertices + 3 * (size_t)T.id[k];
        const double X = (double)p[0], Y = (double)p[1], Z = (double)p[2];
        double x, y, z;
        if (f3dg_mesh_project(X, Y, Z, m, A.fx, A.fy, A.half_w, A.half_h, A.z_near, x, y, z, u[k], v[k])) near = true;
        guard = guard || !(fabs(u[k]) <= RAST_GUARD && fabs(v[k]) <= RAST_GUARD);
        T.q[k] = 1.0 / z;
    }
    if (near) return RAST_NEAR;
    if (guard) return RAST_GUARDED;
    int Us[3], Vs[3];
#pragma unroll
    for (int k = 0; k < 3; k++) { Us[k] = (int)rint(256.0 * u[k]); Vs[k] = (int)rint(256.0 * v[k]); }       // |.| <= 2^22
    const i64 area = (i64)(Us[1] - Us[0]) * (i64)(Vs[2] - Vs[0]) - (i64)(Vs[1] - Vs[0]) * (i64)(Us[2] - Us[0]);
    if (area == 0) return RAST_DEGENERATE;
    if ((A.cull == F3DG_RASTER_CULL_BACK && area > 0) || (A.cull == F3DG_RASTER_CULL_FRONT && area < 0)) return RAST_CULLED;
    T.swapped = area < 0;
    T.absA = (double)(area < 0 ? -area : area);
    T.U[0] = Us[0]; T.Vv[0] = Vs[0];
    T.U[1] = T.swapped ? Us[2] : Us[1]; T.Vv[1] = T.swapped ? Vs[2] : Vs[1];
    T.U[2] = T.swapped ? Us[1] : Us[2]; T.Vv[2] = T.swapped ? Vs[1] : Vs[2];
    const int umin = min(Us[0], min(Us[1], Us[2])), umax = max(Us[0], max(Us[1], Us[2]));
    const int vmin = min(Vs[0], min(Vs[1], Vs[2])), vmax = max(Vs[0], max(Vs[1], Vs[2]));
    T.i0 = max(rast_ceil256(umin), 0); T.i1 = min(rast_floor256(umax), (int)A.W - 1);
    T.j0 = max(rast_ceil256(vmin), 0); T.j1 = min(rast_floor256(vmax), (int)A.H - 1);
    return RAST_OK;
}

__device__ __forceinline__ u32 raster_box(const RasterTri& T)
{
    return (T.i1 < T.i0 || T.j1 < T.j0) ? 0u : (u32)(T.i1 - T.i0 + 1) * (u32)(T.j1 - T.j0 + 1);       // at most 2^28
}

// Is the centre of pixel (i, j) covered, and if so the weights beta[3] of the face's own corners and the depth
__device__ __forceinline__ bool raster_eval(const RasterTri& T, int i, int j, double beta[3], float& depth)
{
    const i64 Px = 256ll * i, Py = 256ll * j;
    i64 E[3];
    bool in = true;
#pragma unroll
    for (int e = 0; e < 3; e++) {                           // edge e runs from oriented corner e to e + 1
        const int a = e, b = (e + 1) % 3;
        const i64 du = (i64)(T.U[b] - T.U[a]), dv = (i64)(T.Vv[b] - T.Vv[a]);
        E[e] = du * (Py - (i64)T.Vv[a]) - dv * (Px - (i64)T.U[a]);
        in = in && (E[e] > 0 || (E[e] == 0 && (dv > 0 || (dv == 0 && du < 0))));
    }
    if (!in) return false;
    // oriented corner 0 / 1 / 2 is opposite edge 1 / 2 / 0; own corners 1 and 2 are oriented 2 and 1 when swapped
    const double w0 = (double)E[1], wa = (double)E[2], wb = (double)E[0];
    const double l0 = w0 / T.absA, l1 = (T.swapped ? wb : wa) / T.absA, l2 = (T.swapped ? wa : wb) / T.absA;
    const double t0 = l0 * T.q[0], t1 = l1 * T.q[1], t2 = l2 * T.q[2];
    const double D = (t0 + t1) + t2;
    depth = (float)(1.0 / D);
    beta[0] = t0 / D; beta[1] = t1 / D; beta[2] = t2 / D;
    return true;
}

__device__ __forceinline__ void raster_put(const RasterTri& T, u32 f, int i, int j, u64* __restrict__ keys_view, u32 W)
{
    double beta[3];
    float depth;
    if (!raster_eval(T, i, j, beta, depth)) return;
    const u64 key = (u64)__float_as_uint(depth) << 32 | (u64)f;
    u64* slot = keys_view + (size_t)j * W + (size_t)i;      // 0 <= i < W, 0 <= j < H: the box was cut to the image
    atomicMin(slot, key);
}

__global__ void __launch_bounds__(F3DG_BLOCK)
raster_fill_kernel(u64* __restrict__ keys, u32 n, RasterHeader* __restrict__ hdr)
{
    const u32 t = blockIdx.x * F3DG_BLOCK + threadIdx.x;
    if (t < n) keys[t] = RAST_EMPTY;
    if (t < 64u) reinterpret_cast<u32*>(hdr)[t] = 0u;
}

__global__ void __launch_bounds__(F3DG_BLOCK)
raster_small_kernel(RasterArgs A, u64* __restrict__ keys, u32* __restrict__ queue, RasterHeader* __restrict__ hdr)
{
    const u32 pair = blockIdx.x * F3DG_BLOCK + threadIdx.x;             // view * F + face, below V F < 2^31
    int cls = -1;
    if (pair < A.V * A.F) {
        const u32 view = pair / A.F, f = pair % A.F;
        RasterTri T;
        cls = raster_setup(A, view, f, T);
        if (cls == RAST_OK) {
            const u32 n = raster_box(T);
            if (n > RAST_SMALL) {
                const u32 slot = atomicAdd(&hdr->n_large, 1u);
                if (slot < A.V * A.F) queue[slot] = pair | (n > RAST_WAVE ? RAST_WG_FLAG : 0u);       // (always: one slot per pair)
            } else if (n > 0u) {
                u64* kv = keys + (size_t)view * A.H * A.W;
                for (int j = T.j0; j <= T.j1; j++)
                    for (int i = T.i0; i <= T.i1; i++) raster_put(T, f, i, j, kv, A.W);
            }
        } else if (cls == RAST_BAD) {
            atomicOr(&hdr->bad, 1u);
        }
    }
#pragma unroll
    for (int c = 0; c < 5; c++) {
        const u64 m = __ballot(cls == c);
        if ((threadIdx.x & 63u) == 0u && m) atomicAdd(&hdr->cls[c], (u32)__popcll(m));
    }
}

// the lanes [lane, lanes) of a wave or a workgroup over the box of queue entry e
__device__ __forceinline__ void raster_large_one(const RasterArgs& A, u32 e, u32 lane, u32 lanes, u64* __restrict__ keys)
{
    const u32 pair = e & ~RAST_WG_FLAG;
    if (pair >= A.V * A.F) return;
    const u32 view = pair / A.F, f = pair % A.F;
    RasterTri T;
    if (raster_setup(A, view, f, T) != RAST_OK) return;     // (not the pair that was queued)
    const u32 n = raster_box(T), bw = (u32)(T.i1 - T.i0 + 1);
    u64* kv = keys + (size_t)view * A.H * A.W;
    for (u32 t = lane; t < n; t += lanes) raster_put(T, f, T.i0 + (int)(t % bw), T.j0 + (int)(t / bw), kv, A.W);
}

__global__ void __launch_bounds__(F3DG_BLOCK)
raster_large_kernel(RasterArgs A, u64* __restrict__ keys, const u32* __restrict__ queue, const RasterHeader* __restrict__ hdr)
{
    if (hdr->bad) return;
    const u32 total = A.V * A.F;
    const u32 n_large = hdr->n_large < total ? hdr->n_large : total;
    const u32 wave = blockIdx.x * (F3DG_BLOCK / 64u) + (threadIdx.x >> 6), waves = gridDim.x * (F3DG_BLOCK / 64u);
    for (u32 b = wave; b < n_large; b += waves) {           // a wave per box of at most RAST_WAVE centres
        const u32 e = queue[b];
        if (!(e & RAST_WG_FLAG)) raster_large_one(A, e, threadIdx.x & 63u, 64u, keys);
    }
    for (u32 b = blockIdx.x; b < n_large; b += gridDim.x) { // a workgroup per larger box
        const u32 e = queue[b];
        if (e & RAST_WG_FLAG) raster_large_one(A, e, threadIdx.x, F3DG_BLOCK, keys);
    }
}

__global__ void __launch_bounds__(F3DG_BLOCK)
raster_resolve_kernel(RasterArgs A, const u64* __restrict__ keys, RasterHeader* __restrict__ hdr, int* __restrict__ face_id,
                      float* __restrict__ depth_out, float* __restrict__ bary, float* __restrict__ attrs_out)
{
    if (hdr->bad) return;
    const u32 hw = A.H * A.W;
    const u32 t = blockIdx.x * F3DG_BLOCK + threadIdx.x;    // view * H W + pixel, below V H W < 2^31
    bool hit = false;
    if (t < A.V * hw) {
        const u32 view = t / hw, pix = t % hw;
        const u64 key = keys[t];
        const u32 f = (u32)(key & 0xFFFFFFFFull);
        double beta[3] = { 0.0, 0.0, 0.0 };
        float depth = 0.0f;
        RasterTri T;
        T.id[0] = T.id[1] = T.id[2] = 0u;
        hit = key != RAST_EMPTY && f < A.F && raster_setup(A, view, f, T) == RAST_OK &&
              raster_eval(T, (int)(pix % A.W), (int)(pix / A.W), beta, depth);
        face_id[t] = hit ? (int)f : -1;
        depth_out[t] = hit ? depth : 0.0f;
#pragma unroll
        for (int k = 0; k < 3; k++) bary[((size_t)view * 3 + k) * hw + pix] = hit ? (float)beta[k] : 0.0f;
        if (A.attrs) {
            for (int c = 0; c < A.C; c++) {
                float a = 0.0f;
                if (hit) {
                    const double a0 = (double)A.attrs[(size_t)T.id[0] * A.C + c], a1 = (double)A.attrs[(size_t)T.id[1] * A.C + c];
                    const double a2 = (double)A.attrs[(size_t)T.id[2] * A.C + c];
                    a = (float)((a0 * beta[0] + a1 * beta[1]) + a2 * beta[2]);
                }
                attrs_out[((size_t)view * A.C + c) * hw + pix] = a;
            }
        }
    }
    const u64 m = __ballot(hit);
    if ((threadIdx.x & 63u) == 0u && m) atomicAdd(&hdr->covered, (u32)__popcll(m));
}

} // namespace

extern "C" size_t f3dg_mesh_raster_workspace_bytes(long long V, long long F, long long H, long long W)
{
    if (raster_check_sizes(V, F, H, W) != F3DG_OK) return 0;
    return raster_layout(V, F, H, W).total;
}

extern "C" int f3dg_mesh_raster(void* stream, void* workspace, size_t workspace_bytes, long long N, long long F, const float* vertices,
                                const void* faces, int faces_int32, int V, const float* world_views, double fx, double fy, int H, int W,
                                double z_near, int cull, int C, const float* attrs, int* face_id, float* depth, float* bary,
                                float* attrs_out, long long* h_counts)
{
    if (!workspace || !vertices || !world_views || !face_id || !depth || !bary || !h_counts || (!faces && F > 0)) return F3DG_ERR_BAD_ARG;
    if ((attrs != nullptr) != (attrs_out != nullptr) || C < 0 || C > RAST_MAX_C || (C == 0) != (attrs == nullptr)) return F3DG_ERR_BAD_ARG;
    if (N <= 0 || cull < 0 || cull > 2 || ((uintptr_t)workspace & 15u)) return F3DG_ERR_BAD_ARG;
    const double dmax = 1.7976931348623157e308;
    if (!(fx > 0.0 && fx <= dmax) || !(fy > 0.0 && fy <= dmax) || !(z_near > 0.0 && z_near <= dmax)) return F3DG_ERR_BAD_ARG;     // (a NaN fails)
    const int rc = raster_check_sizes(V, F, H, W);
    if (rc != F3DG_OK) return rc;
    if (N >= (1ll << 31)) return F3DG_ERR_UNSUPPORTED;
    const RasterLayout L = raster_layout(V, F, H, W);
    if (workspace_bytes < L.total) return F3DG_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    char* ws = (char*)workspace;
    RasterHeader* hdr = reinterpret_cast<RasterHeader*>(ws + L.header);
    u64* keys = reinterpret_cast<u64*>(ws + L.keys);
    u32* queue = reinterpret_cast<u32*>(ws + L.queue);
    RasterArgs A;
    A.vertices = vertices; A.faces = faces; A.world_views = world_views; A.attrs = attrs;
    A.fx = fx; A.fy = fy; A.z_near = z_near; A.half_w = (double)W / 2.0; A.half_h = (double)H / 2.0;
    A.N = (u32)N; A.F = (u32)F; A.V = (u32)V; A.H = (u32)H; A.W = (u32)W;
    A.cull = cull; A.C = C; A.faces_int32 = faces_int32;
    const u32 n_pix = (u32)((i64)V * H * W), n_pair = (u32)((i64)V * F);
    const u32 nb_pix = (n_pix + F3DG_BLOCK - 1) / F3DG_BLOCK, nb_pair = (n_pair + F3DG_BLOCK - 1) / F3DG_BLOCK;
    F3DG_KLAUNCH(raster_fill_kernel, dim3(nb_pix), dim3(F3DG_BLOCK), 0, s, keys, n_pix, hdr);
    if (n_pair) {
        F3DG_KLAUNCH(raster_small_kernel, dim3(nb_pair), dim3(F3DG_BLOCK), 0, s, A, keys, queue, hdr);
        F3DG_KLAUNCH(raster_large_kernel, dim3(RAST_LARGE_GRID), dim3(F3DG_BLOCK), 0, s, A, keys, (const u32*)queue, (const RasterHeader*)hdr);
    }
    F3DG_KLAUNCH(raster_resolve_kernel, dim3(nb_pix), dim3(F3DG_BLOCK), 0, s, A, (const u64*)keys, hdr, face_id, depth, bary,
                 attrs_out);
    F3DG_HIP_CHECK(hipGetLastError());
    // the one host read: the counts and whether an id was out of range
    RasterHeader h;
    F3DG_HIP_CHECK(hipMemcpyAsync(&h, hdr, sizeof(RasterHeader), hipMemcpyDeviceToHost, s));
    F3DG_HIP_CHECK(hipStreamSynchronize(s));
    if (h.bad) return F3DG_ERR_BAD_ARG;                     // nothing but the workspace was written
    for (int c = 0; c < 5; c++) h_counts[c] = (long long)h.cls[c];
    h_counts[5] = (long long)h.n_large;
    h_counts[6] = (long long)h.covered;
    return F3DG_OK;
}
