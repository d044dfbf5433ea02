// f3dg_mesh_bake.hip -- the views' colour put back on a mesh: every vertex projected into every view, tested against the z-buffer
// f3dg_mesh_raster wrote for this mesh and these cameras, sampled bilinearly and blended over the views in ascending order. The
// semantics are this project's, stated in include/f3dg.h and DESIGN.md section 3g-sexies; tests/mesh_bake_truth.py restates them in
// float64 numpy. The projection is f3dg_mesh_project.h's, the rasteriser's own. Integer atomics only (the class counts), no float
// atomics: every output is a function of the input alone.
//   bake_kernel   a wave takes BAKE_VB vertices x a slice of BAKE_VS consecutive views, one (vertex, view) pair per lane
//                 (lane = slice_view * BAKE_VB + vertex). Every lane classifies its pair and leaves (w, s_0 .. s_{C-1}) in the wave's
//                 own LDS rows; the lane of slice view 0 folds its vertex's BAKE_VS samples in ascending view order into registers it
//                 keeps across the slices, which the same wave walks in ascending order: no partial sum is ever re-associated. The
//                 camera matrices are widened to double once per workgroup, BAKE_TABLE views at a time, into an LDS table the
//                 workgroup refills between two barriers; no index into it reaches BAKE_TABLE. The class counts stay in wave-uniform
//                 registers (ballots) until the wave ends: one integer atomicAdd per wave and class. No thread waits on another
//                 wave, and every loop is bounded by V.
#include "f3dg_common.h"
#include "f3dg_mesh_project.h"

namespace {

typedef unsigned int u32;
typedef unsigned long long u64;
typedef long long i64;

#ifndef BAKE_VS
#define BAKE_VS 4                   // views of a slice (a power of two, at most 64); 1 is the plain loop of one lane per vertex, which
                                    // profiles/mesh_color.md measures against 4, 8 and 16
#endif
#define BAKE_VB (64 / BAKE_VS)      // vertices of a wave
#define BAKE_WAVES (F3DG_BLOCK / 64)
#define BAKE_TABLE 128              // views whose matrices the LDS table holds at a time
#define BAKE_MAX_C 8
static_assert(BAKE_VS >= 1 && BAKE_VS <= 64 && (BAKE_VS & (BAKE_VS - 1)) == 0 && BAKE_TABLE % BAKE_VS == 0, "a slice divides the wave and the table");

enum { BAKE_NEAR = 0, BAKE_OUTSIDE = 1, BAKE_UNCOVERED = 2, BAKE_OCCLUDED = 3, BAKE_GRAZING = 4, BAKE_MASKED = 5, BAKE_USED = 6 };

struct BakeHeader {                 // the workspace: 256 bytes
    u32 cls[7];                     // pairs per class
    u32 seen;                       // vertices with a used sample
    u32 reserved[56];
};
static_assert(sizeof(BakeHeader) == 256, "the header is the workspace");

// F3DG_OK, or why the sizes are refused
int bake_check_sizes(i64 V, i64 N, i64 H, i64 W)
{
    if (V <= 0 || N <= 0 || H <= 0 || W <= 0) return F3DG_ERR_BAD_ARG;
    if (H > 16384 || W > 16384 || N >= (1ll << 31) || V >= (1ll << 31)) return F3DG_ERR_UNSUPPORTED;
    if (V * N >= (1ll << 31) || V * H * W >= (1ll << 31)) return F3DG_ERR_UNSUPPORTED;       // (each product is below 2^62)
    return F3DG_OK;
}

struct BakeArgs {                   // by value to the kernel
    const float* vertices;
    const float* normals;           // or null
    const float* world_views;
    const float* images;
    const int* face_id;
    const float* depth;
    const float* alpha;             // or null
    double fx, fy, z_near, half_w, half_h, w_max, h_max;        // half_w = (double)W / 2, w_max = (double)(W - 1)
    double alpha_min, depth_tol, cm2;                           // cm2 = cos_min * cos_min
    u32 N, V, H, W;
    int C, mode;
    float* colors;
    float* weight;
    int* n_used;
    int* best_view;
};

// The class of the pair (vertex at (X, Y, Z) with normal n, view) and, for BAKE_USED, its weight w and sample s[0 .. C). m: the view's
// widened matrix. Every index is inside its array: 0 <= u <= W - 1 and 0 <= v <= H - 1 hold before any pixel is read.
__device__ __forceinline__ int bake_eval(const BakeArgs& A, u32 view, double X, double Y, double Z, double nx, double ny, double nz,
                                         const double* m, double& w, double s[BAKE_MAX_C])
{
    double x, y, z, u, v;
    if (f3dg_mesh_project(X, Y, Z, m, A.fx, A.fy, A.half_w, A.half_h, A.z_near, x, y, z, u, v)) return BAKE_NEAR;
    if (!(0.0 <= u && u <= A.w_max && 0.0 <= v && v <= A.h_max)) return BAKE_OUTSIDE;
    const size_t hw = (size_t)A.H * A.W;
    const size_t plane = (size_t)view * hw;                             // below V H W < 2^31
    const size_t near_pix = plane + (size_t)(int)rint(v) * A.W + (size_t)(int)rint(u);
    if (A.face_id[near_pix] < 0) return BAKE_UNCOVERED;
    if (!(z - (double)A.depth[near_pix] <= A.depth_tol)) return BAKE_OCCLUDED;
    w = 1.0;
    if (A.normals) {
        const double n0 = (nx * m[0] + ny * m[4]) + nz * m[8];
        const double n1 = (nx * m[1] + ny * m[5]) + nz * m[9];
        const double n2 = (nx * m[2] + ny * m[6]) + nz * m[10];
        const double g = -((n0 * x + n1 * y) + n2 * z);
        const double nn = (n0 * n0 + n1 * n1) + n2 * n2;
        const double pp = (x * x + y * y) + z * z;
        if (!f3dg_mesh_finite(nn) || !(nn > 0.0) || !(g > 0.0) || !(g * g >= A.cm2 * (nn * pp))) return BAKE_GRAZING;
        w = (g * g) / (nn * pp);
    }
    const int i0 = (int)floor(u), j0 = (int)floor(v);
    const int i1 = min(i0 + 1, (int)A.W - 1), j1 = min(j0 + 1, (int)A.H - 1);
    const size_t t00 = (size_t)j0 * A.W + i0, t10 = (size_t)j0 * A.W + i1, t01 = (size_t)j1 * A.W + i0, t11 = (size_t)j1 * A.W + i1;
    bool ok = true;
    if (A.alpha) {
        const float* al = A.alpha + plane;
        const double a00 = (double)al[t00], a10 = (double)al[t10], a01 = (double)al[t01], a11 = (double)al[t11];
        ok = (a00 >= A.alpha_min) && (a10 >= A.alpha_min) && (a01 >= A.alpha_min) && (a11 >= A.alpha_min);
    }
    const double a = u - (double)i0, b = v - (double)j0;
    const float* img = A.images + (size_t)view * A.C * hw;              // V C H W floats: size_t throughout
#pragma unroll
    for (int c = 0; c < BAKE_MAX_C; c++) {
        if (c < A.C) {
            const float* p = img + (size_t)c * hw;
            const double c00 = (double)p[t00], c10 = (double)p[t10], c01 = (double)p[t01], c11 = (double)p[t11];
            ok = ok && f3dg_mesh_finite(c00) && f3dg_mesh_finite(c10) && f3dg_mesh_finite(c01) && f3dg_mesh_finite(c11);
            const double top = c00 + a * (c10 - c00);
            const double bot = c01 + a * (c11 - c01);
            s[c] = top + b * (bot - top);
        }
    }
    return ok ? BAKE_USED : BAKE_MASKED;
}

__global__ void __launch_bounds__(F3DG_BLOCK)
bake_kernel(BakeArgs A, BakeHeader* __restrict__ hdr)
{
    __shared__ double tab[BAKE_TABLE * 16];                             // the widened matrices of views [base, base + BAKE_TABLE)
    __shared__ double samp[BAKE_WAVES][BAKE_MAX_C + 1][64];            // per wave: row 0 the weights, row 1 + c channel c, one column per lane
    const u32 lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const u32 sv = lane / BAKE_VB, vl = lane % BAKE_VB;                 // the lane's view of the slice and vertex of the wave
    const u32 vertex = (blockIdx.x * BAKE_WAVES + wave) * BAKE_VB + vl; // below N + 256 <= 2^31 + 255
    const bool live = vertex < A.N;
    const bool folder = live && sv == 0u;
    double X = 0.0, Y = 0.0, Z = 0.0, nx = 0.0, ny = 0.0, nz = 0.0;
    if (live) {
        const float* p = A.vertices + 3 * (size_t)vertex;
        X = (double)p[0]; Y = (double)p[1]; Z = (double)p[2];
        if (A.normals) {
            const float* n = A.normals + 3 * (size_t)vertex;
            nx = (double)n[0]; ny = (double)n[1]; nz = (double)n[2];
        }
    }
    // the folder's state: BLEND keeps the sums in acc, BEST the best sample
    double Sw = 0.0, bw = 0.0, acc[BAKE_MAX_C];
#pragma unroll
    for (int c = 0; c < BAKE_MAX_C; c++) acc[c] = 0.0;
    int used_n = 0, bview = -1;
    u32 cnt[7] = { 0u, 0u, 0u, 0u, 0u, 0u, 0u };                        // wave-uniform
    double (*mine)[64] = samp[wave];

    for (u32 base = 0; base < A.V; base += BAKE_TABLE) {
        const u32 held = min((u32)BAKE_TABLE, A.V - base);
        __syncthreads();                                               // (the table's readers of the last round are done)
        for (u32 t = threadIdx.x; t < held * 16u; t += F3DG_BLOCK) tab[t] = (double)A.world_views[(size_t)base * 16 + t];
        __syncthreads();
        for (u32 s0 = 0; s0 < held; s0 += BAKE_VS) {
            const u32 slot = s0 + sv;                                  // below BAKE_TABLE: s0 <= BAKE_TABLE - BAKE_VS
            int cls = -1;
            double w = 0.0, s[BAKE_MAX_C];
#pragma unroll
            for (int c = 0; c < BAKE_MAX_C; c++) s[c] = 0.0;
            if (live && slot < held) cls = bake_eval(A, base + slot, X, Y, Z, nx, ny, nz, tab + 16 * slot, w, s);
#pragma unroll
            for (int c = 0; c < 7; c++) cnt[c] += (u32)__popcll(__ballot(cls == c));
            const u64 used = __ballot(cls == BAKE_USED);
            if (used == 0ull) continue;                                // (wave-uniform)
            if (BAKE_VS > 1) {
                mine[0][lane] = w;
#pragma unroll
                for (int c = 0; c < BAKE_MAX_C; c++)
                    if (c < A.C) mine[1 + c][lane] = s[c];
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            }
            if (folder) {
                for (u32 k = 0; k < BAKE_VS; k++) {                    // ascending views
                    const u32 src = k * BAKE_VB + vl;
                    if (!((used >> src) & 1ull)) continue;
                    const double wk = BAKE_VS > 1 ? mine[0][src] : w;
                    const bool better = used_n == 0 || wk > bw;
                    used_n++;
                    if (better) { bw = wk; bview = (int)(base + s0 + k); }
                    if (A.mode == F3DG_BAKE_BLEND) Sw = Sw + wk;
#pragma unroll
                    for (int c = 0; c < BAKE_MAX_C; c++) {
                        if (c < A.C) {
                            const double sk = BAKE_VS > 1 ? mine[1 + c][src] : s[c];
                            if (A.mode == F3DG_BAKE_BLEND) acc[c] = acc[c] + wk * sk;
                            else if (better) acc[c] = sk;
                        }
                    }
                }
            }
            if (BAKE_VS > 1) {                                         // the rows are read before the next slice overwrites them
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            }
        }
    }

    if (folder) {
        const bool blend = A.mode == F3DG_BAKE_BLEND;
#pragma unroll
        for (int c = 0; c < BAKE_MAX_C; c++)
            if (c < A.C) A.colors[(size_t)vertex * A.C + c] = used_n == 0 ? 0.0f : (float)(blend ? acc[c] / Sw : acc[c]);
        A.weight[vertex] = used_n == 0 ? 0.0f : (float)(blend ? Sw : bw);
        A.n_used[vertex] = used_n;
        A.best_view[vertex] = bview;
    }
    const u32 seen = (u32)__popcll(__ballot(folder && used_n > 0));
    if (lane == 0u) {
#pragma unroll
        for (int c = 0; c < 7; c++)
            if (cnt[c]) atomicAdd(&hdr->cls[c], cnt[c]);
        if (seen) atomicAdd(&hdr->seen, seen);
    }
}

} // namespace

extern "C" size_t f3dg_mesh_bake_workspace_bytes(long long V, long long N, long long H, long long W)
{
    if (bake_check_sizes(V, N, H, W) != F3DG_OK) return 0;
    return sizeof(BakeHeader);
}

extern "C" int f3dg_mesh_bake_colors(void* stream, void* workspace, size_t workspace_bytes, long long N, const float* vertices,
                                     const float* normals, long long V, const float* world_views, double fx, double fy, long long H,
                                     long long W, double z_near, int C, const float* images, const int* face_id, const float* depth,
                                     const float* alpha, double alpha_min, double depth_tol, double cos_min, int mode, float* colors,
                                     float* weight, int* n_used, int* best_view, long long* h_counts)
{
    if (!workspace || !vertices || !world_views || !images || !face_id || !depth || !colors || !weight || !n_used || !best_view || !h_counts)
        return F3DG_ERR_BAD_ARG;
    if (N <= 0 || V <= 0 || H <= 0 || W <= 0 || C < 1 || C > BAKE_MAX_C || ((uintptr_t)workspace & 15u)) return F3DG_ERR_BAD_ARG;
    if (mode != F3DG_BAKE_BLEND && mode != F3DG_BAKE_BEST) return F3DG_ERR_BAD_ARG;
    const double dmax = 1.7976931348623157e308;
    if (!(fx > 0.0 && fx <= dmax) || !(fy > 0.0 && fy <= dmax) || !(z_near > 0.0 && z_near <= dmax)) return F3DG_ERR_BAD_ARG;     // (a NaN fails)
    if (!(depth_tol >= 0.0 && depth_tol <= dmax) || !(cos_min >= 0.0 && cos_min <= 1.0)) return F3DG_ERR_BAD_ARG;
    if (alpha && alpha_min != alpha_min) return F3DG_ERR_BAD_ARG;
    const int rc = bake_check_sizes(V, N, H, W);
    if (rc != F3DG_OK) return rc;
    if (workspace_bytes < sizeof(BakeHeader)) return F3DG_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    BakeHeader* hdr = reinterpret_cast<BakeHeader*>(workspace);
    BakeArgs A;
    A.vertices = vertices; A.normals = normals; A.world_views = world_views; A.images = images; A.face_id = face_id; A.depth = depth;
    A.alpha = alpha;
    A.fx = fx; A.fy = fy; A.z_near = z_near; A.half_w = (double)W / 2.0; A.half_h = (double)H / 2.0;
    A.w_max = (double)(W - 1); A.h_max = (double)(H - 1);
    A.alpha_min = alpha_min; A.depth_tol = depth_tol; A.cm2 = cos_min * cos_min;
    A.N = (u32)N; A.V = (u32)V; A.H = (u32)H; A.W = (u32)W;
    A.C = C; A.mode = mode;
    A.colors = colors; A.weight = weight; A.n_used = n_used; A.best_view = best_view;
    F3DG_HIP_CHECK(hipMemsetAsync(hdr, 0, sizeof(BakeHeader), s));
    const u32 per_group = BAKE_WAVES * BAKE_VB;
    const u32 groups = (u32)((N + per_group - 1) / per_group);         // at most 2^31 / 4: inside a grid's first dimension
    F3DG_KLAUNCH(bake_kernel, dim3(groups), dim3(F3DG_BLOCK), 0, s, A, hdr);
    F3DG_HIP_CHECK(hipGetLastError());
    // the one host read: the counts
    BakeHeader h;
    F3DG_HIP_CHECK(hipMemcpyAsync(&h, hdr, sizeof(BakeHeader), hipMemcpyDeviceToHost, s));
    F3DG_HIP_CHECK(hipStreamSynchronize(s));
    for (int c = 0; c < 7; c++) h_counts[c] = (long long)h.cls[c];
    h_counts[7] = (long long)h.seen;
    return F3DG_OK;
}
