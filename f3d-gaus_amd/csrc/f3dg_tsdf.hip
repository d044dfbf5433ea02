// f3dg_tsdf.hip -- the TSDF mesh route: rendered depth maps fused into a truncated signed distance volume, the volume's surface cells
// turned into tetrahedra for f3dg_marching_tets_count / _emit (f3dg_mesh.hip), and the crossing edges interpolated into vertices and
// vertex colours. The reference's release holds no TSDF code: the semantics are this project's, stated in include/f3dg.h and DESIGN.md
// section 3g-bis; tests/tsdf_truth.py restates them in float64.
//
//   tsdf_integrate_kernel   one thread per voxel, x fastest across the lanes of a wave64 (the four state arrays stream), a loop over
//                           the views of the launch in ascending order. The camera table (twelve numbers per view, widened to
//                           float64 once) sits in LDS and every lane of a wave reads the same entry (a broadcast); neighbouring
//                           voxels project to neighbouring pixels, so a wave's depth / alpha / colour gathers fall on a few lines.
//                           The projection, the band tests and the running sums are float64 on the float32 inputs, as the forward
//                           warp's (f3dg_warp.hip): the kernel waits on its gathers, and float64 keeps it on the definition's side of
//                           the floor, of Z > z_near and of the two band tests wherever float32 rounding could flip them. One writer
//                           per voxel, a fixed view order, no atomics: bit-reproducible. A voxel no view of the call sees is not
//                           written at all.
// The surface cells are compacted as f3dg_compact.h describes:
//   tsdf_classify_kernel    one thread per cell: eight corners, then the cell's flag and the workgroup's count (block_flag_and_count)
//   tsdf_scan_kernel        one workgroup: compact_scan_counts, total and `ready` into the header
//   tsdf_emit_kernel        one thread per active cell at its compact_rank: six int4
//   tsdf_vertices_kernel    one thread per crossing edge, float32, the operation order of the header
#include "f3dg_common.h"
#include "f3dg_compact.h"

namespace {

struct TsdfArgs {
    int nx, ny, nz, n_views, H, W;
    double ox, oy, oz, voxel, trunc, z_near, fx, fy;
    float alpha_min;
    const float* depth;         // [n_views,H,W]
    const float* color;         // [n_views,3,H,W] or null
    const float* alpha;         // [n_views,H,W] or null
    const float* world_view;    // [n_views,16]
    float* tsdf;
    float* weight;
    float* color_out;
    float* color_weight;
};

__global__ void __launch_bounds__(F3DG_BLOCK)
tsdf_integrate_kernel(TsdfArgs A)
{
    __shared__ double cam[F3DG_TSDF_MAX_VIEWS][12];         // [view][3 r + c] = world_view[r][c], r < 4, c < 3
    for (int i = threadIdx.x; i < A.n_views * 12; i += F3DG_BLOCK) {
        const int v = i / 12, k = i - 12 * v;
        cam[v][k] = (double)A.world_view[16 * (size_t)v + 4 * (k / 3) + (k % 3)];
    }
    __syncthreads();
    const u32 N = (u32)A.nx * (u32)A.ny * (u32)A.nz;        // < 2^31: the entry
    const u32 id = blockIdx.x * F3DG_BLOCK + threadIdx.x;
    if (id >= N) return;
    const u32 x = id % (u32)A.nx, yz = id / (u32)A.nx;
    const u32 y = yz % (u32)A.ny, z = yz / (u32)A.ny;
    const double px = A.ox + A.voxel * (double)x, py = A.oy + A.voxel * (double)y, pz = A.oz + A.voxel * (double)z;
    const int HW = A.H * A.W;
    const double half_w = A.W / 2.0, half_h = A.H / 2.0;
    double S = 0.0, C0 = 0.0, C1 = 0.0, C2 = 0.0;
    u32 n = 0, nc = 0;
    for (int v = 0; v < A.n_views; v++) {
        const double* M = cam[v];
        const double Z = px * M[2] + py * M[5] + pz * M[8] + M[11];
        if (!(Z > A.z_near)) continue;
        const double X = px * M[0] + py * M[3] + pz * M[6] + M[9];
        const double Y = px * M[1] + py * M[4] + pz * M[7] + M[10];
        const double u = A.fx * X / Z + half_w;
        const double w = A.fy * Y / Z + half_h;
        if (!(u >= 0.0 && u < (double)A.W && w >= 0.0 && w < (double)A.H)) continue;        // (NaN fails every comparison)
        const int i = (int)floor(u), j = (int)floor(w);                                     // in [0, W) x [0, H)
        const size_t pix = (size_t)v * HW + (size_t)(j * A.W + i);
        const float df = A.depth[pix];
        if (!(df > 0.0f && df <= 3.402823466e+38f)) continue;                               // NaN, +Inf, zero and negative depths
        if (A.alpha && !(A.alpha[pix] >= A.alpha_min)) continue;
        const double sdf = (double)df - Z;
        if (sdf < -A.trunc) continue;
        S += fmin(1.0, sdf / A.trunc);
        n++;
        if (A.color && fabs(sdf) <= A.trunc) {
            const float* c = A.color + (size_t)v * 3 * HW + (size_t)(j * A.W + i);
            C0 += (double)c[0];
            C1 += (double)c[HW];
            C2 += (double)c[2 * (size_t)HW];
            nc++;
        }
    }
    if (n) {
        const double w0 = (double)A.weight[id], wn = w0 + (double)n;
        if (wn > 0.0) {
            A.tsdf[id] = (float)(((double)A.tsdf[id] * w0 + S) / wn);
            A.weight[id] = (float)wn;
        }
    }
    if (nc) {
        const double w0 = (double)A.color_weight[id], wn = w0 + (double)nc;
        if (wn > 0.0) {
            const size_t Ns = (size_t)N;
            A.color_out[id] = (float)(((double)A.color_out[id] * w0 + C0) / wn);
            A.color_out[Ns + id] = (float)(((double)A.color_out[Ns + id] * w0 + C1) / wn);
            A.color_out[2 * Ns + id] = (float)(((double)A.color_out[2 * Ns + id] * w0 + C2) / wn);
            A.color_weight[id] = (float)wn;
        }
    }
}

// ------------------------------------------------------------------------------------------------ surface cells
struct TsdfCellsHeader {            // first 256 bytes of the workspace
    u64 n_active;
    u32 ready;                      // non-zero once the counts are scanned: f3dg_tsdf_cells_emit may read them
    u32 nx, ny, nz;                 // the volume they were counted on
    u32 reserved[58];
};

struct TsdfCellsLayout {
    size_t header, flags, blk, total;
    u32 n_cells;
    CompactPlan cells;
};

// F3DG_OK, or why the volume is refused (`cells`: the cell entries need two voxels along every axis)
int tsdf_check_dims(int nx, int ny, int nz, bool cells)
{
    const int least = cells ? 2 : 1;
    if (nx < least || ny < least || nz < least) return F3DG_ERR_BAD_ARG;
    if ((long long)nx * ny >= (1ll << 31) || (long long)nx * ny * nz >= (1ll << 31)) return F3DG_ERR_UNSUPPORTED;
    return F3DG_OK;
}

TsdfCellsLayout tsdf_cells_layout(int nx, int ny, int nz)
{
    TsdfCellsLayout L;
    L.n_cells = (u32)(nx - 1) * (u32)(ny - 1) * (u32)(nz - 1);
    L.cells = compact_plan(L.n_cells);
    L.header = 0;
    L.flags = f3dg_align256(sizeof(TsdfCellsHeader));
    L.blk = L.flags + L.cells.flag_bytes;
    L.total = L.blk + L.cells.count_bytes;
    return L;
}

// cell c -> the voxel id of its (0,0,0) corner
__device__ __forceinline__ u32 tsdf_cell_base(u32 c, u32 nx, u32 ny)
{
    const u32 cx = c % (nx - 1u), r = c / (nx - 1u);
    const u32 cy = r % (ny - 1u), cz = r / (ny - 1u);
    return (cz * ny + cy) * nx + cx;
}

__global__ void __launch_bounds__(F3DG_BLOCK)
tsdf_classify_kernel(u32 nx, u32 ny, u32 n_cells, float min_weight, const float* __restrict__ tsdf, const float* __restrict__ weight,
                     u64* __restrict__ flags, u32* __restrict__ blk)
{
    __shared__ u32 w_cnt[F3DG_BLOCK / 64];
    const u32 c = blockIdx.x * F3DG_BLOCK + threadIdx.x;
    bool active = false;
    if (c < n_cells) {
        const u32 base = tsdf_cell_base(c, nx, ny);         // the far corner is base + nx ny + nx + 1 <= nx ny nz - 1
        bool ok = true;
        u32 neg = 0;
#pragma unroll
        for (u32 k = 0; k < 8u; k++) {
            const u32 id = base + (k & 1u) + ((k >> 1) & 1u) * nx + (k >> 2) * nx * ny;
            const float t = tsdf[id];
            ok = ok && weight[id] >= min_weight && fabsf(t) <= 3.402823466e+38f;         // (a NaN weight or tsdf fails)
            neg += t < 0.0f ? 1u : 0u;
        }
        active = ok && neg != 0u && neg != 8u;
    }
    block_flag_and_count(active, c, n_cells, flags, blk, w_cnt);
}

__global__ void __launch_bounds__(F3DG_BLOCK)
tsdf_scan_kernel(u32* __restrict__ blk, u32 n_scan, u32 nx, u32 ny, u32 nz, TsdfCellsHeader* __restrict__ hdr)
{
    __shared__ u64 wtot[F3DG_BLOCK / 64];
    const u64 total = compact_scan_counts(blk, n_scan, wtot);
    if (threadIdx.x == 0) {
        hdr->n_active = total;
        hdr->nx = nx; hdr->ny = ny; hdr->nz = nz;
        hdr->ready = 1u;
    }
}

__global__ void __launch_bounds__(F3DG_BLOCK)
tsdf_emit_kernel(u32 nx, u32 ny, u32 nz, u32 n_cells, u64 n_rows, const u64* __restrict__ flags, const u32* __restrict__ blk,
                 const TsdfCellsHeader* __restrict__ hdr, int4* __restrict__ tets)
{
    if (!hdr->ready || hdr->nx != nx || hdr->ny != ny || hdr->nz != nz) return;      // no completed count of this volume on the workspace
    const u32 c = blockIdx.x * F3DG_BLOCK + threadIdx.x;
    if (c >= n_cells || !compact_kept(flags, c)) return;
    const u64 row = compact_rank(flags, blk, c);
    if (row >= n_rows) return;                                                       // the caller's array ends here
    const int b = (int)tsdf_cell_base(c, nx, ny);
    const int X = 1, Y = (int)nx, Z = (int)(nx * ny), D = X + Y + Z;
    int4* out = tets + 6 * row;
    // axis orders xyz, xzy, yxz, yzx, zxy, zyx; the two middle vertices of the even ones swapped (include/f3dg.h)
    out[0] = make_int4(b, b + X + Y, b + X, b + D);
    out[1] = make_int4(b, b + X, b + X + Z, b + D);
    out[2] = make_int4(b, b + Y, b + X + Y, b + D);
    out[3] = make_int4(b, b + Y + Z, b + Y, b + D);
    out[4] = make_int4(b, b + X + Z, b + Z, b + D);
    out[5] = make_int4(b, b + Z, b + Y + Z, b + D);
}

// ------------------------------------------------------------------------------------------------ vertices
__global__ void __launch_bounds__(F3DG_BLOCK)
tsdf_vertices_kernel(u32 nx, u32 ny, u32 N, float ox, float oy, float oz, float voxel, u64 E, const long long* __restrict__ interp_v,
                     const float* __restrict__ tsdf, const float* __restrict__ color, const float* __restrict__ color_weight,
                     float* __restrict__ vertices, float* __restrict__ vertex_colors)
{
    const u64 e = (u64)blockIdx.x * F3DG_BLOCK + threadIdx.x;
    if (e >= E) return;
    const long long lo = interp_v[2 * e], hi = interp_v[2 * e + 1];
    float vx = 0.0f, vy = 0.0f, vz = 0.0f, c0 = 0.0f, c1 = 0.0f, c2 = 0.0f;
    if (lo >= 0 && lo < (long long)N && hi >= 0 && hi < (long long)N) {              // ids outside the volume index nothing: zeros
        const bool lo_occ = tsdf[lo] < 0.0f;
        const u32 f = (u32)(lo_occ ? hi : lo), o = (u32)(lo_occ ? lo : hi);          // free end, occupied end
        const float tf = tsdf[f], den = tf - tsdf[o];
        const float w = den > 0.0f ? tf / den : 0.0f;                                 // (an edge that does not cross: the free end)
        const u32 fx = f % nx, fr = f / nx, gx = o % nx, gr = o / nx;
        const float pfx = ox + voxel * (float)fx, pfy = oy + voxel * (float)(fr % ny), pfz = oz + voxel * (float)(fr / ny);
        const float pox = ox + voxel * (float)gx, poy = oy + voxel * (float)(gr % ny), poz = oz + voxel * (float)(gr / ny);
        vx = pfx + (pox - pfx) * w;
        vy = pfy + (poy - pfy) * w;
        vz = pfz + (poz - pfz) * w;
        if (vertex_colors) {
            const bool hf = color_weight[f] > 0.0f, ho = color_weight[o] > 0.0f;
            const size_t Ns = (size_t)N;
            if (hf && ho) {
                const float a0 = color[f], a1 = color[Ns + f], a2 = color[2 * Ns + f];
                c0 = a0 + (color[o] - a0) * w;
                c1 = a1 + (color[Ns + o] - a1) * w;
                c2 = a2 + (color[2 * Ns + o] - a2) * w;
            } else if (hf || ho) {
                const u32 k = hf ? f : o;
                c0 = color[k]; c1 = color[Ns + k]; c2 = color[2 * Ns + k];
            }
        }
    }
    vertices[3 * e] = vx; vertices[3 * e + 1] = vy; vertices[3 * e + 2] = vz;
    if (vertex_colors) { vertex_colors[3 * e] = c0; vertex_colors[3 * e + 1] = c1; vertex_colors[3 * e + 2] = c2; }
}

bool tsdf_finite_pos(float v) { return v > 0.0f && v <= 3.402823466e+38f; }

} // namespace

extern "C" int f3dg_tsdf_integrate(void* stream, int nx, int ny, int nz, const float* origin, float voxel, float trunc, float z_near,
                                   int n_views, int H, int W, const float* depth, const float* color, const float* alpha, float alpha_min,
                                   const float* world_view, float fx, float fy, float* tsdf, float* weight, float* color_out,
                                   float* color_weight)
{
    if (!origin || !depth || !world_view || !tsdf || !weight || (color && (!color_out || !color_weight))) return F3DG_ERR_BAD_ARG;
    if (n_views <= 0 || H <= 0 || W <= 0) return F3DG_ERR_BAD_ARG;
    if (!tsdf_finite_pos(voxel) || !tsdf_finite_pos(trunc) || !tsdf_finite_pos(fx) || !tsdf_finite_pos(fy)) return F3DG_ERR_BAD_ARG;
    if (!(z_near >= 0.0f && z_near <= 3.402823466e+38f) || !(alpha_min == alpha_min)) return F3DG_ERR_BAD_ARG;
    for (int k = 0; k < 3; k++)
        if (!(fabsf(origin[k]) <= 3.402823466e+38f)) return F3DG_ERR_BAD_ARG;
    const int rc = tsdf_check_dims(nx, ny, nz, false);
    if (rc != F3DG_OK) return rc;
    if ((long long)H * W >= (1ll << 31)) return F3DG_ERR_UNSUPPORTED;
    const u32 N = (u32)nx * (u32)ny * (u32)nz;
    const size_t HW = (size_t)H * W;
    TsdfArgs A = { nx, ny, nz, 0, H, W, (double)origin[0], (double)origin[1], (double)origin[2], (double)voxel, (double)trunc, (double)z_near,
                   (double)fx, (double)fy, alpha_min, depth, color, alpha, world_view, tsdf, weight, color ? color_out : nullptr,
                   color ? color_weight : nullptr };
    // more views than the camera table holds: consecutive launches over consecutive views, each on the state the one before left
    for (int v0 = 0; v0 < n_views; v0 += F3DG_TSDF_MAX_VIEWS) {
        A.n_views = n_views - v0 < F3DG_TSDF_MAX_VIEWS ? n_views - v0 : F3DG_TSDF_MAX_VIEWS;
        A.depth = depth + (size_t)v0 * HW;
        A.color = color ? color + (size_t)v0 * 3 * HW : nullptr;
        A.alpha = alpha ? alpha + (size_t)v0 * HW : nullptr;
        A.world_view = world_view + 16 * (size_t)v0;
        F3DG_KLAUNCH(tsdf_integrate_kernel, dim3((N + F3DG_BLOCK - 1) / F3DG_BLOCK), dim3(F3DG_BLOCK), 0, (hipStream_t)stream, A);
        F3DG_HIP_CHECK(hipGetLastError());
    }
    return F3DG_OK;
}

extern "C" size_t f3dg_tsdf_cells_workspace_bytes(int nx, int ny, int nz)
{
    if (tsdf_check_dims(nx, ny, nz, true) != F3DG_OK) return 0;
    return tsdf_cells_layout(nx, ny, nz).total;
}

extern "C" int f3dg_tsdf_cells_count(void* stream, int nx, int ny, int nz, float min_weight, const float* tsdf, const float* weight,
                                     void* workspace, size_t workspace_bytes, long long* h_n_active)
{
    if (!tsdf || !weight || !workspace || !h_n_active || ((uintptr_t)workspace & 15u) || !(min_weight == min_weight)) return F3DG_ERR_BAD_ARG;
    const int rc = tsdf_check_dims(nx, ny, nz, true);
    if (rc != F3DG_OK) return rc;
    const TsdfCellsLayout L = tsdf_cells_layout(nx, ny, nz);
    if (workspace_bytes < L.total) return F3DG_ERR_WORKSPACE;
    *h_n_active = 0;
    hipStream_t s = (hipStream_t)stream;
    char* ws = (char*)workspace;
    TsdfCellsHeader* hdr = (TsdfCellsHeader*)(ws + L.header);
    u32* blk = (u32*)(ws + L.blk);
    F3DG_HIP_CHECK(hipMemsetAsync(hdr, 0, sizeof(TsdfCellsHeader), s));
    F3DG_HIP_CHECK(compact_clear_padding(s, blk, L.cells));
    F3DG_KLAUNCH(tsdf_classify_kernel, dim3(L.cells.n_blocks), dim3(F3DG_BLOCK), 0, s, (u32)nx, (u32)ny, L.n_cells, min_weight, tsdf, weight,
                 (u64*)(ws + L.flags), blk);
    F3DG_KLAUNCH(tsdf_scan_kernel, dim3(1), dim3(F3DG_BLOCK), 0, s, blk, L.cells.n_scan, (u32)nx, (u32)ny, (u32)nz, hdr);
    F3DG_HIP_CHECK(hipGetLastError());
    // the one host read: the number of active cells
    u64 n_active = 0;
    F3DG_HIP_CHECK(hipMemcpyAsync(&n_active, &hdr->n_active, sizeof(u64), hipMemcpyDeviceToHost, s));
    F3DG_HIP_CHECK(hipStreamSynchronize(s));
    *h_n_active = (long long)n_active;
    return F3DG_OK;
}

extern "C" int f3dg_tsdf_cells_emit(void* stream, int nx, int ny, int nz, void* workspace, size_t workspace_bytes, long long n_active,
                                    int* tets)
{
    if (!workspace || !tets || ((uintptr_t)workspace & 15u) || ((uintptr_t)tets & 15u) || n_active <= 0) return F3DG_ERR_BAD_ARG;
    const int rc = tsdf_check_dims(nx, ny, nz, true);
    if (rc != F3DG_OK) return rc;
    const TsdfCellsLayout L = tsdf_cells_layout(nx, ny, nz);
    if (workspace_bytes < L.total) return F3DG_ERR_WORKSPACE;
    char* ws = (char*)workspace;
    F3DG_KLAUNCH(tsdf_emit_kernel, dim3(L.cells.n_blocks), dim3(F3DG_BLOCK), 0, (hipStream_t)stream, (u32)nx, (u32)ny, (u32)nz, L.n_cells, (u64)n_active,
                 (const u64*)(ws + L.flags), (const u32*)(ws + L.blk), (const TsdfCellsHeader*)(ws + L.header), (int4*)tets);
    F3DG_HIP_CHECK(hipGetLastError());
    return F3DG_OK;
}

extern "C" int f3dg_tsdf_vertices(void* stream, int nx, int ny, int nz, const float* origin, float voxel, long long E, const long long* interp_v,
                                  const float* tsdf, const float* color, const float* color_weight, float* vertices, float* vertex_colors)
{
    if (!origin || !interp_v || !tsdf || !vertices || (vertex_colors && (!color || !color_weight)) || E <= 0) return F3DG_ERR_BAD_ARG;
    if (!tsdf_finite_pos(voxel)) return F3DG_ERR_BAD_ARG;
    for (int k = 0; k < 3; k++)
        if (!(fabsf(origin[k]) <= 3.402823466e+38f)) return F3DG_ERR_BAD_ARG;
    const int rc = tsdf_check_dims(nx, ny, nz, false);
    if (rc != F3DG_OK) return rc;
    const u64 blocks = ((u64)E + F3DG_BLOCK - 1) / F3DG_BLOCK;
    if (blocks > 0x7FFFFFFFull) return F3DG_ERR_UNSUPPORTED;
    F3DG_KLAUNCH(tsdf_vertices_kernel, dim3((u32)blocks), dim3(F3DG_BLOCK), 0, (hipStream_t)stream, (u32)nx, (u32)ny, (u32)nx * (u32)ny * (u32)nz,
                 origin[0], origin[1], origin[2], voxel, (u64)E, interp_v, tsdf, color, color_weight, vertices, vertex_colors);
    F3DG_HIP_CHECK(hipGetLastError());
    return F3DG_OK;
}
