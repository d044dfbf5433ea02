// f3dg_mesh_smooth.hip -- what a mesh gets after extraction and clean-up: the vertex adjacency of a triangle mesh (a CSR of the distinct
// neighbours of every vertex, and which vertices lie on the boundary), Taubin lambda|mu smoothing over it, and area-weighted vertex
// normals. The semantics are this project's, stated in include/f3dg.h and DESIGN.md section 3g-quater; tests/mesh_smooth_truth.py restates
// them in float64 numpy. Integer atomics only, no float atomics: every output is a function of the input alone.
//
// Adjacency: every non-degenerate face gives each of its corners two 64-bit entries  nbr << 32 | face << 1 | succ ; a vertex's row is its
// entries sorted ascending. No thread waits for another thread's write, and every loop is bounded by a row length.
//   adj_count_kernel       one thread per face: the range check of its ids BEFORE anything is indexed with them, cnt[v] += 2 per corner
//   adj_scan_kernel        one 1024-thread workgroup: cnt -> start in place (scan_array_in_place, f3dg_scan.h); later the degrees
//   adj_scatter_kernel     one thread per face: two entries into the row of each corner (an integer atomicAdd on the row's fill counter
//                          hands out the slots; the sort below erases their arrival order)
//   adj_sort_small_kernel  rows of at most 32 entries: one thread each, insertion sort in place; longer rows are queued
//   adj_sort_big_kernel    one 1024-thread workgroup per queued row: bitonic network in LDS (up to 4,096 entries, 32 KB) or in place.
//                          (The shape of sort_small_kernel / sort_big_kernel / bitonic_any of f3dg_mesh.hip, on 64-bit keys.)
//   adj_degree_kernel      one thread per vertex: its distinct neighbours (runs of equal nbr in the sorted row) and whether a run has
//                          exactly one entry (a boundary edge); the counts of the call
//   adj_emit_kernel        one thread per vertex, after the scan of the degrees: nbr_start and its segment of nbr
// A face with an id out of range sets hdr->bad in the first kernel; every later kernel returns at once then, so a refused mesh writes no
// output. The sorted rows stay in the workspace, stamped with (N, F), for the normals.
//   mesh_smooth_kernel     one thread per vertex, one launch per step: d independent gathers, the sum and the step in float64
//   mesh_normals_kernel    one thread per vertex over its sorted row: the cross product of every face whose entry has succ == 1
#include "f3dg_common.h"
#include "f3dg_compact.h"
#include "f3dg_mesh_adjacency.h"    // the workspace header, its layout and stamp, load_face: f3dg_mesh_simplify.hip reads the rows too

namespace {

template <typename I>
__global__ void __launch_bounds__(F3DG_BLOCK)
adj_count_kernel(const I* __restrict__ faces, u32 F, u32 N, u32* __restrict__ cnt, AdjHeader* __restrict__ hdr)
{
    const u32 f = blockIdx.x * F3DG_BLOCK + threadIdx.x;
    bool dead = false;
    if (f < F) {
        u32 v[3];
        if (!load_face(faces, f, N, v)) {
            atomicOr(&hdr->bad, 1u);
        } else if (degenerate(v)) {
            dead = true;
        } else {
#pragma unroll
            for (int i = 0; i < 3; i++) atomicAdd(&cnt[v[i]], 2u);
        }
    }
    const u64 m = __ballot(dead);
    if ((threadIdx.x & 63u) == 0u && m) atomicAdd(&hdr->degenerate, (u32)__popcll(m));
}

// a[0, n_scan) -> its exclusive prefix sums, in place, by one workgroup. final == 0: the row lengths (a[N] = 0 comes out as the number of
// entries); final == 1: the degrees, and the stamp that lets the normals read the rows
__global__ void __launch_bounds__(ADJ_BIG_THREADS)
adj_scan_kernel(u32* __restrict__ a, u32 n_scan, u32 N, u32 F, int final, AdjHeader* __restrict__ hdr)
{
    __shared__ u64 wtot[ADJ_SCAN_WAVES];
    if (hdr->bad) return;                                   // (the whole workgroup: the flag was set by an earlier launch)
    const u64 total = scan_array_in_place<ADJ_SCAN_WAVES, ADJ_SCAN_ITEMS, u64>(a, n_scan, 0u, wtot);
    if (threadIdx.x == 0) {
        if (!final) {
            hdr->entries = total;
        } else {
            hdr->two_e = total;
            hdr->N = N; hdr->F = F;
            hdr->ready = ADJ_READY;
        }
    }
}

template <typename I>
__global__ void __launch_bounds__(F3DG_BLOCK)
adj_scatter_kernel(const I* __restrict__ faces, u32 F, u32 N, const u32* __restrict__ start, u32* __restrict__ fill, u64* __restrict__ rows,
                   const AdjHeader* __restrict__ hdr)
{
    if (hdr->bad) return;
    const u32 f = blockIdx.x * F3DG_BLOCK + threadIdx.x;
    if (f >= F) return;
    u32 v[3];
    if (!load_face(faces, f, N, v) || degenerate(v)) return;
#pragma unroll
    for (int i = 0; i < 3; i++) {
        const u32 a = v[i], b = v[(i + 1) % 3], c = v[(i + 2) % 3];
        const u32 slot = start[a] + atomicAdd(&fill[a], 2u);
        if (slot + 2u > start[a + 1u]) continue;            // (not the faces that were counted)
        rows[slot] = (u64)b << 32 | (u64)(2u * f + 1u);
        rows[slot + 1u] = (u64)c << 32 | (u64)(2u * f);
    }
}

__global__ void __launch_bounds__(F3DG_BLOCK)
adj_sort_small_kernel(u32 N, const u32* __restrict__ start, u64* rows, u32* __restrict__ big, u32 big_cap, AdjHeader* __restrict__ hdr)
{
    if (hdr->bad) return;
    const u32 v = blockIdx.x * F3DG_BLOCK + threadIdx.x;
    if (v >= N) return;
    const u32 s = start[v], n = start[v + 1] - s;
    if (n > ADJ_SMALL) {
        const u32 slot = atomicAdd(&hdr->n_big, 1u);
        if (slot < big_cap) big[slot] = v;          // (always: big_cap counts every row that can be this long)
        return;
    }
    u64* a = rows + s;
    for (u32 i = 1; i < n; i++) {
        const u64 x = a[i];
        u32 j = i;
        while (j > 0u && a[j - 1u] > x) { a[j] = a[j - 1u]; j--; }
        a[j] = x;
    }
}

// Bitonic network over a[0 .. n), any n: every compare-exchange puts the larger value at the HIGHER index, so the positions from n
// up to the next power of two behave as +infinity that never moves and are simply skipped.
__device__ void bitonic_any64(u64* a, u32 n)
{
    for (u64 k64 = 2; (k64 >> 1) < n; k64 <<= 1) {
        const u32 k = (u32)k64, half = (u32)(k64 >> 1);       // (k = 2^32 wraps to 0 only where blk is 0)
        for (u32 base = 0; base < n; base += ADJ_BIG_THREADS) {       // pair index i: block i / half, offset i % half
            const u32 i = base + threadIdx.x;
            const u32 blk = i / half, off = i % half;
            const u32 p = blk * k + off, q = blk * k + (k - 1u - off);
            if (q < n) { const u64 x = a[p], y = a[q]; if (x > y) { a[p] = y; a[q] = x; } }
        }
        __syncthreads();
        for (u32 j = half >> 1; j > 0u; j >>= 1) {
            for (u32 base = 0; base < n; base += ADJ_BIG_THREADS) {
                const u32 i = base + threadIdx.x;
                const u32 p = 2u * j * (i / j) + (i % j), q = p + j;
                if (q < n) { const u64 x = a[p], y = a[q]; if (x > y) { a[p] = y; a[q] = x; } }
            }
            __syncthreads();
        }
    }
}

__global__ void __launch_bounds__(ADJ_BIG_THREADS)
adj_sort_big_kernel(const u32* __restrict__ start, u64* rows, const u32* __restrict__ big, u32 big_cap, const AdjHeader* __restrict__ hdr)
{
    __shared__ u64 lds[ADJ_BIG_LDS];
    if (hdr->bad) return;
    const u32 n_big = hdr->n_big < big_cap ? hdr->n_big : big_cap;
    for (u32 b = blockIdx.x; b < n_big; b += gridDim.x) {
        const u32 v = big[b];
        const u32 s = start[v], n = start[v + 1] - s;
        u64* a = rows + s;
        if (n <= ADJ_BIG_LDS) {
            for (u32 i = threadIdx.x; i < n; i += ADJ_BIG_THREADS) lds[i] = a[i];
            __syncthreads();
            bitonic_any64(lds, n);
            for (u32 i = threadIdx.x; i < n; i += ADJ_BIG_THREADS) a[i] = lds[i];
            __syncthreads();
        } else {
            __syncthreads();
            bitonic_any64(a, n);
        }
    }
}

__global__ void __launch_bounds__(F3DG_BLOCK)
adj_degree_kernel(u32 N, const u32* __restrict__ start, const u64* __restrict__ rows, u32* __restrict__ deg, unsigned char* __restrict__ boundary,
                  AdjHeader* __restrict__ hdr)
{
    if (hdr->bad) return;
    const u32 v = blockIdx.x * F3DG_BLOCK + threadIdx.x;
    u32 n = 0;
    bool rim = false;
    if (v < N) {
        const u32 s = start[v];
        n = start[v + 1] - s;
        u32 d = 0, run = 0, prev = 0;
        for (u32 i = 0; i < n; i++) {
            const u32 w = (u32)(rows[s + i] >> 32);
            if (i == 0u || w != prev) {
                rim = rim || run == 1u;
                d++;
                run = 1u;
                prev = w;
            } else {
                run++;
            }
        }
        rim = rim || run == 1u;
        deg[v] = d;
        boundary[v] = rim ? 1 : 0;
    }
    const u64 m = __ballot(rim);
    u32 longest = n;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const u32 o = __shfl_down(longest, off, 64);
        longest = o > longest ? o : longest;
    }
    if ((threadIdx.x & 63u) == 0u) {
        if (m) atomicAdd(&hdr->n_boundary, (u32)__popcll(m));
        if (longest) atomicMax(&hdr->max_row, longest);
    }
}

__global__ void __launch_bounds__(F3DG_BLOCK)
adj_emit_kernel(u32 N, u32 F, const u32* __restrict__ start, const u64* __restrict__ rows, const u32* __restrict__ deg_start,
                const AdjHeader* __restrict__ hdr, int* __restrict__ nbr_start, int* __restrict__ nbr)
{
    if (!adj_ready(hdr, N, F)) return;
    const u32 v = blockIdx.x * F3DG_BLOCK + threadIdx.x;
    if (v >= N) return;
    u32 o = deg_start[v];
    nbr_start[v] = (int)o;
    if (v == N - 1u) nbr_start[N] = (int)deg_start[N];
    const u32 s = start[v], n = start[v + 1] - s;
    u32 prev = 0;
    for (u32 i = 0; i < n; i++) {
        const u32 w = (u32)(rows[s + i] >> 32);
        if (i == 0u || w != prev) nbr[o++] = (int)w;        // o < deg_start[v + 1] <= 2E <= 6 F, the caller's capacity
        prev = w;
    }
}

__global__ void __launch_bounds__(F3DG_BLOCK)
mesh_smooth_kernel(u32 N, const int* __restrict__ nbr_start, const int* __restrict__ nbr, const unsigned char* __restrict__ pinned,
                   const float* __restrict__ in, float* __restrict__ out, float s)
{
    const u32 v = blockIdx.x * F3DG_BLOCK + threadIdx.x;
    if (v >= N) return;
    float p[3] = { in[3 * (size_t)v], in[3 * (size_t)v + 1], in[3 * (size_t)v + 2] };
    const int b = nbr_start[v], e = nbr_start[v + 1];
    if (b >= 0 && e > b && !(pinned && pinned[v])) {
        double S[3] = { 0.0, 0.0, 0.0 };
        for (int j = b; j < e; j++) {                       // ascending in w: the row is sorted
            const u32 w = (u32)nbr[j];
            if (w >= N) continue;
            const float* q = in + 3 * (size_t)w;
            S[0] += (double)q[0]; S[1] += (double)q[1]; S[2] += (double)q[2];
        }
        const double d = (double)(e - b);
#pragma unroll
        for (int c = 0; c < 3; c++) p[c] = (float)((double)p[c] + (double)s * (S[c] / d - (double)p[c]));
    }
    out[3 * (size_t)v] = p[0]; out[3 * (size_t)v + 1] = p[1]; out[3 * (size_t)v + 2] = p[2];
}

template <typename I>
__global__ void __launch_bounds__(F3DG_BLOCK)
mesh_normals_kernel(const I* __restrict__ faces, u32 F, u32 N, const float* __restrict__ vertices, const u32* __restrict__ start,
                    const u64* __restrict__ rows, const AdjHeader* __restrict__ hdr, float* __restrict__ normals)
{
    if (!adj_ready(hdr, N, F)) return;                      // no completed adjacency build of this mesh on the workspace
    const u32 v = blockIdx.x * F3DG_BLOCK + threadIdx.x;
    if (v >= N) return;
    const u32 s = start[v], n = start[v + 1] - s;
    double sum[3] = { 0.0, 0.0, 0.0 };
    for (u32 i = 0; i < n; i++) {
        const u64 e = rows[s + i];
        if (!(e & 1ull)) continue;                          // succ == 1: every incident face once
        const u32 f = (u32)(e & 0xFFFFFFFFull) >> 1;
        u32 id[3];
        if (f >= F || !load_face(faces, f, N, id)) continue;        // (not the faces that were counted)
        double P[3][3];
#pragma unroll
        for (int k = 0; k < 3; k++)
#pragma unroll
            for (int c = 0; c < 3; c++) P[k][c] = (double)vertices[3 * (size_t)id[k] + c];
        const double ux = P[1][0] - P[0][0], uy = P[1][1] - P[0][1], uz = P[1][2] - P[0][2];
        const double wx = P[2][0] - P[0][0], wy = P[2][1] - P[0][1], wz = P[2][2] - P[0][2];
        sum[0] += uy * wz - uz * wy;
        sum[1] += uz * wx - ux * wz;
        sum[2] += ux * wy - uy * wx;
    }
    const double len = sqrt((sum[0] * sum[0] + sum[1] * sum[1]) + sum[2] * sum[2]);
    const bool ok = len > 0.0 && len <= 1.7976931348623157e308;       // not zero, not NaN, not infinite
#pragma unroll
    for (int c = 0; c < 3; c++) normals[3 * (size_t)v + c] = ok ? (float)(sum[c] / len) : 0.0f;
}

template <typename I>
int adjacency_impl(hipStream_t s, char* ws, const AdjLayout& L, u32 N, u32 F, const I* faces, int* nbr_start, int* nbr, unsigned char* boundary,
                   long long* h_counts)
{
    AdjHeader* hdr = reinterpret_cast<AdjHeader*>(ws + L.header);
    u32* start = reinterpret_cast<u32*>(ws + L.start);
    u32* fill = reinterpret_cast<u32*>(ws + L.fill);        // the fill counters of the scatter, then the degrees and their scan
    u32* big = reinterpret_cast<u32*>(ws + L.big);
    u64* rows = reinterpret_cast<u64*>(ws + L.rows);
    const u32 nb_f = (F + F3DG_BLOCK - 1) / F3DG_BLOCK, nb_v = (N + F3DG_BLOCK - 1) / F3DG_BLOCK;
    F3DG_HIP_CHECK(hipMemsetAsync(hdr, 0, L.big, s));       // the header, start and fill (their padding included)
    F3DG_KLAUNCH(adj_count_kernel<I>, dim3(nb_f), dim3(F3DG_BLOCK), 0, s, faces, F, N, start, hdr);
    F3DG_KLAUNCH(adj_scan_kernel, dim3(1), dim3(ADJ_BIG_THREADS), 0, s, start, L.n_scan, N, F, 0, hdr);
    F3DG_KLAUNCH(adj_scatter_kernel<I>, dim3(nb_f), dim3(F3DG_BLOCK), 0, s, faces, F, N, (const u32*)start, fill, rows, (const AdjHeader*)hdr);
    F3DG_KLAUNCH(adj_sort_small_kernel, dim3(nb_v), dim3(F3DG_BLOCK), 0, s, N, (const u32*)start, rows, big, L.big_cap, hdr);
    const u32 big_grid = L.big_cap < 2048u ? L.big_cap : 2048u;
    F3DG_KLAUNCH(adj_sort_big_kernel, dim3(big_grid), dim3(ADJ_BIG_THREADS), 0, s, (const u32*)start, rows, (const u32*)big, L.big_cap, (const AdjHeader*)hdr);
    F3DG_HIP_CHECK(hipMemsetAsync(fill, 0, (size_t)L.n_scan * 4, s));
    F3DG_KLAUNCH(adj_degree_kernel, dim3(nb_v), dim3(F3DG_BLOCK), 0, s, N, (const u32*)start, (const u64*)rows, fill, boundary, hdr);
    F3DG_KLAUNCH(adj_scan_kernel, dim3(1), dim3(ADJ_BIG_THREADS), 0, s, fill, L.n_scan, N, F, 1, hdr);
    F3DG_KLAUNCH(adj_emit_kernel, dim3(nb_v), dim3(F3DG_BLOCK), 0, s, N, F, (const u32*)start, (const u64*)rows, (const u32*)fill, (const AdjHeader*)hdr,
                 nbr_start, nbr);
    F3DG_HIP_CHECK(hipGetLastError());
    // the one host read: the counts and whether an id was out of range
    AdjHeader h;
    F3DG_HIP_CHECK(hipMemcpyAsync(&h, hdr, sizeof(AdjHeader), hipMemcpyDeviceToHost, s));
    F3DG_HIP_CHECK(hipStreamSynchronize(s));
    if (h.bad) return F3DG_ERR_BAD_ARG;                     // nothing but the workspace was written
    h_counts[0] = (long long)h.two_e;
    h_counts[1] = (long long)h.n_boundary;
    h_counts[2] = (long long)h.degenerate;
    h_counts[3] = (long long)h.max_row;
    return F3DG_OK;
}

template <typename I>
int normals_impl(hipStream_t s, char* ws, const AdjLayout& L, u32 N, u32 F, const I* faces, const float* vertices, float* normals)
{
    F3DG_KLAUNCH(mesh_normals_kernel<I>, dim3((N + F3DG_BLOCK - 1) / F3DG_BLOCK), dim3(F3DG_BLOCK), 0, s, faces, F, N, vertices,
                 reinterpret_cast<const u32*>(ws + L.start), reinterpret_cast<const u64*>(ws + L.rows), reinterpret_cast<const AdjHeader*>(ws + L.header),
                 normals);
    F3DG_HIP_CHECK(hipGetLastError());
    return F3DG_OK;
}

} // namespace

extern "C" size_t f3dg_mesh_adjacency_workspace_bytes(long long N, long long F)
{
    if (adj_check_sizes(N, F) != F3DG_OK) return 0;
    return adj_layout((u32)N, (u32)F).total;
}

extern "C" int f3dg_mesh_adjacency(void* stream, void* workspace, size_t workspace_bytes, long long N, long long F, const void* faces,
                                   int faces_int32, int* nbr_start, int* nbr, unsigned char* boundary, long long* h_counts)
{
    if (!workspace || !nbr_start || !boundary || !h_counts || ((!faces || !nbr) && F > 0) || ((uintptr_t)workspace & 15u)) return F3DG_ERR_BAD_ARG;
    const int rc = adj_check_sizes(N, F);
    if (rc != F3DG_OK) return rc;
    const AdjLayout L = adj_layout((u32)N, (u32)F);
    if (workspace_bytes < L.total) return F3DG_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    if (F == 0) {                                           // no edges; the header says that no rows are there to read
        F3DG_HIP_CHECK(hipMemsetAsync(workspace, 0, sizeof(AdjHeader), s));
        F3DG_HIP_CHECK(hipMemsetAsync(nbr_start, 0, ((size_t)N + 1) * 4, s));
        F3DG_HIP_CHECK(hipMemsetAsync(boundary, 0, (size_t)N, s));
        F3DG_HIP_CHECK(hipStreamSynchronize(s));
        h_counts[0] = h_counts[1] = h_counts[2] = h_counts[3] = 0;
        return F3DG_OK;
    }
    return faces_int32 ? adjacency_impl(s, (char*)workspace, L, (u32)N, (u32)F, (const int*)faces, nbr_start, nbr, boundary, h_counts)
                       : adjacency_impl(s, (char*)workspace, L, (u32)N, (u32)F, (const long long*)faces, nbr_start, nbr, boundary, h_counts);
}

extern "C" int f3dg_mesh_smooth(void* stream, long long N, const int* nbr_start, const int* nbr, const unsigned char* pinned,
                                const float* vertices_in, float lambda, float mu, int iterations, float* scratch, float* vertices_out)
{
    if (!nbr_start || !vertices_in || !vertices_out || N <= 0 || iterations < 0) return F3DG_ERR_BAD_ARG;
    if (!(lambda > 0.0f && lambda <= 1.0f) || !(mu == 0.0f || mu < -lambda)) return F3DG_ERR_BAD_ARG;         // (a NaN fails both)
    if (N >= (1ll << 31)) return F3DG_ERR_UNSUPPORTED;
    const long long steps = (long long)iterations * (mu == 0.0f ? 1 : 2);
    if (steps > 1 && !scratch) return F3DG_ERR_BAD_ARG;
    if (vertices_in == vertices_out || (scratch && (scratch == vertices_out || scratch == vertices_in))) return F3DG_ERR_BAD_ARG;
    hipStream_t s = (hipStream_t)stream;
    if (steps == 0) {
        F3DG_HIP_CHECK(hipMemcpyAsync(vertices_out, vertices_in, (size_t)N * 12, hipMemcpyDeviceToDevice, s));
        return F3DG_OK;
    }
    const u32 nb = (u32)((N + F3DG_BLOCK - 1) / F3DG_BLOCK);
    const float* src = vertices_in;
    for (long long k = 0; k < steps; k++) {
        float* dst = ((steps - 1 - k) & 1) ? scratch : vertices_out;        // the last step lands in vertices_out
        const float factor = (mu != 0.0f && (k & 1)) ? mu : lambda;
        F3DG_KLAUNCH(mesh_smooth_kernel, dim3(nb), dim3(F3DG_BLOCK), 0, s, (u32)N, nbr_start, nbr, pinned, src, dst, factor);
        src = dst;
    }
    F3DG_HIP_CHECK(hipGetLastError());
    return F3DG_OK;
}

extern "C" int f3dg_mesh_vertex_normals(void* stream, void* workspace, size_t workspace_bytes, long long N, long long F, const void* faces,
                                        int faces_int32, const float* vertices, float* normals)
{
    if (!workspace || !vertices || !normals || (!faces && F > 0) || ((uintptr_t)workspace & 15u)) return F3DG_ERR_BAD_ARG;
    const int rc = adj_check_sizes(N, F);
    if (rc != F3DG_OK) return rc;
    const AdjLayout L = adj_layout((u32)N, (u32)F);
    if (workspace_bytes < L.total) return F3DG_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    if (F == 0) {                                           // no face: every normal is zero
        F3DG_HIP_CHECK(hipMemsetAsync(normals, 0, (size_t)N * 12, s));
        return F3DG_OK;
    }
    return faces_int32 ? normals_impl(s, (char*)workspace, L, (u32)N, (u32)F, (const int*)faces, vertices, normals)
                       : normals_impl(s, (char*)workspace, L, (u32)N, (u32)F, (const long long*)faces, vertices, normals);
}
