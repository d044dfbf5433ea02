// f3dg_mesh.hip -- marching tetrahedra: the integer topology of _unbatched_marching_tetrahedra (src/utils_tetmesh.py:47-138).
//
// The reference sorts six int64 edges per surface tetrahedron with torch.unique(dim=0) and then masks the crossing ones out of the
// result. Only an edge with exactly ONE occupied endpoint ever reaches its output, so this file deduplicates the crossing edges alone
// and never touches the others:
//   occupancy_kernel   sdf > 0 as one bit per point (NaN and 0 are outside), :98
//   classify_kernel    one thread per tetrahedron: range check of the four ids BEFORE anything is indexed with them, case index
//                      sum occ_i 2^i (:126), per-workgroup counts of the one- and two-triangle tetrahedra, cnt[lo] += 1 per crossing edge
//   (scans)            the two count arrays (the ballots and the ranks are f3dg_compact.h's; the arrays are long enough here to keep
//                      the three-launch scan), and cnt -> start: every point `lo` owns the bucket [start[lo], start[lo + 1]) of the
//                      `hi` ends of its crossing edges
//   scatter_kernel     hi into the bucket of lo (integer atomics hand out the slots; their arrival order is erased by the sort below)
//   sort_small_kernel  buckets of at most 32 entries: one thread each, insertion sort in place; longer buckets are queued
//   sort_big_kernel    one 1024-thread workgroup per queued bucket: bitonic network in LDS (up to 8192 entries) or in place
//   (scan)             first-occurrence flags -> rank of every bucket entry = row of that edge in interp_v: buckets are in `lo` order and
//                      sorted by `hi`, so the rows are in ascending lexicographic order by construction, as torch.unique leaves them
//   faces_kernel       one thread per tetrahedron: binary search of its crossing edges in their buckets, the triangle table (:23-43),
//                      rows written at the scanned count plus the rank inside the workgroup (block_rank; the ballots are rebuilt from the
//                      cases, no flag words are stored), one-triangle tetrahedra first, then the two-triangle ones (:131-136); every
//                      thread also writes the (lo, hi) row of the edges it looks up (all writers of a row write the same two values)
// Nothing here is floating-point arithmetic and every count is an integer sum: the outputs are bit-reproducible.
#include "f3dg_common.h"
#include "f3dg_compact.h"

namespace {

#define MESH_SMALL 32u              // longest bucket one thread sorts
#define MESH_BIG_THREADS 1024
#define MESH_BIG_LDS 8192u          // entries of a bucket that is sorted in LDS (32 KB)

struct MeshHeader {                 // first 256 bytes of the workspace
    u32 n_one, n_two;               // surface tetrahedra whose case gives one / two triangles
    u32 bad;                        // 1: a tetrahedron holds an id outside [0, N)
    u32 n_big;                      // buckets queued for sort_big_kernel
    u64 emitted;                    // crossing edges of all surface tetrahedra, duplicates included (M)
    u32 ready;                      // non-zero once the buckets are sorted and ranked: f3dg_marching_tets_emit may read them
    u32 reserved[57];
};

struct MeshLayout {
    size_t header, occ, cases, blk_one, blk_two, cnt, start, big, bucket, first, scan_tmp, total;
    u32 scan_tmp_elems, big_cap;
};

MeshLayout mesh_layout(long long N, long long F, long long cap)
{
    MeshLayout L;
    const size_t nb = (size_t)((F + F3DG_BLOCK - 1) / F3DG_BLOCK);
    size_t o = 0;
    auto take = [&](size_t bytes) { const size_t at = o; o = f3dg_align256(o + bytes); return at; };
    L.header = take(sizeof(MeshHeader));
    L.occ = take((size_t)((N + 63) / 64) * 8);
    L.cases = take((size_t)F);
    L.blk_one = take(nb * 4);
    L.blk_two = take(nb * 4);
    L.cnt = take((size_t)(N + 1) * 4);
    L.start = take((size_t)(N + 1) * 4);
    const size_t big_cap = (size_t)cap / (MESH_SMALL + 1) + 1;          // a queued bucket holds more than MESH_SMALL entries
    L.big_cap = (u32)(big_cap < (size_t)N ? big_cap : (size_t)N);
    L.big = take((size_t)L.big_cap * 4);
    L.bucket = take((size_t)cap * 4);
    L.first = take((size_t)(cap + 1) * 4);
    size_t longest = (size_t)N + 1;
    if ((size_t)cap + 1 > longest) longest = (size_t)cap + 1;
    if (nb > longest) longest = nb;
    L.scan_tmp_elems = (u32)((longest + F3DG_SCAN_CHUNK - 1) / F3DG_SCAN_CHUNK);
    L.scan_tmp = take((size_t)L.scan_tmp_elems * 4);
    L.total = o;
    return L;
}

// the tetrahedron's four ids; false when one of them is outside [0, N) (nothing has been indexed with them yet)
template <typename I>
__device__ __forceinline__ bool load_tet(const I* __restrict__ tets, u32 t, u32 N, u32 v[4])
{
    I w[4];
    if constexpr (sizeof(I) == 8) {
        const longlong2 a = reinterpret_cast<const longlong2*>(tets)[2 * (size_t)t];
        const longlong2 b = reinterpret_cast<const longlong2*>(tets)[2 * (size_t)t + 1];
        w[0] = a.x; w[1] = a.y; w[2] = b.x; w[3] = b.y;
    } else {
        const int4 a = reinterpret_cast<const int4*>(tets)[t];
        w[0] = a.x; w[1] = a.y; w[2] = a.z; w[3] = a.w;
    }
    bool ok = true;
#pragma unroll
    for (int i = 0; i < 4; i++) {
        ok = ok && w[i] >= 0 && w[i] < (I)N;
        v[i] = (u32)w[i];
    }
    return ok;
}

// base_tet_edges, utils_tetmesh.py:43: (0,1) (0,2) (0,3) (1,2) (1,3) (2,3)
__device__ __forceinline__ int edge_a(int e) { return e < 3 ? 0 : (e < 5 ? 1 : 2); }
__device__ __forceinline__ int edge_b(int e) { return e < 3 ? e + 1 : (e < 5 ? e - 1 : 3); }

// triangle_table, utils_tetmesh.py:23-40: tetrahedron edges of the one or two triangles of every case (rows 0 and 15 are empty)
__device__ const signed char k_triangle_table[16][6] = {
    {-1, -1, -1, -1, -1, -1}, {1, 0, 2, -1, -1, -1}, {4, 0, 3, -1, -1, -1}, {1, 4, 2, 1, 3, 4},
    {3, 1, 5, -1, -1, -1},    {2, 3, 0, 2, 5, 3},    {1, 4, 0, 1, 5, 4},    {4, 2, 5, -1, -1, -1},
    {4, 5, 2, -1, -1, -1},    {4, 1, 0, 4, 5, 1},    {3, 2, 0, 3, 5, 2},    {1, 3, 5, -1, -1, -1},
    {4, 1, 2, 4, 3, 1},       {3, 0, 4, -1, -1, -1}, {2, 0, 1, -1, -1, -1}, {-1, -1, -1, -1, -1, -1}};

// num_triangles_table, :42: one triangle when one or three corners are occupied, two when two are
__device__ __forceinline__ u32 case_triangles(u32 c) { const u32 p = __popc(c); return p == 2u ? 2u : ((p == 1u || p == 3u) ? 1u : 0u); }

__global__ void __launch_bounds__(F3DG_BLOCK)
occupancy_kernel(const float* __restrict__ sdf, u32 N, u64* __restrict__ occ)
{
    const u32 i = blockIdx.x * F3DG_BLOCK + threadIdx.x;
    const bool in = i < N && sdf[i] > 0.0f;            // NaN > 0 is false
    store_flag_word(occ, __ballot(in), i, N);
}

template <typename I>
__global__ void __launch_bounds__(F3DG_BLOCK)
classify_kernel(const I* __restrict__ tets, u32 F, u32 N, const u64* __restrict__ occ, unsigned char* __restrict__ cases,
                u32* __restrict__ cnt, u32* __restrict__ blk_one, u32* __restrict__ blk_two, MeshHeader* __restrict__ hdr)
{
    __shared__ u32 w_one[F3DG_BLOCK / 64], w_two[F3DG_BLOCK / 64], w_emit[F3DG_BLOCK / 64];
    const u32 t = blockIdx.x * F3DG_BLOCK + threadIdx.x;
    u32 c = 0, emitted = 0;
    if (t < F) {
        u32 v[4];
        if (load_tet(tets, t, N, v)) {
#pragma unroll
            for (int i = 0; i < 4; i++) c |= (u32)((occ[v[i] >> 6] >> (v[i] & 63u)) & 1ull) << i;
            if (c != 0u && c != 15u) {
#pragma unroll
                for (int e = 0; e < 6; e++) {
                    const int a = edge_a(e), b = edge_b(e);
                    if (((c >> a) ^ (c >> b)) & 1u) {           // exactly one end occupied: the ids differ
                        atomicAdd(&cnt[v[a] < v[b] ? v[a] : v[b]], 1u);
                        emitted++;
                    }
                }
            }
        } else {
            atomicOr(&hdr->bad, 1u);
        }
        cases[t] = (unsigned char)c;
    }
    const u32 nt = case_triangles(c);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) emitted += __shfl_down(emitted, off, 64);
    if ((threadIdx.x & 63) == 0) w_emit[threadIdx.x >> 6] = emitted;
    wave_ballot(nt == 1u, w_one);
    wave_ballot(nt == 2u, w_two);
    __syncthreads();
    if (threadIdx.x == 0) {
        const u32 o = block_count(w_one), w = block_count(w_two), m = block_count(w_emit);
        blk_one[blockIdx.x] = o;
        blk_two[blockIdx.x] = w;
        if (o) atomicAdd(&hdr->n_one, o);
        if (w) atomicAdd(&hdr->n_two, w);
        if (m) atomicAdd(&hdr->emitted, (u64)m);
    }
}

template <typename I>
__global__ void __launch_bounds__(F3DG_BLOCK)
scatter_kernel(const I* __restrict__ tets, u32 F, u32 N, const unsigned char* __restrict__ cases, const u32* __restrict__ start,
               u32* __restrict__ fill, u32* __restrict__ bucket)
{
    const u32 t = blockIdx.x * F3DG_BLOCK + threadIdx.x;
    if (t >= F) return;
    const u32 c = cases[t];
    if (c == 0u || c == 15u) return;           // (a tetrahedron with an id out of range was given case 0)
    u32 v[4];
    load_tet(tets, t, N, v);
#pragma unroll
    for (int e = 0; e < 6; e++) {
        const int a = edge_a(e), b = edge_b(e);
        if (((c >> a) ^ (c >> b)) & 1u) {
            const u32 lo = v[a] < v[b] ? v[a] : v[b], hi = v[a] < v[b] ? v[b] : v[a];
            bucket[start[lo] + atomicAdd(&fill[lo], 1u)] = hi;
        }
    }
}

__device__ __forceinline__ void mark_first(const u32* a, u32* first, u32 i) { first[i] = (i == 0u || a[i] != a[i - 1u]) ? 1u : 0u; }

__global__ void __launch_bounds__(F3DG_BLOCK)
sort_small_kernel(u32 N, const u32* __restrict__ start, u32* bucket, u32* __restrict__ first, u32* __restrict__ big, u32 big_cap,
                  MeshHeader* __restrict__ hdr)
{
    const u32 lo = blockIdx.x * F3DG_BLOCK + threadIdx.x;
    if (lo >= N) return;
    const u32 s = start[lo], n = start[lo + 1] - s;
    if (n == 0u) return;
    if (n > MESH_SMALL) {
        const u32 slot = atomicAdd(&hdr->n_big, 1u);
        if (slot < big_cap) big[slot] = lo;         // (always: big_cap counts every bucket that can be this long)
        return;
    }
    u32* a = bucket + s;
    for (u32 i = 1; i < n; i++) {
        const u32 x = a[i];
        u32 j = i;
        while (j > 0u && a[j - 1u] > x) { a[j] = a[j - 1u]; j--; }
        a[j] = x;
    }
    for (u32 i = 0; i < n; i++) mark_first(a, first + s, i);
}

// Bitonic network over a[0 .. n), any n: every compare-exchange puts the larger value at the HIGHER index, so the positions from n
// up to the next power of two behave as +infinity that never moves and are simply skipped.
__device__ void bitonic_any(u32* a, u32 n)
{
    for (u64 k64 = 2; (k64 >> 1) < n; k64 <<= 1) {
        const u32 k = (u32)k64, half = (u32)(k64 >> 1);       // (k = 2^32 wraps to 0 only where blk is 0)
        for (u32 base = 0; base < n; base += MESH_BIG_THREADS) {      // pair index i: block i / half, offset i % half
            const u32 i = base + threadIdx.x;
            const u32 blk = i / half, off = i % half;
            const u32 p = blk * k + off, q = blk * k + (k - 1u - off);
            if (q < n) { const u32 x = a[p], y = a[q]; if (x > y) { a[p] = y; a[q] = x; } }
        }
        __syncthreads();
        for (u32 j = half >> 1; j > 0u; j >>= 1) {
            for (u32 base = 0; base < n; base += MESH_BIG_THREADS) {
                const u32 i = base + threadIdx.x;
                const u32 p = 2u * j * (i / j) + (i % j), q = p + j;
                if (q < n) { const u32 x = a[p], y = a[q]; if (x > y) { a[p] = y; a[q] = x; } }
            }
            __syncthreads();
        }
    }
}

__global__ void __launch_bounds__(MESH_BIG_THREADS)
sort_big_kernel(const u32* __restrict__ start, u32* bucket, u32* __restrict__ first, const u32* __restrict__ big, u32 big_cap,
                const MeshHeader* __restrict__ hdr)
{
    __shared__ u32 lds[MESH_BIG_LDS];
    const u32 n_big = hdr->n_big < big_cap ? hdr->n_big : big_cap;
    for (u32 b = blockIdx.x; b < n_big; b += gridDim.x) {
        const u32 lo = big[b];
        const u32 s = start[lo], n = start[lo + 1] - s;
        u32* a = bucket + s;
        if (n <= MESH_BIG_LDS) {
            for (u32 i = threadIdx.x; i < n; i += MESH_BIG_THREADS) lds[i] = a[i];
            __syncthreads();
            bitonic_any(lds, n);
            for (u32 i = threadIdx.x; i < n; i += MESH_BIG_THREADS) {
                a[i] = lds[i];
                mark_first(lds, first + s, i);
            }
            __syncthreads();
        } else {
            __syncthreads();
            bitonic_any(a, n);
            for (u32 i = threadIdx.x; i < n; i += MESH_BIG_THREADS) mark_first(a, first + s, i);
        }
    }
}

template <typename I>
__global__ void __launch_bounds__(F3DG_BLOCK)
faces_kernel(const I* __restrict__ tets, u32 F, u32 N, const unsigned char* __restrict__ cases, const u32* __restrict__ start,
             const u32* __restrict__ bucket, const u32* __restrict__ rank, const u32* __restrict__ blk_one, const u32* __restrict__ blk_two,
             const MeshHeader* __restrict__ hdr, u64 n_one_total, long long* __restrict__ interp_v, long long* __restrict__ faces)
{
    if (!hdr->ready) return;            // no completed f3dg_marching_tets_count on this workspace: nothing to index
    __shared__ u32 w_one[F3DG_BLOCK / 64], w_two[F3DG_BLOCK / 64];
    const u32 t = blockIdx.x * F3DG_BLOCK + threadIdx.x;
    const u32 c = t < F ? cases[t] : 0u;
    const u32 nt = case_triangles(c);
    const u64 m_one = wave_ballot(nt == 1u, w_one), m_two = wave_ballot(nt == 2u, w_two);
    __syncthreads();
    if (nt == 0u) return;
    const u64 at = nt == 1u ? (u64)blk_one[blockIdx.x] + block_rank(m_one, w_one) : (u64)blk_two[blockIdx.x] + block_rank(m_two, w_two);

    u32 v[4];
    load_tet(tets, t, N, v);
    u32 row[6] = {0u, 0u, 0u, 0u, 0u, 0u};
#pragma unroll
    for (int e = 0; e < 6; e++) {
        const int a = edge_a(e), b = edge_b(e);
        if (((c >> a) ^ (c >> b)) & 1u) {
            const u32 lo = v[a] < v[b] ? v[a] : v[b], hi = v[a] < v[b] ? v[b] : v[a];
            u32 l = start[lo], r = start[lo + 1];      // first entry of the bucket that is >= hi (hi is in the bucket)
            while (l < r) {
                const u32 m = l + ((r - l) >> 1);
                if (bucket[m] < hi) l = m + 1u; else r = m;
            }
            const u32 k = rank[l];
            row[e] = k;
            interp_v[2 * (size_t)k] = (long long)lo;
            interp_v[2 * (size_t)k + 1] = (long long)hi;
        }
    }
    auto pick = [&](int e) -> long long {
        u32 x = row[0];
#pragma unroll
        for (int i = 1; i < 6; i++) x = e == i ? row[i] : x;
        return (long long)x;
    };
    const signed char* tri = k_triangle_table[c];
    long long* out = faces + 3 * (nt == 1u ? (size_t)at : (size_t)n_one_total + 2 * (size_t)at);
    for (u32 i = 0; i < 3u * nt; i++) out[i] = pick(tri[i]);
}

int check_sizes(long long N, long long F, long long cap)
{
    if (N <= 0 || F < 0 || N >= (1ll << 31) || F >= (1ll << 31)) return F3DG_ERR_BAD_ARG;
    if (cap < 0 || cap > 4 * F) return F3DG_ERR_BAD_ARG;
    return F3DG_OK;
}

template <typename I>
int count_impl(hipStream_t s, char* ws, const MeshLayout& L, u32 N, u32 F, long long cap, const float* sdf, const I* tets, long long* h_counts)
{
    MeshHeader* hdr = reinterpret_cast<MeshHeader*>(ws + L.header);
    u64* occ = reinterpret_cast<u64*>(ws + L.occ);
    unsigned char* cases = reinterpret_cast<unsigned char*>(ws + L.cases);
    u32* blk_one = reinterpret_cast<u32*>(ws + L.blk_one);
    u32* blk_two = reinterpret_cast<u32*>(ws + L.blk_two);
    u32* cnt = reinterpret_cast<u32*>(ws + L.cnt);
    u32* start = reinterpret_cast<u32*>(ws + L.start);
    u32* big = reinterpret_cast<u32*>(ws + L.big);
    u32* bucket = reinterpret_cast<u32*>(ws + L.bucket);
    u32* first = reinterpret_cast<u32*>(ws + L.first);
    u32* scan_tmp = reinterpret_cast<u32*>(ws + L.scan_tmp);
    const u32 nb = (F + F3DG_BLOCK - 1) / F3DG_BLOCK, nbN = (N + F3DG_BLOCK - 1) / F3DG_BLOCK;

    F3DG_HIP_CHECK(hipMemsetAsync(hdr, 0, sizeof(MeshHeader), s));
    F3DG_HIP_CHECK(hipMemsetAsync(cnt, 0, ((size_t)N + 1) * 4, s));
    F3DG_KLAUNCH(occupancy_kernel, dim3(nbN), dim3(F3DG_BLOCK), 0, s, sdf, N, occ);
    F3DG_KLAUNCH(classify_kernel<I>, dim3(nb), dim3(F3DG_BLOCK), 0, s, tets, F, N, occ, cases, cnt, blk_one, blk_two, hdr);
    F3DG_HIP_CHECK(hipGetLastError());
    // host read 1 of 2: the counts (and whether an id was out of range)
    MeshHeader h;
    F3DG_HIP_CHECK(hipMemcpyAsync(&h, hdr, sizeof(MeshHeader), hipMemcpyDeviceToHost, s));
    F3DG_HIP_CHECK(hipStreamSynchronize(s));
    if (h.bad) return F3DG_ERR_BAD_ARG;
    h_counts[0] = 0;
    h_counts[1] = (long long)h.n_one;
    h_counts[2] = (long long)h.n_two;
    h_counts[3] = (long long)h.emitted;
    if (h.emitted > (u64)cap) return F3DG_ERR_OVERFLOW;
    if (h.emitted >= 0x80000000ull) return F3DG_ERR_UNSUPPORTED;        // bucket positions are 32-bit
    if (h.emitted == 0) return F3DG_OK;
    const u32 M = (u32)h.emitted;

    int rc = f3dg_launch_scan_inclusive(s, cnt, start, (u64)N + 1, scan_tmp, L.scan_tmp_elems, 1, nullptr);
    if (rc != F3DG_OK) return rc;
    // the two count arrays keep the three-launch scan: at the mesh path's size they hold 125,611 counts each, 31 rounds of 4,096 for
    // the single workgroup of compact_scan_counts, which measured slower than these six launches (profiles/mesh_compaction_refactor.md)
    rc = f3dg_launch_scan_inclusive(s, blk_one, blk_one, (u64)nb, scan_tmp, L.scan_tmp_elems, 1, nullptr);
    if (rc != F3DG_OK) return rc;
    rc = f3dg_launch_scan_inclusive(s, blk_two, blk_two, (u64)nb, scan_tmp, L.scan_tmp_elems, 1, nullptr);
    if (rc != F3DG_OK) return rc;
    F3DG_HIP_CHECK(hipMemsetAsync(cnt, 0, (size_t)N * 4, s));         // from here on: the fill count of every bucket
    F3DG_HIP_CHECK(hipMemsetAsync(first + M, 0, 4, s));
    F3DG_KLAUNCH(scatter_kernel<I>, dim3(nb), dim3(F3DG_BLOCK), 0, s, tets, F, N, cases, start, cnt, bucket);
    F3DG_KLAUNCH(sort_small_kernel, dim3(nbN), dim3(F3DG_BLOCK), 0, s, N, start, bucket, first, big, L.big_cap, hdr);
    const u32 big_grid = L.big_cap < 2048u ? L.big_cap : 2048u;
    F3DG_KLAUNCH(sort_big_kernel, dim3(big_grid), dim3(MESH_BIG_THREADS), 0, s, start, bucket, first, big, L.big_cap, hdr);
    F3DG_HIP_CHECK(hipGetLastError());
    rc = f3dg_launch_scan_inclusive(s, first, first, (u64)M + 1, scan_tmp, L.scan_tmp_elems, 1, nullptr);
    if (rc != F3DG_OK) return rc;
    // host read 2 of 2: E, the number of unique crossing edges
    u32 E = 0;
    F3DG_HIP_CHECK(hipMemcpyAsync(&E, first + M, 4, hipMemcpyDeviceToHost, s));
    F3DG_HIP_CHECK(hipStreamSynchronize(s));
    F3DG_HIP_CHECK(hipMemsetAsync(&hdr->ready, 1, 4, s));
    h_counts[0] = (long long)E;
    return F3DG_OK;
}

template <typename I>
int emit_impl(hipStream_t s, char* ws, const MeshLayout& L, u32 N, u32 F, const I* tets, long long n_one, long long* interp_v, long long* faces)
{
    const u32 nb = (F + F3DG_BLOCK - 1) / F3DG_BLOCK;
    F3DG_KLAUNCH(faces_kernel<I>, dim3(nb), dim3(F3DG_BLOCK), 0, s, tets, F, N, reinterpret_cast<const unsigned char*>(ws + L.cases),
                 reinterpret_cast<const u32*>(ws + L.start), reinterpret_cast<const u32*>(ws + L.bucket),
                 reinterpret_cast<const u32*>(ws + L.first), reinterpret_cast<const u32*>(ws + L.blk_one),
                 reinterpret_cast<const u32*>(ws + L.blk_two), reinterpret_cast<const MeshHeader*>(ws + L.header), (u64)n_one, interp_v, faces);
    F3DG_HIP_CHECK(hipGetLastError());
    return F3DG_OK;
}

} // namespace

extern "C" size_t f3dg_marching_tets_workspace_bytes(long long N, long long F, long long max_edges)
{
    if (check_sizes(N, F, max_edges) != F3DG_OK) return 0;
    return mesh_layout(N, F, max_edges).total;
}

extern "C" int f3dg_marching_tets_count(void* stream, void* workspace, size_t workspace_bytes, long long N, long long F, long long max_edges,
                                        const float* sdf, const void* tets, int tets_int32, long long* h_counts)
{
    if (!workspace || !sdf || !h_counts || (!tets && F > 0)) return F3DG_ERR_BAD_ARG;
    const int rc = check_sizes(N, F, max_edges);
    if (rc != F3DG_OK) return rc;
    const MeshLayout L = mesh_layout(N, F, max_edges);
    if (workspace_bytes < L.total) return F3DG_ERR_WORKSPACE;
    h_counts[0] = h_counts[1] = h_counts[2] = h_counts[3] = 0;
    if (F == 0) return F3DG_OK;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    char* ws = reinterpret_cast<char*>(workspace);
    return tets_int32 ? count_impl(s, ws, L, (u32)N, (u32)F, max_edges, sdf, reinterpret_cast<const int*>(tets), h_counts)
                      : count_impl(s, ws, L, (u32)N, (u32)F, max_edges, sdf, reinterpret_cast<const long long*>(tets), h_counts);
}

extern "C" int f3dg_marching_tets_emit(void* stream, void* workspace, size_t workspace_bytes, long long N, long long F, long long max_edges,
                                       const void* tets, int tets_int32, long long n_one, long long* interp_v, long long* faces)
{
    if (!workspace || !tets || !interp_v || !faces || n_one < 0) return F3DG_ERR_BAD_ARG;
    const int rc = check_sizes(N, F, max_edges);
    if (rc != F3DG_OK) return rc;
    if (F == 0) return F3DG_ERR_BAD_ARG;            // nothing was counted: there is nothing to write
    const MeshLayout L = mesh_layout(N, F, max_edges);
    if (workspace_bytes < L.total) return F3DG_ERR_WORKSPACE;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    char* ws = reinterpret_cast<char*>(workspace);
    return tets_int32 ? emit_impl(s, ws, L, (u32)N, (u32)F, reinterpret_cast<const int*>(tets), n_one, interp_v, faces)
                      : emit_impl(s, ws, L, (u32)N, (u32)F, reinterpret_cast<const long long*>(tets), n_one, interp_v, faces);
}
