// f3dg_mesh_simplify.hip -- mesh reduction by uniform-grid vertex clustering (Rossignac-Borrel): the vertices of a grid cell become one
// vertex, placed at the cell's least vertex id (`root`: grid welding at a small cell), at the members' mean, or where the regularised
// quadric of the members' faces is least (Lindstrom's use of the Garland-Heckbert quadrics); faces that collapse and faces that repeat
// a set of three clusters go, the rest is compacted. The semantics are this project's, stated in include/f3dg.h and DESIGN.md section
// 3g-septies; tests/mesh_simplify_truth.py restates them in float64 numpy. Integer atomics only, no float atomics, no sum that depends
// on arrival order: every output is a function of the input alone, equal to the restatement to the bit.
//
// Grouping: a LEAST-ID HASH SET, used twice. An open-addressed table of 32-bit ids (empty = 0xFFFFFFFF, a power of two of at least
// twice the items). An item probes from the hash of its key: an empty slot is claimed by compare-and-swap with the item's own id; for
// an occupied slot the OWNER's key is recomputed from the immutable inputs, and if it is the item's key the item's id goes into the
// slot by atomicMin. A slot's key never changes once it is claimed (only ids of that key are ever written into it), so after the
// insert launch a lookup returns the least id of the key, whatever order the inserts arrived in. No thread waits on another thread's
// write; a probe sequence is bounded by the capacity. Inside the insert launches every access to a table word is a device-scope atomic.
//   ms_insert_kernel       one thread per vertex and per face: the vertex's cell (non-finite or out of range: hdr->bad) and its
//                          insert; the range check of the face's ids. EVERY refusal is found here; every later kernel returns on it
//   ms_root_kernel         one thread per vertex: root[v] = the least id of its cell, cnt[root] += 1, the number of clusters
//   ms_scan_kernel         one 1024-thread workgroup: cnt -> start in place (scan_array_in_place, f3dg_scan.h)
//   ms_scatter_kernel      one thread per vertex: into its root's member row (an integer atomicAdd on the row's fill counter hands out
//                          the slots; the sort below erases their arrival order)
//   ms_sort_small_kernel   rows of at most 32 members: one thread each, insertion sort; longer rows are queued; the longest row
//   ms_sort_big_kernel     one 1024-thread workgroup per queued row: bitonic network in LDS (up to 4,096 members) or in place
//   ms_face_insert_kernel  one thread per face: degenerate / collapsed are counted, every other face is inserted under the sorted
//                          triple of its corners' roots
//   ms_face_flag_kernel    one thread per face: it survives iff the lookup of its triple returns itself (else: a duplicate); the flag
//                          word and workgroup count (f3dg_compact.h), and one bit per used root (atomicOr: order-free)
//   ms_vcount_kernel / ms_finish_kernel   the used roots per 256 vertices; one workgroup scans both count arrays, totals and stamp
//   ms_place_kernel        one thread per vertex: vertex_map; the thread of a used root walks its member row (twice for `quadric`, the
//                          second time over the members' sorted incidence rows in a completed f3dg_mesh_adjacency workspace)
//   ms_emit_faces_kernel   one thread per face at its compact_rank, in the new numbering
#include "f3dg_common.h"
#include "f3dg_compact.h"
#include "f3dg_mesh_adjacency.h"

namespace {

#define MS_EMPTY 0xFFFFFFFFu
#define MS_SMALL 32u                // longest member row one thread sorts
#define MS_BIG_THREADS 1024
#define MS_BIG_LDS 4096u            // members of a row that is sorted in LDS (16 KB of u32)
#define MS_SCAN_WAVES (MS_BIG_THREADS / 64)
#define MS_SCAN_ITEMS 16
#define MS_READY 0x6D73696Du
#define MS_MIN_CAPACITY 16ull
#define MS_CELLS 2097152.0          // 2^21 cells per axis
#define MS_BAD_NONFINITE 1u
#define MS_BAD_CELL 2u
#define MS_BAD_FACE 4u

struct MsHeader {                   // first 256 bytes of the workspace
    u32 bad;                        // MS_BAD_* bits: a non-finite coordinate, a cell index out of range, a face id outside [0, N)
    u32 clusters;                   // occupied cells
    u32 degenerate, collapsed, duplicate;       // faces dropped, by reason
    u32 max_row;                    // members of the largest cluster
    u32 n_big;                      // rows queued for ms_sort_big_kernel
    u32 ready;                      // MS_READY once the counts are scanned: f3dg_mesh_simplify_emit may read the workspace
    u32 N, F;                       // the mesh it was counted on
    u64 n_faces, n_vertices;        // surviving faces, used clusters
    double cell;                    // the cell size of the count (the bound of the quadric step)
    u32 reserved[48];
};
static_assert(sizeof(MsHeader) == 256, "the header is the first 256 bytes");

struct MsLayout {
    size_t header, vtab, ftab, root, start, fill, members, big, flags_f, flags_v, blk_f, blk_v, total;
    u64 cap_v, cap_f;               // slots of the two tables
    u32 n_scan, big_cap;            // entries of start / fill (N + 1 rounded up to whole scan items), capacity of the queue
    CompactPlan f, v;               // of the faces / vertices
};

// slots of a table for `items` items: a power of two, at least twice the items
u64 ms_capacity(u64 items)
{
    u64 c = MS_MIN_CAPACITY;
    while (c < 2ull * items) c <<= 1;
    return c;
}

MsLayout ms_layout(u32 N, u32 F)
{
    MsLayout L;
    L.cap_v = ms_capacity(N);
    L.cap_f = ms_capacity(F);
    L.n_scan = (u32)(((u64)N + 1 + MS_SCAN_ITEMS - 1) / MS_SCAN_ITEMS * MS_SCAN_ITEMS);
    L.big_cap = N / (MS_SMALL + 1u) + 1u;                    // a queued row holds more than MS_SMALL of the N members
    L.f = compact_plan(F);
    L.v = compact_plan(N);
    L.header = 0;
    L.vtab = f3dg_align256(sizeof(MsHeader));
    L.ftab = L.vtab + f3dg_align256((size_t)L.cap_v * 4);
    L.root = L.ftab + f3dg_align256((size_t)L.cap_f * 4);
    L.start = L.root + f3dg_align256((size_t)N * 4);
    L.fill = L.start + f3dg_align256((size_t)L.n_scan * 4);          // directly behind start: one memset clears both
    L.members = L.fill + f3dg_align256((size_t)L.n_scan * 4);
    L.big = L.members + f3dg_align256((size_t)N * 4);
    L.flags_f = L.big + f3dg_align256((size_t)L.big_cap * 4);
    L.flags_v = L.flags_f + L.f.flag_bytes;
    L.blk_f = L.flags_v + L.v.flag_bytes;
    L.blk_v = L.blk_f + L.f.count_bytes;
    L.total = L.blk_v + L.v.count_bytes;
    return L;
}

// F3DG_OK, or why the sizes are refused
int ms_check_sizes(long long N, long long F)
{
    if (N <= 0 || F < 0) return F3DG_ERR_BAD_ARG;
    if (N >= (1ll << 31) || F >= (1ll << 31)) return F3DG_ERR_UNSUPPORTED;
    return F3DG_OK;
}

struct Grid { double ox, oy, oz, cell; };

// ------------------------------------------------------------------------------------------------ keys
// the cell key of vertex v, or which MS_BAD_* bit it raises. One subtraction, one division, floor, per axis.
__device__ __forceinline__ u32 cell_key(const float* __restrict__ vertices, u32 v, const Grid& g, u64& key)
{
    const float x = vertices[3 * (size_t)v], y = vertices[3 * (size_t)v + 1], z = vertices[3 * (size_t)v + 2];
    if (!(fabsf(x) <= 3.402823466e38f) || !(fabsf(y) <= 3.402823466e38f) || !(fabsf(z) <= 3.402823466e38f)) return MS_BAD_NONFINITE;      // (a NaN fails)
    const double cx = floor(((double)x - g.ox) / g.cell), cy = floor(((double)y - g.oy) / g.cell), cz = floor(((double)z - g.oz) / g.cell);
    if (!(cx >= 0.0 && cx < MS_CELLS) || !(cy >= 0.0 && cy < MS_CELLS) || !(cz >= 0.0 && cz < MS_CELLS)) return MS_BAD_CELL;
    key = (u64)cx | (u64)cy << 21 | (u64)cz << 42;
    return 0u;
}

struct VertexKeyOf {                // the key of a vertex that is in the table: it passed cell_key
    const float* vertices;
    Grid g;
    __device__ __forceinline__ u64 operator()(u32 v) const { u64 k = 0; cell_key(vertices, v, g, k); return k; }
};

struct Tri {
    u32 a, b, c;
    __device__ __forceinline__ bool operator==(const Tri& o) const { return a == o.a && b == o.b && c == o.c; }
};

__device__ __forceinline__ Tri sorted_tri(u32 a, u32 b, u32 c)
{
    u32 t;
    if (a > b) { t = a; a = b; b = t; }
    if (b > c) { t = b; b = c; c = t; }
    if (a > b) { t = a; a = b; b = t; }
    return Tri{ a, b, c };
}

// how a face is classed before the duplicates are looked for
#define MS_FACE_BAD 0
#define MS_FACE_DEGENERATE 1
#define MS_FACE_COLLAPSED 2
#define MS_FACE_LIVE 3
template <typename I>
__device__ __forceinline__ int face_class(const I* __restrict__ faces, u32 f, u32 N, const u32* __restrict__ root, Tri& key)
{
    u32 v[3];
    if (!load_face(faces, f, N, v)) return MS_FACE_BAD;                 // (not after a count that found no bad id)
    if (degenerate(v)) return MS_FACE_DEGENERATE;
    const u32 r[3] = { root[v[0]], root[v[1]], root[v[2]] };
    if (degenerate(r)) return MS_FACE_COLLAPSED;
    key = sorted_tri(r[0], r[1], r[2]);
    return MS_FACE_LIVE;
}

template <typename I>
struct FaceKeyOf {                  // the key of a face that is in the table: it is live
    const I* faces;
    const u32* root;
    u32 N;
    __device__ __forceinline__ Tri operator()(u32 f) const { Tri k{ MS_EMPTY, MS_EMPTY, MS_EMPTY }; face_class(faces, f, N, root, k); return k; }
};

__device__ __forceinline__ u32 mix64(u64 k)
{
    k ^= k >> 33; k *= 0xff51afd7ed558ccdull; k ^= k >> 33; k *= 0xc4ceb9fe1a85ec53ull; k ^= k >> 33;
    return (u32)k;
}
__device__ __forceinline__ u32 hash_of(u64 key) { return mix64(key); }
__device__ __forceinline__ u32 hash_of(const Tri& t) { return mix64(((u64)t.a << 32 | t.b) ^ (u64)t.c * 0x9E3779B97F4A7C15ull); }

// ------------------------------------------------------------------------------------------------ the least-id hash set
// table[0 .. mask]: mask + 1 slots, a power of two. At most mask + 1 probes, and the table is at most half full.
template <typename K, typename KeyOf>
__device__ __forceinline__ void least_id_insert(u32* table, u32 mask, u32 id, const K& key, const KeyOf& key_of)
{
    u32 slot = hash_of(key) & mask;
    for (u32 p = 0;; p++) {
        u32 cur = __hip_atomic_load(table + slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (cur == MS_EMPTY) {
            cur = atomicCAS(table + slot, MS_EMPTY, id);
            if (cur == MS_EMPTY) return;                    // claimed: the slot's key is this item's from now on
        }
        if (key_of(cur) == key) { atomicMin(table + slot, id); return; }
        if (p == mask) return;
        slot = (slot + 1u) & mask;
    }
}

// the least id of `key` after the insert launch; MS_EMPTY where the key is not in the table
template <typename K, typename KeyOf>
__device__ __forceinline__ u32 least_id_lookup(const u32* __restrict__ table, u32 mask, const K& key, const KeyOf& key_of)
{
    u32 slot = hash_of(key) & mask;
    for (u32 p = 0;; p++) {
        const u32 cur = table[slot];
        if (cur == MS_EMPTY) return MS_EMPTY;
        if (key_of(cur) == key) return cur;
        if (p == mask) return MS_EMPTY;
        slot = (slot + 1u) & mask;
    }
}

// adds the popcount of the wave's ballot to *counter
__device__ __forceinline__ void wave_count(bool flag, u32* counter)
{
    const u64 m = __ballot(flag);
    if ((threadIdx.x & 63u) == 0u && m) atomicAdd(counter, (u32)__popcll(m));
}

// ------------------------------------------------------------------------------------------------ clusters
template <typename I>
__global__ void __launch_bounds__(F3DG_BLOCK)
ms_insert_kernel(const float* __restrict__ vertices, u32 N, const I* __restrict__ faces, u32 F, Grid g, u32* vtab, u32 mask_v, MsHeader* __restrict__ hdr)
{
    const u32 i = blockIdx.x * F3DG_BLOCK + threadIdx.x;
    u32 bad = 0;
    if (i < N) {
        u64 key = 0;
        bad = cell_key(vertices, i, g, key);
        if (!bad) least_id_insert(vtab, mask_v, i, key, VertexKeyOf{ vertices, g });
    }
    if (i < F) {
        u32 v[3];
        if (!load_face(faces, i, N, v)) bad |= MS_BAD_FACE;
    }
    if (bad) atomicOr(&hdr->bad, bad);
}

__global__ void __launch_bounds__(F3DG_BLOCK)
ms_root_kernel(const float* __restrict__ vertices, u32 N, Grid g, const u32* __restrict__ vtab, u32 mask_v, u32* __restrict__ root, u32* __restrict__ cnt,
               MsHeader* __restrict__ hdr)
{
    if (hdr->bad) return;
    const u32 v = blockIdx.x * F3DG_BLOCK + threadIdx.x;
    bool is_root = false;
    if (v < N) {
        const VertexKeyOf key_of{ vertices, g };
        u32 r = least_id_lookup(vtab, mask_v, key_of(v), key_of);
        if (r >= N) r = v;                                  // (not after the insert launch)
        root[v] = r;
        atomicAdd(&cnt[r], 1u);
        is_root = r == v;
    }
    wave_count(is_root, &hdr->clusters);
}

// cnt[0, n_scan) -> its exclusive prefix sums, in place, by one workgroup (cnt[N] = 0 comes out as N)
__global__ void __launch_bounds__(MS_BIG_THREADS)
ms_scan_kernel(u32* __restrict__ a, u32 n_scan, const MsHeader* __restrict__ hdr)
{
    __shared__ u64 wtot[MS_SCAN_WAVES];
    if (hdr->bad) return;                                   // (the whole workgroup: the flag was set by an earlier launch)
    scan_array_in_place<MS_SCAN_WAVES, MS_SCAN_ITEMS, u64>(a, n_scan, 0u, wtot);
}

__global__ void __launch_bounds__(F3DG_BLOCK)
ms_scatter_kernel(u32 N, const u32* __restrict__ root, const u32* __restrict__ start, u32* __restrict__ fill, u32* __restrict__ members,
                  const MsHeader* __restrict__ hdr)
{
    if (hdr->bad) return;
    const u32 v = blockIdx.x * F3DG_BLOCK + threadIdx.x;
    if (v >= N) return;
    const u32 r = root[v];
    const u32 slot = start[r] + atomicAdd(&fill[r], 1u);
    if (slot < start[r + 1u]) members[slot] = v;            // (always: the row was counted from these roots)
}

__global__ void __launch_bounds__(F3DG_BLOCK)
ms_sort_small_kernel(u32 N, const u32* __restrict__ start, u32* members, u32* __restrict__ big, u32 big_cap, MsHeader* __restrict__ hdr)
{
    if (hdr->bad) return;
    const u32 v = blockIdx.x * F3DG_BLOCK + threadIdx.x;
    u32 n = 0;
    if (v < N) {
        const u32 s = start[v];
        n = start[v + 1] - s;                               // 0 for a vertex that is not a root
        if (n > MS_SMALL) {
            const u32 slot = atomicAdd(&hdr->n_big, 1u);
            if (slot < big_cap) big[slot] = v;              // (always: big_cap counts every row that can be this long)
        } else {
            u32* a = members + s;
            for (u32 i = 1; i < n; i++) {
                const u32 x = a[i];
                u32 j = i;
                while (j > 0u && a[j - 1u] > x) { a[j] = a[j - 1u]; j--; }
                a[j] = x;
            }
        }
    }
    u32 longest = n;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const u32 o = __shfl_down(longest, off, 64);
        longest = o > longest ? o : longest;
    }
    if ((threadIdx.x & 63u) == 0u && longest) atomicMax(&hdr->max_row, longest);
}

// Bitonic network over a[0 .. n), any n: every compare-exchange puts the larger value at the HIGHER index, so the positions from n
// up to the next power of two behave as +infinity that never moves and are simply skipped. (bitonic_any64 of f3dg_mesh_smooth.hip
// on 32-bit ids.)
__device__ void bitonic_any32(u32* a, u32 n)
{
    for (u64 k64 = 2; (k64 >> 1) < n; k64 <<= 1) {
        const u32 k = (u32)k64, half = (u32)(k64 >> 1);       // (k = 2^32 wraps to 0 only where blk is 0)
        for (u32 base = 0; base < n; base += MS_BIG_THREADS) {        // pair index i: block i / half, offset i % half
            const u32 i = base + threadIdx.x;
            const u32 blk = i / half, off = i % half;
            const u32 p = blk * k + off, q = blk * k + (k - 1u - off);
            if (q < n) { const u32 x = a[p], y = a[q]; if (x > y) { a[p] = y; a[q] = x; } }
        }
        __syncthreads();
        for (u32 j = half >> 1; j > 0u; j >>= 1) {
            for (u32 base = 0; base < n; base += MS_BIG_THREADS) {
                const u32 i = base + threadIdx.x;
                const u32 p = 2u * j * (i / j) + (i % j), q = p + j;
                if (q < n) { const u32 x = a[p], y = a[q]; if (x > y) { a[p] = y; a[q] = x; } }
            }
            __syncthreads();
        }
    }
}

__global__ void __launch_bounds__(MS_BIG_THREADS)
ms_sort_big_kernel(const u32* __restrict__ start, u32* members, const u32* __restrict__ big, u32 big_cap, const MsHeader* __restrict__ hdr)
{
    __shared__ u32 lds[MS_BIG_LDS];
    if (hdr->bad) return;
    const u32 n_big = hdr->n_big < big_cap ? hdr->n_big : big_cap;
    for (u32 b = blockIdx.x; b < n_big; b += gridDim.x) {
        const u32 v = big[b];
        const u32 s = start[v], n = start[v + 1] - s;
        u32* a = members + s;
        if (n <= MS_BIG_LDS) {
            for (u32 i = threadIdx.x; i < n; i += MS_BIG_THREADS) lds[i] = a[i];
            __syncthreads();
            bitonic_any32(lds, n);
            for (u32 i = threadIdx.x; i < n; i += MS_BIG_THREADS) a[i] = lds[i];
            __syncthreads();
        } else {
            __syncthreads();
            bitonic_any32(a, n);
        }
    }
}

// ------------------------------------------------------------------------------------------------ faces
template <typename I>
__global__ void __launch_bounds__(F3DG_BLOCK)
ms_face_insert_kernel(const I* __restrict__ faces, u32 F, u32 N, const u32* __restrict__ root, u32* ftab, u32 mask_f, MsHeader* __restrict__ hdr)
{
    if (hdr->bad) return;
    const u32 f = blockIdx.x * F3DG_BLOCK + threadIdx.x;
    int cls = MS_FACE_BAD;
    if (f < F) {
        Tri key{ 0u, 0u, 0u };
        cls = face_class(faces, f, N, root, key);
        if (cls == MS_FACE_LIVE) least_id_insert(ftab, mask_f, f, key, FaceKeyOf<I>{ faces, root, N });
    }
    wave_count(cls == MS_FACE_DEGENERATE, &hdr->degenerate);
    wave_count(cls == MS_FACE_COLLAPSED, &hdr->collapsed);
}

template <typename I>
__global__ void __launch_bounds__(F3DG_BLOCK)
ms_face_flag_kernel(const I* __restrict__ faces, u32 F, u32 N, const u32* __restrict__ root, const u32* __restrict__ ftab, u32 mask_f,
                    u64* __restrict__ flags_f, u64* flags_v, u32* __restrict__ blk_f, MsHeader* __restrict__ hdr)
{
    __shared__ u32 w_cnt[F3DG_BLOCK / 64];
    if (hdr->bad) return;                                   // (the whole workgroup)
    const u32 f = blockIdx.x * F3DG_BLOCK + threadIdx.x;
    bool keep = false, dup = false;
    if (f < F) {
        Tri key{ 0u, 0u, 0u };
        if (face_class(faces, f, N, root, key) == MS_FACE_LIVE) {
            keep = least_id_lookup(ftab, mask_f, key, FaceKeyOf<I>{ faces, root, N }) == f;
            dup = !keep;
            if (keep) {
                atomicOr(flags_v + (key.a >> 6), 1ull << (key.a & 63u));
                atomicOr(flags_v + (key.b >> 6), 1ull << (key.b & 63u));
                atomicOr(flags_v + (key.c >> 6), 1ull << (key.c & 63u));
            }
        }
    }
    wave_count(dup, &hdr->duplicate);
    block_flag_and_count(keep, f, F, flags_f, blk_f, w_cnt);
}

__global__ void __launch_bounds__(F3DG_BLOCK)
ms_vcount_kernel(const u64* __restrict__ flags_v, u32 nw_v, u32* __restrict__ blk_v, u32 nb_v, const MsHeader* __restrict__ hdr)
{
    if (hdr->bad) return;
    const u32 b = blockIdx.x * F3DG_BLOCK + threadIdx.x;
    if (b >= nb_v) return;
    u32 n = 0;
    for (u32 w = 4u * b; w < 4u * b + 4u && w < nw_v; w++) n += (u32)__popcll(flags_v[w]);
    blk_v[b] = n;
}

__global__ void __launch_bounds__(F3DG_BLOCK)
ms_finish_kernel(u32* __restrict__ blk_f, u32 ns_f, u32* __restrict__ blk_v, u32 ns_v, u32 N, u32 F, double cell, MsHeader* __restrict__ hdr)
{
    __shared__ u64 wtot[F3DG_BLOCK / 64];
    if (hdr->bad) return;                                   // (the whole workgroup)
    const u64 nf = compact_scan_counts(blk_f, ns_f, wtot);
    const u64 nv = compact_scan_counts(blk_v, ns_v, wtot);
    if (threadIdx.x == 0) {
        hdr->n_faces = nf;
        hdr->n_vertices = nv;
        hdr->N = N; hdr->F = F;
        hdr->cell = cell;
        hdr->ready = MS_READY;
    }
}

__device__ __forceinline__ bool ms_ready(const MsHeader* __restrict__ hdr, u32 N, u32 F)
{
    return hdr->ready == MS_READY && hdr->N == N && hdr->F == F;
}

// ------------------------------------------------------------------------------------------------ placement
__device__ __forceinline__ bool finite64(double x) { return fabs(x) <= 1.7976931348623157e308; }        // (a NaN fails)

template <int PLACEMENT, typename I>
__global__ void __launch_bounds__(F3DG_BLOCK)
ms_place_kernel(u32 N, u32 F, u64 n_rows, const float* __restrict__ vertices, const I* __restrict__ faces, u32 C, const float* __restrict__ attrs,
                const u32* __restrict__ root, const u32* __restrict__ start, const u32* __restrict__ members, const u64* __restrict__ flags_v,
                const u32* __restrict__ blk_v, const MsHeader* __restrict__ hdr, const AdjHeader* __restrict__ adj_hdr,
                const u32* __restrict__ adj_start, const u64* __restrict__ adj_rows, float* __restrict__ vertices_out, float* __restrict__ attrs_out,
                long long* __restrict__ vertex_map, long long* __restrict__ cluster_root, long long* __restrict__ cluster_size)
{
    if (!ms_ready(hdr, N, F)) return;                       // no completed count of this mesh on the workspace
    if (PLACEMENT == F3DG_SIMPLIFY_QUADRIC && !adj_ready(adj_hdr, N, F)) return;        // no completed adjacency build of it either
    const u32 v = blockIdx.x * F3DG_BLOCK + threadIdx.x;
    if (v >= N) return;
    const u32 r = root[v];
    const bool used = compact_kept(flags_v, r);
    const u64 row = used ? compact_rank(flags_v, blk_v, r) : 0ull;
    vertex_map[v] = used ? (long long)row : -1ll;
    if (r != v || !used || row >= n_rows) return;           // one thread per used cluster; the caller's arrays end at n_rows
    const u32 s = start[v], n = start[v + 1] - s;
    const double count = (double)n;
    cluster_root[row] = (long long)v;
    cluster_size[row] = (long long)n;
    for (u32 c = 0; c < C; c++) {                           // a walk per channel: no array of sums
        double sum = 0.0;
        for (u32 k = 0; k < n; k++) sum += (double)attrs[(size_t)members[s + k] * C + c];
        attrs_out[row * C + c] = (float)(sum / count);
    }
    float* out = vertices_out + 3 * row;
    if (PLACEMENT == F3DG_SIMPLIFY_ROOT) {
        out[0] = vertices[3 * (size_t)v]; out[1] = vertices[3 * (size_t)v + 1]; out[2] = vertices[3 * (size_t)v + 2];
        return;
    }
    double mx = 0.0, my = 0.0, mz = 0.0;
    for (u32 k = 0; k < n; k++) {                           // ascending in the member id: the row is sorted
        const float* p = vertices + 3 * (size_t)members[s + k];
        mx += (double)p[0]; my += (double)p[1]; mz += (double)p[2];
    }
    mx /= count; my /= count; mz /= count;
    if (PLACEMENT == F3DG_SIMPLIFY_MEAN) {
        out[0] = (float)mx; out[1] = (float)my; out[2] = (float)mz;
        return;
    }
    double axx = 0.0, axy = 0.0, axz = 0.0, ayy = 0.0, ayz = 0.0, azz = 0.0, gx = 0.0, gy = 0.0, gz = 0.0;
    for (u32 k = 0; k < n; k++) {
        const u32 m = members[s + k];
        const u32 as = adj_start[m], an = adj_start[m + 1] - as;
        for (u32 i = 0; i < an; i++) {
            const u64 e = adj_rows[as + i];
            if (!(e & 1ull)) continue;                      // succ == 1: every face of the member once, in row order
            const u32 f = (u32)(e & 0xFFFFFFFFull) >> 1;
            u32 id[3];
            if (f >= F || !load_face(faces, f, N, id)) continue;        // (not the faces the rows were built on)
            const float* q0 = vertices + 3 * (size_t)id[0];
            const float* q1 = vertices + 3 * (size_t)id[1];
            const float* q2 = vertices + 3 * (size_t)id[2];
            const double p0x = (double)q0[0], p0y = (double)q0[1], p0z = (double)q0[2];
            const double ux = (double)q1[0] - p0x, uy = (double)q1[1] - p0y, uz = (double)q1[2] - p0z;
            const double wx = (double)q2[0] - p0x, wy = (double)q2[1] - p0y, wz = (double)q2[2] - p0z;
            const double nx = uy * wz - uz * wy, ny = uz * wx - ux * wz, nz = ux * wy - uy * wx;
            const double res = (nx * (mx - p0x) + ny * (my - p0y)) + nz * (mz - p0z);
            axx += nx * nx; axy += nx * ny; axz += nx * nz; ayy += ny * ny; ayz += ny * nz; azz += nz * nz;
            gx += res * nx; gy += res * ny; gz += res * nz;
        }
    }
    const double tr = (axx + ayy) + azz;
    double dx = 0.0, dy = 0.0, dz = 0.0;
    if (tr > 0.0 && finite64(tr)) {
        const double mu = (0.001 * tr) / 3.0;
        const double a = axx + mu, d = ayy + mu, h = azz + mu, b = axy, c = axz, e = ayz;
        const double c00 = d * h - e * e, c01 = c * e - b * h, c02 = b * e - c * d;
        const double c11 = a * h - c * c, c12 = b * c - a * e, c22 = a * d - b * b;
        const double det = (a * c00 + b * c01) + c * c02;
        if (det > 0.0 && finite64(det)) {
            const double tx = -((c00 * gx + c01 * gy) + c02 * gz) / det;
            const double ty = -((c01 * gx + c11 * gy) + c12 * gz) / det;
            const double tz = -((c02 * gx + c12 * gy) + c22 * gz) / det;
            const double cell = hdr->cell;
            if (fabs(tx) <= cell && fabs(ty) <= cell && fabs(tz) <= cell) { dx = tx; dy = ty; dz = tz; }       // (a NaN or an infinity fails)
        }
    }
    out[0] = (float)(mx + dx); out[1] = (float)(my + dy); out[2] = (float)(mz + dz);
}

template <typename I>
__global__ void __launch_bounds__(F3DG_BLOCK)
ms_emit_faces_kernel(const I* __restrict__ faces, u32 F, u32 N, u64 n_rows, const u32* __restrict__ root, const u64* __restrict__ flags_f,
                     const u64* __restrict__ flags_v, const u32* __restrict__ blk_f, const u32* __restrict__ blk_v, const MsHeader* __restrict__ hdr,
                     const AdjHeader* __restrict__ adj_hdr, long long* __restrict__ faces_out)
{
    if (!ms_ready(hdr, N, F)) return;
    if (adj_hdr && !adj_ready(adj_hdr, N, F)) return;      // (quadric: the vertices are not written either, so nothing is)
    const u32 f = blockIdx.x * F3DG_BLOCK + threadIdx.x;
    if (f >= F || !compact_kept(flags_f, f)) return;
    const u64 row = compact_rank(flags_f, blk_f, f);
    if (row >= n_rows) return;                              // the caller's array ends here
    u32 v[3];
    if (!load_face(faces, f, N, v)) return;                 // (not the faces that were counted)
    long long* out = faces_out + 3 * row;
    // a used cluster's new id: the used roots below its own; the face keeps its own winding
    out[0] = (long long)compact_rank(flags_v, blk_v, root[v[0]]);
    out[1] = (long long)compact_rank(flags_v, blk_v, root[v[1]]);
    out[2] = (long long)compact_rank(flags_v, blk_v, root[v[2]]);
}

// ------------------------------------------------------------------------------------------------ host
template <typename I>
int simplify_count_impl(hipStream_t s, char* ws, const MsLayout& L, u32 N, u32 F, const float* vertices, const I* faces, const Grid& g,
                        long long* h_counts)
{
    MsHeader* hdr = reinterpret_cast<MsHeader*>(ws + L.header);
    u32* vtab = reinterpret_cast<u32*>(ws + L.vtab);
    u32* ftab = reinterpret_cast<u32*>(ws + L.ftab);
    u32* root = reinterpret_cast<u32*>(ws + L.root);
    u32* start = reinterpret_cast<u32*>(ws + L.start);
    u32* fill = reinterpret_cast<u32*>(ws + L.fill);
    u32* members = reinterpret_cast<u32*>(ws + L.members);
    u32* big = reinterpret_cast<u32*>(ws + L.big);
    u64* flags_f = reinterpret_cast<u64*>(ws + L.flags_f);
    u64* flags_v = reinterpret_cast<u64*>(ws + L.flags_v);
    u32* blk_f = reinterpret_cast<u32*>(ws + L.blk_f);
    u32* blk_v = reinterpret_cast<u32*>(ws + L.blk_v);
    const u32 mask_v = (u32)(L.cap_v - 1ull), mask_f = (u32)(L.cap_f - 1ull);
    const u32 nb_f = L.f.n_blocks, nb_v = L.v.n_blocks, nb_both = nb_f > nb_v ? nb_f : nb_v;
    F3DG_HIP_CHECK(hipMemsetAsync(hdr, 0, sizeof(MsHeader), s));
    F3DG_HIP_CHECK(hipMemsetAsync(vtab, 0xFF, (size_t)L.cap_v * 4, s));
    if (F) F3DG_HIP_CHECK(hipMemsetAsync(ftab, 0xFF, (size_t)L.cap_f * 4, s));
    F3DG_HIP_CHECK(hipMemsetAsync(start, 0, L.members - L.start, s));       // start and fill (their padding included)
    F3DG_HIP_CHECK(hipMemsetAsync(flags_v, 0, (size_t)L.v.n_words * 8, s));
    F3DG_HIP_CHECK(compact_clear_padding(s, blk_f, L.f));
    F3DG_HIP_CHECK(compact_clear_padding(s, blk_v, L.v));
    F3DG_KLAUNCH(ms_insert_kernel<I>, dim3(nb_both), dim3(F3DG_BLOCK), 0, s, vertices, N, faces, F, g, vtab, mask_v, hdr);
    F3DG_KLAUNCH(ms_root_kernel, dim3(nb_v), dim3(F3DG_BLOCK), 0, s, vertices, N, g, (const u32*)vtab, mask_v, root, start, hdr);
    F3DG_KLAUNCH(ms_scan_kernel, dim3(1), dim3(MS_BIG_THREADS), 0, s, start, L.n_scan, (const MsHeader*)hdr);
    F3DG_KLAUNCH(ms_scatter_kernel, dim3(nb_v), dim3(F3DG_BLOCK), 0, s, N, (const u32*)root, (const u32*)start, fill, members, (const MsHeader*)hdr);
    F3DG_KLAUNCH(ms_sort_small_kernel, dim3(nb_v), dim3(F3DG_BLOCK), 0, s, N, (const u32*)start, members, big, L.big_cap, hdr);
    const u32 big_grid = L.big_cap < 2048u ? L.big_cap : 2048u;
    F3DG_KLAUNCH(ms_sort_big_kernel, dim3(big_grid), dim3(MS_BIG_THREADS), 0, s, (const u32*)start, members, (const u32*)big, L.big_cap, (const MsHeader*)hdr);
    if (F) {
        F3DG_KLAUNCH(ms_face_insert_kernel<I>, dim3(nb_f), dim3(F3DG_BLOCK), 0, s, faces, F, N, (const u32*)root, ftab, mask_f, hdr);
        F3DG_KLAUNCH(ms_face_flag_kernel<I>, dim3(nb_f), dim3(F3DG_BLOCK), 0, s, faces, F, N, (const u32*)root, (const u32*)ftab, mask_f, flags_f, flags_v,
                     blk_f, hdr);
    }
    F3DG_KLAUNCH(ms_vcount_kernel, dim3((nb_v + F3DG_BLOCK - 1) / F3DG_BLOCK), dim3(F3DG_BLOCK), 0, s, (const u64*)flags_v, L.v.n_words, blk_v, nb_v,
                 (const MsHeader*)hdr);
    F3DG_KLAUNCH(ms_finish_kernel, dim3(1), dim3(F3DG_BLOCK), 0, s, blk_f, L.f.n_scan, blk_v, L.v.n_scan, N, F, g.cell, hdr);
    F3DG_HIP_CHECK(hipGetLastError());
    // the one host read: the counts and whether the mesh is refused
    MsHeader h;
    F3DG_HIP_CHECK(hipMemcpyAsync(&h, hdr, sizeof(MsHeader), hipMemcpyDeviceToHost, s));
    F3DG_HIP_CHECK(hipStreamSynchronize(s));
    if (h.bad) return F3DG_ERR_BAD_ARG;                     // nothing but the workspace was written
    h_counts[0] = (long long)h.clusters;
    h_counts[1] = (long long)h.n_vertices;
    h_counts[2] = (long long)h.degenerate;
    h_counts[3] = (long long)h.collapsed;
    h_counts[4] = (long long)h.duplicate;
    h_counts[5] = (long long)h.n_faces;
    h_counts[6] = (long long)h.max_row;
    h_counts[7] = 0;
    return F3DG_OK;
}

struct MsOutputs {
    float* vertices; long long* faces; float* attrs; long long* vertex_map; long long* cluster_root; long long* cluster_size;
};

template <int PLACEMENT, typename I>
int simplify_emit_impl(hipStream_t s, const char* ws, const MsLayout& L, u32 N, u32 F, const float* vertices, const I* faces, u32 C, const float* attrs,
                       const char* adj_ws, u64 n_vertices, u64 n_faces, const MsOutputs& o)
{
    const MsHeader* hdr = reinterpret_cast<const MsHeader*>(ws + L.header);
    const u32* root = reinterpret_cast<const u32*>(ws + L.root);
    const u32* start = reinterpret_cast<const u32*>(ws + L.start);
    const u32* members = reinterpret_cast<const u32*>(ws + L.members);
    const u64* flags_f = reinterpret_cast<const u64*>(ws + L.flags_f);
    const u64* flags_v = reinterpret_cast<const u64*>(ws + L.flags_v);
    const u32* blk_f = reinterpret_cast<const u32*>(ws + L.blk_f);
    const u32* blk_v = reinterpret_cast<const u32*>(ws + L.blk_v);
    const AdjHeader* adj_hdr = nullptr;
    const u32* adj_start = nullptr;
    const u64* adj_rows = nullptr;
    if (PLACEMENT == F3DG_SIMPLIFY_QUADRIC) {
        const AdjLayout A = adj_layout(N, F);
        adj_hdr = reinterpret_cast<const AdjHeader*>(adj_ws + A.header);
        adj_start = reinterpret_cast<const u32*>(adj_ws + A.start);
        adj_rows = reinterpret_cast<const u64*>(adj_ws + A.rows);
    }
    F3DG_KLAUNCH((ms_place_kernel<PLACEMENT, I>), dim3(L.v.n_blocks), dim3(F3DG_BLOCK), 0, s, N, F, n_vertices, vertices, faces, C, attrs, root, start,
                 members, flags_v, blk_v, hdr, adj_hdr, adj_start, adj_rows, o.vertices, o.attrs, o.vertex_map, o.cluster_root, o.cluster_size);
    F3DG_KLAUNCH(ms_emit_faces_kernel<I>, dim3(L.f.n_blocks), dim3(F3DG_BLOCK), 0, s, faces, F, N, n_faces, root, flags_f, flags_v, blk_f, blk_v, hdr,
                 adj_hdr, o.faces);
    F3DG_HIP_CHECK(hipGetLastError());
    return F3DG_OK;
}

template <typename I>
int simplify_emit_any(int placement, hipStream_t s, const char* ws, const MsLayout& L, u32 N, u32 F, const float* vertices, const I* faces, u32 C,
                      const float* attrs, const char* adj_ws, u64 n_vertices, u64 n_faces, const MsOutputs& o)
{
    switch (placement) {
    case F3DG_SIMPLIFY_ROOT: return simplify_emit_impl<F3DG_SIMPLIFY_ROOT>(s, ws, L, N, F, vertices, faces, C, attrs, adj_ws, n_vertices, n_faces, o);
    case F3DG_SIMPLIFY_MEAN: return simplify_emit_impl<F3DG_SIMPLIFY_MEAN>(s, ws, L, N, F, vertices, faces, C, attrs, adj_ws, n_vertices, n_faces, o);
    default: return simplify_emit_impl<F3DG_SIMPLIFY_QUADRIC>(s, ws, L, N, F, vertices, faces, C, attrs, adj_ws, n_vertices, n_faces, o);
    }
}

bool finite_host(double x) { return x == x && x - x == 0.0; }

} // namespace

extern "C" size_t f3dg_mesh_simplify_workspace_bytes(long long N, long long F)
{
    if (ms_check_sizes(N, F) != F3DG_OK) return 0;
    return ms_layout((u32)N, (u32)F).total;
}

extern "C" int f3dg_mesh_simplify_count(void* stream, void* workspace, size_t workspace_bytes, long long N, long long F, const float* vertices,
                                        const void* faces, int faces_int32, const double* origin, double cell, long long* h_counts)
{
    if (!workspace || !vertices || !origin || !h_counts || (!faces && F > 0) || ((uintptr_t)workspace & 15u)) return F3DG_ERR_BAD_ARG;
    if (!(cell > 0.0) || !finite_host(cell) || !finite_host(origin[0]) || !finite_host(origin[1]) || !finite_host(origin[2])) return F3DG_ERR_BAD_ARG;
    const int rc = ms_check_sizes(N, F);
    if (rc != F3DG_OK) return rc;
    const MsLayout L = ms_layout((u32)N, (u32)F);
    if (workspace_bytes < L.total) return F3DG_ERR_WORKSPACE;
    const Grid g{ origin[0], origin[1], origin[2], cell };
    hipStream_t s = (hipStream_t)stream;
    return faces_int32 ? simplify_count_impl(s, (char*)workspace, L, (u32)N, (u32)F, vertices, (const int*)faces, g, h_counts)
                       : simplify_count_impl(s, (char*)workspace, L, (u32)N, (u32)F, vertices, (const long long*)faces, g, h_counts);
}

extern "C" int f3dg_mesh_simplify_emit(void* stream, void* workspace, size_t workspace_bytes, long long N, long long F, const float* vertices,
                                       const void* faces, int faces_int32, int placement, int C, const float* attrs, const void* adjacency_workspace,
                                       size_t adjacency_workspace_bytes, long long n_vertices_out, long long n_faces_out, float* vertices_out,
                                       long long* faces_out, float* attrs_out, long long* vertex_map, long long* cluster_root, long long* cluster_size)
{
    if (!workspace || !vertices || !faces || !vertices_out || !faces_out || !vertex_map || !cluster_root || !cluster_size) return F3DG_ERR_BAD_ARG;
    if (n_vertices_out <= 0 || n_faces_out <= 0 || C < 0 || C > F3DG_SIMPLIFY_MAX_ATTRS || (C > 0 && (!attrs || !attrs_out))) return F3DG_ERR_BAD_ARG;
    if (placement != F3DG_SIMPLIFY_ROOT && placement != F3DG_SIMPLIFY_MEAN && placement != F3DG_SIMPLIFY_QUADRIC) return F3DG_ERR_BAD_ARG;
    if (placement == F3DG_SIMPLIFY_QUADRIC && (!adjacency_workspace || ((uintptr_t)adjacency_workspace & 15u))) return F3DG_ERR_BAD_ARG;
    if (((uintptr_t)workspace & 15u) || ((uintptr_t)faces_out & 7u) || ((uintptr_t)vertex_map & 7u) || ((uintptr_t)cluster_root & 7u) ||
        ((uintptr_t)cluster_size & 7u)) return F3DG_ERR_BAD_ARG;
    // no output is another output, an input or a workspace
    const void* outs[6] = { vertices_out, faces_out, C > 0 ? attrs_out : nullptr, vertex_map, cluster_root, cluster_size };
    const void* ins[5] = { workspace, vertices, faces, C > 0 ? attrs : nullptr, placement == F3DG_SIMPLIFY_QUADRIC ? adjacency_workspace : nullptr };
    for (int i = 0; i < 6; i++) {
        if (!outs[i]) continue;
        for (int j = 0; j < i; j++) if (outs[j] == outs[i]) return F3DG_ERR_BAD_ARG;
        for (int j = 0; j < 5; j++) if (ins[j] == outs[i]) return F3DG_ERR_BAD_ARG;
    }
    const int rc = ms_check_sizes(N, F);
    if (rc != F3DG_OK) return rc;
    if (F == 0) return F3DG_ERR_BAD_ARG;                    // nothing survives a mesh without faces: there is nothing to write
    if (placement == F3DG_SIMPLIFY_QUADRIC) {
        const int ra = adj_check_sizes(N, F);
        if (ra != F3DG_OK) return ra;
    }
    const MsLayout L = ms_layout((u32)N, (u32)F);
    if (workspace_bytes < L.total) return F3DG_ERR_WORKSPACE;
    if (placement == F3DG_SIMPLIFY_QUADRIC && adjacency_workspace_bytes < adj_layout((u32)N, (u32)F).total) return F3DG_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    const MsOutputs o{ vertices_out, faces_out, attrs_out, vertex_map, cluster_root, cluster_size };
    return faces_int32 ? simplify_emit_any(placement, s, (const char*)workspace, L, (u32)N, (u32)F, vertices, (const int*)faces, (u32)C, attrs,
                                           (const char*)adjacency_workspace, (u64)n_vertices_out, (u64)n_faces_out, o)
                       : simplify_emit_any(placement, s, (const char*)workspace, L, (u32)N, (u32)F, vertices, (const long long*)faces, (u32)C, attrs,
                                           (const char*)adjacency_workspace, (u64)n_vertices_out, (u64)n_faces_out, o);
}
