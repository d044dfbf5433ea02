// f3dg_mesh_clean.hip -- what follows either mesh route: the connected components of a triangle mesh (vertex connectivity) and the
// compaction that keeps the chosen ones. Integers only, no float arithmetic; every output is a function of the input alone. The
// semantics are this project's, stated in include/f3dg.h and DESIGN.md section 3g-ter; tests/mesh_clean_truth.py restates them.
//
// Components: a union-find forest over the vertices, parent[v] <= v AT ALL TIMES, so every walk and every retry below follows a strictly
// decreasing vertex id and ends. No thread waits for another thread's write: no spin, no ticket, no barrier between workgroups. Inside a
// kernel every access to `parent` is a device-scope atomic (atomicCAS / atomicMin, relaxed agent-scope loads): the L2s of the XCDs are
// not coherent for plain accesses within one launch. Correctness does not rest on those reads being fresh: a stale parent is an older
// ancestor (links are only ever replaced by links to an ancestor), and a separate verification launch decides whether a round converged.
//   cc_init_kernel       parent[v] = v
//   cc_hook_kernel       one thread per face: the range check of its ids BEFORE anything is indexed with them, then two unions. A union
//                        hooks ROOTS only, the greater under the lesser, by compare-and-swap; a failed swap returns the root's new
//                        parent (a smaller id) and the union goes on from there, so no link is ever lost. The walks halve their path
//                        (atomicMin of the grandparent, an ancestor): chains stay short on meshes whose ids run against the hooks.
//   cc_compress_kernel   one thread per vertex: parent[v] = its root
//   cc_verify_kernel     one thread per face: counts the faces whose three corners do not all point at one self-parented root. If all
//                        do, that root is the least vertex id of the component: it is a vertex of the component (links join only vertices
//                        that faces join), it is <= everything that points at it, and faces that share a vertex share it.
//   cc_label_kernel      one thread per face: its label, and the per-root face counts. A closed surface is ONE address, so equal labels
//                        are combined within the wave first (a ballot loop over the distinct labels, one atomicAdd of the popcount each).
//   cc_stats_kernel      a fixed grid over the vertices: the number of roots that own faces and the largest count, one atomic per workgroup
// Compaction (f3dg_compact.h), of the kept faces and of the vertices they use:
//   mc_flag_kernel       one thread per face: the face's flag and the workgroup's count (block_flag_and_count), and one bit per used vertex
//                        (atomicOr: order-free)
//   mc_vcount_kernel     one thread per 256 vertices: their count (the vertex bits come from atomics, not from a ballot)
//   mc_scan_kernel       one workgroup: compact_scan_counts over both count arrays, totals and `ready` into the header
//   mc_emit_faces_kernel / mc_emit_vertices_kernel   one thread per face / vertex at its compact_rank; a vertex's new id is its rank among
//                        the used bits. Rows of 24 bytes at data-dependent offsets and single 8-byte ids: no 16-byte store fits either
//                        layout; the count arrays are scanned in uint4s.
#include "f3dg_common.h"
#include "f3dg_compact.h"

namespace {

#define MC_MAX_ROUNDS 32
#define MC_READY 0x6D636C6Eu
#define MC_STATS_BLOCKS 1024u

struct CcHeader {                   // first 256 bytes of the components workspace; the first 8 bytes are a round's host read
    u32 mismatch;                   // faces whose corners did not share a root in the last verification
    u32 bad;                        // 1: a face holds an id outside [0, N)
    u32 n_components, largest, degenerate;
    u32 reserved[59];
};

struct McHeader {                   // first 256 bytes of the compaction workspace
    u64 n_faces, n_vertices;
    u32 bad;                        // 1: a kept face holds an id outside [0, N)
    u32 ready;                      // MC_READY once the counts are scanned: f3dg_mesh_compact_emit may read them
    u32 N, F;                       // the mesh they were counted on
    u32 reserved[56];
};

struct McLayout {
    size_t header, flags_f, flags_v, blk_f, blk_v, total;
    CompactPlan f, v;                               // of the faces / vertices
};

McLayout mc_layout(u32 N, u32 F)
{
    McLayout L;
    L.f = compact_plan(F);
    L.v = compact_plan(N);
    L.header = 0;
    L.flags_f = f3dg_align256(sizeof(McHeader));
    L.flags_v = L.flags_f + L.f.flag_bytes;
    L.blk_f = L.flags_v + L.v.flag_bytes;
    L.blk_v = L.blk_f + L.f.count_bytes;
    L.total = L.blk_v + L.v.count_bytes;
    return L;
}

size_t cc_total(u32 N) { return f3dg_align256(sizeof(CcHeader)) + f3dg_align256((size_t)N * 4); }

// F3DG_OK, or why the sizes are refused
int mc_check_sizes(long long N, long long F)
{
    if (N <= 0 || F < 0) return F3DG_ERR_BAD_ARG;
    if (N >= (1ll << 31) || F >= (1ll << 31)) return F3DG_ERR_UNSUPPORTED;
    return F3DG_OK;
}

// the three ids of face f; false when one lies outside [0, N) (nothing may be indexed with them then)
template <typename I>
__device__ __forceinline__ bool load_face(const I* __restrict__ faces, u32 f, u32 N, u32 v[3])
{
    bool ok = true;
#pragma unroll
    for (int i = 0; i < 3; i++) {
        const long long id = (long long)faces[3 * (size_t)f + i];
        ok = ok && id >= 0 && id < (long long)N;
        v[i] = (u32)id;
    }
    return ok;
}

__device__ __forceinline__ bool degenerate(const u32 v[3]) { return v[0] == v[1] || v[1] == v[2] || v[0] == v[2]; }

__device__ __forceinline__ u32 parent_load(const u32* parent, u32 x)
{
    return __hip_atomic_load(parent + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// the root of x. x strictly decreases from step to step (parent[x] <= x), so the walk ends after at most x steps. On the way every
// vertex passed is re-pointed at its grandparent: an ancestor, so no link is lost, and a smaller id, so parent[v] <= v stays.
__device__ __forceinline__ u32 find_root(u32* parent, u32 x)
{
    u32 p = parent_load(parent, x);
    while (p < x) {
        const u32 g = parent_load(parent, p);
        if (g < p) atomicMin(parent + x, g);
        x = p;
        p = g;
    }
    return x;
}

// join the trees of a and b. Only a ROOT is ever hooked, by compare-and-swap from its own id, the greater root under the lesser. A swap
// that fails returns what another thread hooked that root under -- a smaller id --, and the union goes on from there: every repeat
// strictly lowers the greater of the two ids, so the loop ends, and it never waits for anybody.
__device__ __forceinline__ void unite(u32* parent, u32 a, u32 b)
{
    for (;;) {
        a = find_root(parent, a);
        b = find_root(parent, b);
        if (a == b) return;
        if (a < b) { const u32 t = a; a = b; b = t; }
        const u32 old = atomicCAS(parent + a, a, b);
        if (old >= a) return;       // == a: hooked. (> a cannot be, parent[a] <= a; it would end the union all the same)
        a = old;                    // < the a that was tried
    }
}

__global__ void __launch_bounds__(F3DG_BLOCK)
cc_init_kernel(u32* __restrict__ parent, u32 N)
{
    const u32 v = blockIdx.x * F3DG_BLOCK + threadIdx.x;
    if (v < N) parent[v] = v;
}

template <typename I>
__global__ void __launch_bounds__(F3DG_BLOCK)
cc_hook_kernel(const I* __restrict__ faces, u32 F, u32 N, u32* parent, CcHeader* __restrict__ hdr)
{
    const u32 f = blockIdx.x * F3DG_BLOCK + threadIdx.x;
    if (f >= F) return;
    u32 v[3];
    if (!load_face(faces, f, N, v)) {
        atomicOr(&hdr->bad, 1u);
        return;
    }
    if (degenerate(v)) return;
    unite(parent, v[0], v[1]);
    unite(parent, v[0], v[2]);
}

__global__ void __launch_bounds__(F3DG_BLOCK)
cc_compress_kernel(u32* parent, u32 N)
{
    const u32 v = blockIdx.x * F3DG_BLOCK + threadIdx.x;
    if (v >= N) return;
    const u32 r = find_root(parent, v);
    if (r < v) atomicMin(parent + v, r);
}

template <typename I>
__global__ void __launch_bounds__(F3DG_BLOCK)
cc_verify_kernel(const I* __restrict__ faces, u32 F, u32 N, const u32* parent, CcHeader* __restrict__ hdr)
{
    const u32 f = blockIdx.x * F3DG_BLOCK + threadIdx.x;
    bool wrong = false;
    if (f < F) {
        u32 v[3];
        if (load_face(faces, f, N, v) && !degenerate(v)) {
            const u32 r = parent_load(parent, v[0]);
            wrong = parent_load(parent, v[1]) != r || parent_load(parent, v[2]) != r || parent_load(parent, r) != r;
        }
    }
    const u64 m = __ballot(wrong);
    if ((threadIdx.x & 63u) == 0u && m) atomicAdd(&hdr->mismatch, (u32)__popcll(m));
}

template <typename I>
__global__ void __launch_bounds__(F3DG_BLOCK)
cc_label_kernel(const I* __restrict__ faces, u32 F, u32 N, const u32* __restrict__ parent, int* __restrict__ face_component,
                u32* __restrict__ component_faces, CcHeader* __restrict__ hdr)
{
    const u32 f = blockIdx.x * F3DG_BLOCK + threadIdx.x;
    const u32 lane = threadIdx.x & 63u;
    u32 label = 0xFFFFFFFFu;                                // no component: a degenerate face, or no face at all
    if (f < F) {
        u32 v[3];
        if (load_face(faces, f, N, v) && !degenerate(v)) label = parent[v[0]];          // (every id was in range in the rounds before)
        face_component[f] = (int)label;
    }
    const bool live = label != 0xFFFFFFFFu;
    const u64 dead = __ballot(f < F && !live);
    if (lane == 0u && dead) atomicAdd(&hdr->degenerate, (u32)__popcll(dead));
    // one atomic per distinct label of the wave: every pass retires the first remaining lane's label (at most 64 passes, wave-uniform)
    u64 todo = __ballot(live);
    while (todo) {
        const int leader = __ffsll((long long)todo) - 1;
        const u32 l = (u32)__shfl((int)label, leader, 64);
        const u64 same = __ballot(live && label == l);
        if (lane == (u32)leader) atomicAdd(&component_faces[l], (u32)__popcll(same));
        todo &= ~same;
    }
}

__global__ void __launch_bounds__(F3DG_BLOCK)
cc_stats_kernel(const u32* __restrict__ component_faces, u32 N, CcHeader* __restrict__ hdr)
{
    __shared__ u32 w_n[F3DG_BLOCK / 64], w_max[F3DG_BLOCK / 64];
    u32 n = 0, big = 0;
    for (u64 v = (u64)blockIdx.x * F3DG_BLOCK + threadIdx.x; v < (u64)N; v += (u64)gridDim.x * F3DG_BLOCK) {
        const u32 c = component_faces[v];
        n += c ? 1u : 0u;
        big = c > big ? c : big;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        n += __shfl_down(n, off, 64);
        const u32 o = __shfl_down(big, off, 64);
        big = o > big ? o : big;
    }
    if ((threadIdx.x & 63u) == 0u) { w_n[threadIdx.x >> 6] = n; w_max[threadIdx.x >> 6] = big; }
    __syncthreads();
    if (threadIdx.x == 0) {
        u32 tn = 0, tm = 0;
#pragma unroll
        for (int w = 0; w < F3DG_BLOCK / 64; w++) { tn += w_n[w]; tm = w_max[w] > tm ? w_max[w] : tm; }
        if (tn) { atomicAdd(&hdr->n_components, tn); atomicMax(&hdr->largest, tm); }
    }
}

// ------------------------------------------------------------------------------------------------ compaction
template <typename I>
__global__ void __launch_bounds__(F3DG_BLOCK)
mc_flag_kernel(const I* __restrict__ faces, u32 F, u32 N, const int* __restrict__ face_component, const unsigned char* __restrict__ keep_root,
               u64* __restrict__ flags_f, u64* flags_v, u32* __restrict__ blk_f, McHeader* __restrict__ hdr)
{
    __shared__ u32 w_cnt[F3DG_BLOCK / 64];
    const u32 f = blockIdx.x * F3DG_BLOCK + threadIdx.x;
    bool keep = false;
    if (f < F) {
        const int c = face_component[f];
        if (c >= 0 && (u32)c < N && keep_root[c] != 0) {
            u32 v[3];
            if (!load_face(faces, f, N, v)) {
                atomicOr(&hdr->bad, 1u);
            } else if (!degenerate(v)) {
                keep = true;
#pragma unroll
                for (int i = 0; i < 3; i++) atomicOr(flags_v + (v[i] >> 6), 1ull << (v[i] & 63u));
            }
        }
    }
    block_flag_and_count(keep, f, F, flags_f, blk_f, w_cnt);
}

__global__ void __launch_bounds__(F3DG_BLOCK)
mc_vcount_kernel(const u64* __restrict__ flags_v, u32 nw_v, u32* __restrict__ blk_v, u32 nb_v)
{
    const u32 b = blockIdx.x * F3DG_BLOCK + threadIdx.x;
    if (b >= nb_v) return;
    u32 n = 0;
    for (u32 w = 4u * b; w < 4u * b + 4u && w < nw_v; w++) n += (u32)__popcll(flags_v[w]);
    blk_v[b] = n;
}

__global__ void __launch_bounds__(F3DG_BLOCK)
mc_scan_kernel(u32* __restrict__ blk_f, u32 ns_f, u32* __restrict__ blk_v, u32 ns_v, u32 N, u32 F, McHeader* __restrict__ hdr)
{
    __shared__ u64 wtot[F3DG_BLOCK / 64];
    const u64 nf = compact_scan_counts(blk_f, ns_f, wtot);
    const u64 nv = compact_scan_counts(blk_v, ns_v, wtot);
    if (threadIdx.x == 0) {
        hdr->n_faces = nf;
        hdr->n_vertices = nv;
        hdr->N = N; hdr->F = F;
        hdr->ready = hdr->bad ? 0u : MC_READY;
    }
}

__device__ __forceinline__ bool mc_ready(const McHeader* __restrict__ hdr, u32 N, u32 F)
{
    return hdr->ready == MC_READY && hdr->N == N && hdr->F == F;
}

template <typename I>
__global__ void __launch_bounds__(F3DG_BLOCK)
mc_emit_faces_kernel(const I* __restrict__ faces, u32 F, u32 N, u64 n_rows, const u64* __restrict__ flags_f, const u64* __restrict__ flags_v,
                     const u32* __restrict__ blk_f, const u32* __restrict__ blk_v, const McHeader* __restrict__ hdr, long long* __restrict__ faces_out)
{
    if (!mc_ready(hdr, N, F)) return;                       // no completed count of this mesh on the workspace
    const u32 f = blockIdx.x * F3DG_BLOCK + threadIdx.x;
    if (f >= F || !compact_kept(flags_f, f)) return;
    const u64 row = compact_rank(flags_f, blk_f, f);
    if (row >= n_rows) return;                              // the caller's array ends here
    u32 v[3];
    if (!load_face(faces, f, N, v)) return;                 // (not the faces that were counted)
    long long* out = faces_out + 3 * row;
    // a used vertex's new id: the used vertices below it
    out[0] = (long long)compact_rank(flags_v, blk_v, v[0]);
    out[1] = (long long)compact_rank(flags_v, blk_v, v[1]);
    out[2] = (long long)compact_rank(flags_v, blk_v, v[2]);
}

__global__ void __launch_bounds__(F3DG_BLOCK)
mc_emit_vertices_kernel(u32 N, u32 F, u64 n_rows, const u64* __restrict__ flags_v, const u32* __restrict__ blk_v,
                        const McHeader* __restrict__ hdr, long long* __restrict__ vertex_ids)
{
    if (!mc_ready(hdr, N, F)) return;
    const u32 v = blockIdx.x * F3DG_BLOCK + threadIdx.x;
    if (v >= N || !compact_kept(flags_v, v)) return;
    const u64 row = compact_rank(flags_v, blk_v, v);
    if (row < n_rows) vertex_ids[row] = (long long)v;
}

template <typename I>
int components_impl(hipStream_t s, char* ws, u32 N, u32 F, const I* faces, int* face_component, int* component_faces, long long* h_counts)
{
    CcHeader* hdr = reinterpret_cast<CcHeader*>(ws);
    u32* parent = reinterpret_cast<u32*>(ws + f3dg_align256(sizeof(CcHeader)));
    const u32 nb_f = (F + F3DG_BLOCK - 1) / F3DG_BLOCK, nb_v = (N + F3DG_BLOCK - 1) / F3DG_BLOCK;
    F3DG_HIP_CHECK(hipMemsetAsync(hdr, 0, sizeof(CcHeader), s));
    F3DG_KLAUNCH(cc_init_kernel, dim3(nb_v), dim3(F3DG_BLOCK), 0, s, parent, N);
    u32 state[2] = { 1u, 0u };                              // mismatch, bad
    int rounds = 0;
    while (state[0] != 0u && rounds < MC_MAX_ROUNDS) {
        rounds++;
        if (rounds > 1) F3DG_HIP_CHECK(hipMemsetAsync(&hdr->mismatch, 0, 4, s));
        F3DG_KLAUNCH(cc_hook_kernel<I>, dim3(nb_f), dim3(F3DG_BLOCK), 0, s, faces, F, N, parent, hdr);
        F3DG_KLAUNCH(cc_compress_kernel, dim3(nb_v), dim3(F3DG_BLOCK), 0, s, parent, N);
        F3DG_KLAUNCH(cc_verify_kernel<I>, dim3(nb_f), dim3(F3DG_BLOCK), 0, s, faces, F, N, (const u32*)parent, hdr);
        F3DG_HIP_CHECK(hipGetLastError());
        // the round's one host read, 8 bytes: the faces that do not agree on a root yet, and whether an id was out of range
        F3DG_HIP_CHECK(hipMemcpyAsync(state, hdr, 8, hipMemcpyDeviceToHost, s));
        F3DG_HIP_CHECK(hipStreamSynchronize(s));
        if (state[1]) return F3DG_ERR_BAD_ARG;              // nothing but the workspace was written
    }
    if (state[0] != 0u) return F3DG_ERR_UNSUPPORTED;        // the cap: a round with a live hook at least halves the trees, N < 2^31
    F3DG_HIP_CHECK(hipMemsetAsync(component_faces, 0, (size_t)N * 4, s));
    F3DG_KLAUNCH(cc_label_kernel<I>, dim3(nb_f), dim3(F3DG_BLOCK), 0, s, faces, F, N, (const u32*)parent, face_component,
                 (u32*)component_faces, hdr);
    F3DG_KLAUNCH(cc_stats_kernel, dim3(nb_v < MC_STATS_BLOCKS ? nb_v : MC_STATS_BLOCKS), dim3(F3DG_BLOCK), 0, s, (const u32*)component_faces, N, hdr);
    F3DG_HIP_CHECK(hipGetLastError());
    CcHeader h;
    F3DG_HIP_CHECK(hipMemcpyAsync(&h, hdr, sizeof(CcHeader), hipMemcpyDeviceToHost, s));
    F3DG_HIP_CHECK(hipStreamSynchronize(s));
    h_counts[0] = (long long)h.n_components;
    h_counts[1] = (long long)h.largest;
    h_counts[2] = (long long)h.degenerate;
    h_counts[3] = (long long)rounds;
    return F3DG_OK;
}

template <typename I>
int compact_count_impl(hipStream_t s, char* ws, const McLayout& L, u32 N, u32 F, const I* faces, const int* face_component,
                       const unsigned char* keep_root, long long* h_counts)
{
    McHeader* hdr = reinterpret_cast<McHeader*>(ws + L.header);
    u64* flags_f = reinterpret_cast<u64*>(ws + L.flags_f);
    u64* flags_v = reinterpret_cast<u64*>(ws + L.flags_v);
    u32* blk_f = reinterpret_cast<u32*>(ws + L.blk_f);
    u32* blk_v = reinterpret_cast<u32*>(ws + L.blk_v);
    F3DG_HIP_CHECK(hipMemsetAsync(hdr, 0, sizeof(McHeader), s));
    F3DG_HIP_CHECK(hipMemsetAsync(flags_v, 0, (size_t)L.v.n_words * 8, s));
    F3DG_HIP_CHECK(compact_clear_padding(s, blk_f, L.f));
    F3DG_HIP_CHECK(compact_clear_padding(s, blk_v, L.v));
    F3DG_KLAUNCH(mc_flag_kernel<I>, dim3(L.f.n_blocks), dim3(F3DG_BLOCK), 0, s, faces, F, N, face_component, keep_root, flags_f, flags_v, blk_f, hdr);
    F3DG_KLAUNCH(mc_vcount_kernel, dim3((L.v.n_blocks + F3DG_BLOCK - 1) / F3DG_BLOCK), dim3(F3DG_BLOCK), 0, s, (const u64*)flags_v, L.v.n_words, blk_v,
                 L.v.n_blocks);
    F3DG_KLAUNCH(mc_scan_kernel, dim3(1), dim3(F3DG_BLOCK), 0, s, blk_f, L.f.n_scan, blk_v, L.v.n_scan, N, F, hdr);
    F3DG_HIP_CHECK(hipGetLastError());
    // the one host read: the two counts and whether an id was out of range
    McHeader h;
    F3DG_HIP_CHECK(hipMemcpyAsync(&h, hdr, sizeof(McHeader), hipMemcpyDeviceToHost, s));
    F3DG_HIP_CHECK(hipStreamSynchronize(s));
    if (h.bad) return F3DG_ERR_BAD_ARG;
    h_counts[0] = (long long)h.n_faces;
    h_counts[1] = (long long)h.n_vertices;
    return F3DG_OK;
}

template <typename I>
int compact_emit_impl(hipStream_t s, char* ws, const McLayout& L, u32 N, u32 F, const I* faces, u64 n_faces, u64 n_vertices, long long* faces_out,
                      long long* vertex_ids)
{
    const McHeader* hdr = reinterpret_cast<const McHeader*>(ws + L.header);
    const u64* flags_f = reinterpret_cast<const u64*>(ws + L.flags_f);
    const u64* flags_v = reinterpret_cast<const u64*>(ws + L.flags_v);
    const u32* blk_f = reinterpret_cast<const u32*>(ws + L.blk_f);
    const u32* blk_v = reinterpret_cast<const u32*>(ws + L.blk_v);
    F3DG_KLAUNCH(mc_emit_faces_kernel<I>, dim3(L.f.n_blocks), dim3(F3DG_BLOCK), 0, s, faces, F, N, n_faces, flags_f, flags_v, blk_f, blk_v, hdr, faces_out);
    F3DG_KLAUNCH(mc_emit_vertices_kernel, dim3(L.v.n_blocks), dim3(F3DG_BLOCK), 0, s, N, F, n_vertices, flags_v, blk_v, hdr, vertex_ids);
    F3DG_HIP_CHECK(hipGetLastError());
    return F3DG_OK;
}

} // namespace

extern "C" size_t f3dg_mesh_components_workspace_bytes(long long N, long long F)
{
    if (mc_check_sizes(N, F) != F3DG_OK) return 0;
    return cc_total((u32)N);
}

extern "C" int f3dg_mesh_components(void* stream, void* workspace, size_t workspace_bytes, long long N, long long F, const void* faces,
                                    int faces_int32, int* face_component, int* component_faces, long long* h_counts)
{
    if (!workspace || !component_faces || !h_counts || ((!faces || !face_component) && F > 0) || ((uintptr_t)workspace & 15u)) return F3DG_ERR_BAD_ARG;
    const int rc = mc_check_sizes(N, F);
    if (rc != F3DG_OK) return rc;
    if (workspace_bytes < cc_total((u32)N)) return F3DG_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    if (F == 0) {
        F3DG_HIP_CHECK(hipMemsetAsync(component_faces, 0, (size_t)N * 4, s));
        F3DG_HIP_CHECK(hipStreamSynchronize(s));
        h_counts[0] = h_counts[1] = h_counts[2] = h_counts[3] = 0;
        return F3DG_OK;
    }
    return faces_int32 ? components_impl(s, (char*)workspace, (u32)N, (u32)F, (const int*)faces, face_component, component_faces, h_counts)
                       : components_impl(s, (char*)workspace, (u32)N, (u32)F, (const long long*)faces, face_component, component_faces, h_counts);
}

extern "C" size_t f3dg_mesh_compact_workspace_bytes(long long N, long long F)
{
    if (mc_check_sizes(N, F) != F3DG_OK) return 0;
    return mc_layout((u32)N, (u32)F).total;
}

extern "C" int f3dg_mesh_compact_count(void* stream, void* workspace, size_t workspace_bytes, long long N, long long F, const void* faces,
                                       int faces_int32, const int* face_component, const unsigned char* keep_root, long long* h_counts)
{
    if (!workspace || !keep_root || !h_counts || ((!faces || !face_component) && F > 0) || ((uintptr_t)workspace & 15u)) return F3DG_ERR_BAD_ARG;
    const int rc = mc_check_sizes(N, F);
    if (rc != F3DG_OK) return rc;
    const McLayout L = mc_layout((u32)N, (u32)F);
    if (workspace_bytes < L.total) return F3DG_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    if (F == 0) {                                           // nothing is kept; the header says that no count is there to emit from
        F3DG_HIP_CHECK(hipMemsetAsync(workspace, 0, sizeof(McHeader), s));
        F3DG_HIP_CHECK(hipStreamSynchronize(s));
        h_counts[0] = h_counts[1] = 0;
        return F3DG_OK;
    }
    return faces_int32 ? compact_count_impl(s, (char*)workspace, L, (u32)N, (u32)F, (const int*)faces, face_component, keep_root, h_counts)
                       : compact_count_impl(s, (char*)workspace, L, (u32)N, (u32)F, (const long long*)faces, face_component, keep_root, h_counts);
}

extern "C" int f3dg_mesh_compact_emit(void* stream, void* workspace, size_t workspace_bytes, long long N, long long F, const void* faces,
                                      int faces_int32, const int* face_component, const unsigned char* keep_root, long long n_faces_kept,
                                      long long n_vertices_kept, long long* faces_out, long long* vertex_ids)
{
    if (!workspace || !faces || !face_component || !keep_root || !faces_out || !vertex_ids || n_faces_kept <= 0 || n_vertices_kept <= 0) return F3DG_ERR_BAD_ARG;
    if (((uintptr_t)workspace & 15u) || ((uintptr_t)faces_out & 7u) || ((uintptr_t)vertex_ids & 7u)) return F3DG_ERR_BAD_ARG;
    const int rc = mc_check_sizes(N, F);
    if (rc != F3DG_OK) return rc;
    if (F == 0) return F3DG_ERR_BAD_ARG;                    // nothing was counted: there is nothing to write
    const McLayout L = mc_layout((u32)N, (u32)F);
    if (workspace_bytes < L.total) return F3DG_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    return faces_int32 ? compact_emit_impl(s, (char*)workspace, L, (u32)N, (u32)F, (const int*)faces, (u64)n_faces_kept, (u64)n_vertices_kept, faces_out, vertex_ids)
                       : compact_emit_impl(s, (char*)workspace, L, (u32)N, (u32)F, (const long long*)faces, (u64)n_faces_kept, (u64)n_vertices_kept, faces_out, vertex_ids);
}
