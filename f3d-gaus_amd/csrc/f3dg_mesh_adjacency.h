// f3dg_mesh_adjacency.h -- the workspace of f3dg_mesh_adjacency as its readers see it: the header, the layout, the stamp that says the
// sorted incidence rows of a mesh of (N, F) are there, and the checked face load. f3dg_mesh_smooth.hip builds the rows and reads them for
// the normals; f3dg_mesh_simplify.hip reads them for the quadric placement.
#pragma once
#include "f3dg_common.h"
#include "f3dg_compact.h"

namespace {

#define ADJ_SMALL 32u               // longest row one thread sorts
#define ADJ_BIG_THREADS 1024
#define ADJ_BIG_LDS 4096u           // entries of a row that is sorted in LDS (32 KB of u64)
#define ADJ_SCAN_WAVES (ADJ_BIG_THREADS / 64)
#define ADJ_SCAN_ITEMS 16
#define ADJ_READY 0x61646A79u

struct AdjHeader {                  // first 256 bytes of the workspace
    u32 bad;                        // 1: a face holds an id outside [0, N)
    u32 degenerate;                 // faces with two equal ids
    u32 n_big;                      // rows queued for adj_sort_big_kernel
    u32 n_boundary;                 // vertices with a boundary edge
    u32 max_row;                    // entries of the longest row
    u32 ready;                      // ADJ_READY once the rows are sorted and the degrees scanned: the normals may read them
    u32 N, F;                       // the mesh they were built on
    u64 entries;                    // incidence entries, 6 per non-degenerate face
    u64 two_e;                      // sum of the degrees
    u32 reserved[52];
};
static_assert(sizeof(AdjHeader) == 256, "the header is the first 256 bytes");

struct AdjLayout {
    size_t header, start, fill, big, rows, total;
    u32 n_scan, big_cap;            // entries of start / fill (N + 1 rounded up to whole scan items), capacity of the queue
};

AdjLayout adj_layout(u32 N, u32 F)
{
    AdjLayout L;
    L.n_scan = (u32)(((u64)N + 1 + ADJ_SCAN_ITEMS - 1) / ADJ_SCAN_ITEMS * ADJ_SCAN_ITEMS);
    const u64 cap = 6ull * F / (ADJ_SMALL + 1u) + 1ull;      // a queued row holds more than ADJ_SMALL of the 6 F entries
    L.big_cap = (u32)(cap < (u64)N ? cap : (u64)N);
    L.header = 0;
    L.start = f3dg_align256(sizeof(AdjHeader));
    L.fill = L.start + f3dg_align256((size_t)L.n_scan * 4);          // directly behind start: one memset clears both
    L.big = L.fill + f3dg_align256((size_t)L.n_scan * 4);
    L.rows = L.big + f3dg_align256((size_t)L.big_cap * 4);
    L.total = L.rows + f3dg_align256((size_t)F * 48);
    return L;
}

// F3DG_OK, or why the sizes are refused
int adj_check_sizes(long long N, long long F)
{
    if (N <= 0 || F < 0) return F3DG_ERR_BAD_ARG;
    if (N >= (1ll << 31) || F >= (1ll << 31) || 6 * F >= (1ll << 31)) return F3DG_ERR_UNSUPPORTED;
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

__device__ __forceinline__ bool adj_ready(const AdjHeader* __restrict__ hdr, u32 N, u32 F)
{
    return hdr->ready == ADJ_READY && hdr->N == N && hdr->F == F;
}

} // namespace
