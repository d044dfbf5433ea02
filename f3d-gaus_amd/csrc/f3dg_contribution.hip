// f3dg_contribution.hip -- which Gaussians matter: per-Gaussian contribution statistics of the views of a call, and the compaction of a
// Gaussian set by them.
//
// STATISTICS. contribution_kernel follows a forward on the same workspace and walks every pixel's tile list again, front to back from
// T = 1, in the REFERENCE's arithmetic whatever the forward ran in (f3dg_pair_eval<false, false, false>, this file is built with
// -ffp-contract=off). A (pixel, entry) pair is
//   skipped   the pixel is done, or t <= 0.2, or alpha < 1/255: counts nowhere;
//   a stopper not skipped and T (1 - alpha) < 0.0001f: the pixel is done, stops[g] += 1 (forward.cu:543-547: the entry that ends a pixel's
//             walk is itself not blended -- take it away and the pixel blends on, so "never blended" is not "no effect");
//   blended   otherwise: w = alpha T is the float32 number the exact forward adds to its alpha channel; blended[g] += 1,
//             max_weight[g] = max(., w), sum_weight[g] += w, T = T (1 - alpha).
// Every statistic is a function of the SET of pairs: the counters are integers, the maximum of non-negative floats is the unsigned
// maximum of their bit patterns, and the sum is kept in fixed point -- every pair adds round(w 2^32) (half to even; w < 1) to a u64.
// So every output is bit-reproducible, run to run and path to path.
// LIMITS: one record takes the pairs of fewer than 2^31 pixels (views x W x H summed over the calls that add into it): each counter
// then fits its 32 bits and the sum stays below 2^63. The callers check it (f3dg_contribution per call, contribution.py over calls).
//
// The record, 32 bytes per Gaussian, ADDED INTO (the caller clears it once):
//   u64 sum_fixed;  u64 blended | stops << 32;  u32 max_bits;  u32 pad[3]
//
// Schedule: one wave64 per (view, tile, 8x8 quadrant), the front end of the compositing forwards (F3dgHalfWindow, f3dg_quad.h: scan,
// global_load_lds staging, phase 1). Phase 2 is this kernel's own: every pixel walks its pass mask through the three-way decision and
// adds what it finds to its slot's accumulators in LDS (ds atomics: integer adds and a maximum); when a half of the window retires,
// lane e flushes slot e with one u64 add for the sum, one u64 add for both counters and one u32 max (issued only when the slot's maximum
// exceeds what the record already holds) -- once per staged entry that reached a pixel, not once per pair, and nothing for the entries
// that reached none.
//
// COMPACTION (f3dg_compact.h): gc_count_kernel (keep bits, flag words, workgroup counts), gc_scan_kernel (one workgroup), one host
// read of the kept count, gc_emit_kernel (kept ids ascending, up to F3DG_COMPACT_MAX_ARRAYS row arrays gathered in input order).
#include "f3dg_blend.h"
#include "f3dg_compact.h"
#include "f3dg_quad.h"

#include <string.h>
#include <vector>

namespace {

struct __attribute__((aligned(32))) ContribRec {
    u64 sum_fixed;
    u64 counts;             // blended | stops << 32
    u32 max_bits;
    u32 pad[3];
};
static_assert(sizeof(ContribRec) == F3DG_CONTRIBUTION_BYTES, "the record of include/f3dg.h");

#define CONTRIB_STOP (1u << 16)     // a slot's LDS counter: blended in the low half, stops in the high one (at most 64 pairs each)

template <bool FINAL_T>
__global__ void __launch_bounds__(64, 4)
contribution_kernel(int V, int P, int W, int H, int tiles_x, int T, float focal_x, float focal_y,
                    const F3dgHeader* __restrict__ hdr, const uint2* __restrict__ ranges,
                    const unsigned* __restrict__ point_list_general, const unsigned* __restrict__ small_list,
                    const F3dgRec* __restrict__ rec, const float4* __restrict__ cull, ContribRec* __restrict__ stats, float* __restrict__ final_T)
{
    const F3dgQuad qd = f3dg_quad(V, T, tiles_x);
    const unsigned lane = threadIdx.x & 63u;
    const F3dgQuadPixel px = f3dg_quad_pixel(qd, lane, W, H, focal_x, focal_y);

    __shared__ float4 sR[4][64];                  // records, [16-byte chunk][slot]
    __shared__ unsigned sQ[F3DG_QUAD_RING];       // ids of kept entries not staged yet (they stay readable for the slide that staged them)
    __shared__ unsigned sId[64];                  // Gaussian of every staged slot
    __shared__ u64 sSum[64];                      // per slot: fixed-point sum of w,
    __shared__ unsigned sCnt[64], sMax[64];       // ... blended | stops << 16, maximum of the bits of w

    sSum[lane] = 0ull; sCnt[lane] = 0u; sMax[lane] = 0u; sId[lane] = 0u;
    f3dg_wave_fence();

    // the lists of the forward that left this workspace: the general path's, or the per-tile slots of the small-call path
    const unsigned* point_list = hdr->small_path != 0u ? small_list : point_list_general;

    // slots of physical half `half` (2: both): lane e flushes slot e
    auto flush = [&](unsigned half) {
        f3dg_wave_fence();
        const unsigned c = sCnt[lane];
        if ((half == 2u || (lane >> 5) == half) && c != 0u) {
            const unsigned id = sId[lane];
            if (id < (unsigned)P) {
                ContribRec* r = stats + id;
                const unsigned nb = c & (CONTRIB_STOP - 1u), ns = c >> 16;
                if (nb != 0u) {
                    atomicAdd(&r->sum_fixed, sSum[lane]);
                    // the maximum only grows, so whatever a plain load returns -- even a stale line -- is a value the record has held: a
                    // slot that does not exceed it cannot change the record. Most do not: one atomic in three gone, 19.4 -> 16.5 ms over the
                    // real set's orbit
                    if (sMax[lane] > __atomic_load_n(&r->max_bits, __ATOMIC_RELAXED)) atomicMax(&r->max_bits, sMax[lane]);
                }
                atomicAdd(&r->counts, (u64)nb | ((u64)ns << 32));
            }
            sSum[lane] = 0ull; sCnt[lane] = 0u; sMax[lane] = 0u;
        }
        f3dg_wave_fence();
    };

    bool done = !px.inside;
    float Tr = 1.0f;
    F3dgHalfWindow<false> win(sR, sQ, nullptr, nullptr, qd, lane, P, T, hdr, ranges, point_list, rec, cull);
    unsigned long long& pass = win.pass;
    if (__ballot(!done) != 0ull)
    for (;;) {
        flush(win.flip);                          // the older half retires
        if (!win.slide(done))
            break;
        // the Gaussians of the entries the slide staged into the retired half: still in the ring, behind its head
        if (lane < win.m) sId[(win.flip ^ 1u) * 32u + lane] = sQ[(win.qhead - win.m + lane) & (F3DG_QUAD_RING - 1)];
        f3dg_wave_fence();
        const unsigned xr = win.xr;

        // ---- phase 2: as render3s_fwd_kernel's -- until every live pixel has finished the older half
        while (pass != 0ull && __ballot((unsigned)pass != 0u) != 0ull) {
            const unsigned j = (unsigned)__builtin_ctzll(pass) ^ xr;
            pass &= pass - 1;
            const float4 q0 = sR[0][j], q1 = sR[1][j], q2 = sR[2][j];
            const F3dgPair pr = f3dg_pair_eval<false, false, false>(px.ray_x, px.ray_y, q0, q1, q2);
            if (pr.live) {
                const float alpha = pr.alpha;
                const float test_T = Tr * (1 - alpha);
                if (test_T < 0.0001f) {
                    atomicAdd(&sCnt[j], CONTRIB_STOP);
                    done = true;
                    pass = 0ull;
                } else {
                    const float w = alpha * Tr;
                    atomicAdd(&sCnt[j], 1u);
                    atomicMax(&sMax[j], __float_as_uint(w));
                    atomicAdd(&sSum[j], (u64)__double2ull_rn((double)w * 4294967296.0));
                    Tr = test_T;
                }
            }
        }
        if (__ballot(!done) == 0ull)
            break;
    }
    flush(2u);
    if (FINAL_T && px.inside) final_T[(size_t)qd.view * ((size_t)H * W) + px.id] = Tr;
}

// ------------------------------------------------------------------------------------------------ compaction of a Gaussian set
struct GcHeader {                   // first 256 bytes of the compaction workspace
    u64 n_kept;
    u32 P;
    u32 ready;                      // GC_READY once the counts are scanned: f3dg_gaussian_compact_emit may read them
    u32 pad[60];
};
#define GC_READY 0x47435259u

struct GcLayout {
    CompactPlan p;
    size_t header, flags, counts, total;
};

GcLayout gc_layout(u32 P)
{
    GcLayout L;
    L.p = compact_plan(P);
    L.header = 0;
    L.flags = f3dg_align256(sizeof(GcHeader));
    L.counts = L.flags + L.p.flag_bytes;
    L.total = L.counts + L.p.count_bytes;
    return L;
}

// P in [0, the id range of a list entry]
int gc_check_size(long long P) { return P < 0 ? F3DG_ERR_BAD_ARG : P > (long long)F3DG_ID_MASK ? F3DG_ERR_UNSUPPORTED : F3DG_OK; }

__global__ void __launch_bounds__(F3DG_BLOCK)
gc_count_kernel(u32 P, const ContribRec* __restrict__ stats, const unsigned char* __restrict__ keep, u64 min_touched, float min_max_weight,
                double min_sum_weight, u64* __restrict__ flags, u32* __restrict__ counts)
{
    __shared__ u32 w_cnt[F3DG_BLOCK / 64];
    const u32 i = blockIdx.x * F3DG_BLOCK + threadIdx.x;
    bool k = i < P;
    if (k && stats != nullptr) {
        const ContribRec r = stats[i];
        const u64 touched = (r.counts & 0xFFFFFFFFull) + (r.counts >> 32);
        // sum_weight as the Python side states it: the fixed-point sum as a float64, over 2^32
        k = touched >= min_touched && __uint_as_float(r.max_bits) >= min_max_weight && (double)r.sum_fixed * (1.0 / 4294967296.0) >= min_sum_weight;
    }
    if (k && keep != nullptr) k = keep[i] != 0;
    block_flag_and_count(k, i, P, flags, counts, w_cnt);
}

__global__ void __launch_bounds__(F3DG_BLOCK)
gc_scan_kernel(u32* __restrict__ counts, u32 n_scan, u32 P, GcHeader* __restrict__ hdr)
{
    __shared__ u64 wtot[F3DG_BLOCK / 64];
    const u64 n = compact_scan_counts(counts, n_scan, wtot);
    if (threadIdx.x == 0) {
        hdr->n_kept = n;
        hdr->P = P;
        hdr->ready = GC_READY;
    }
}

struct GcArrays {
    int n;
    const float* src[F3DG_COMPACT_MAX_ARRAYS];
    float* dst[F3DG_COMPACT_MAX_ARRAYS];
    int row_floats[F3DG_COMPACT_MAX_ARRAYS];
};

__global__ void __launch_bounds__(F3DG_BLOCK)
gc_emit_kernel(u32 P, u64 n_rows, const u64* __restrict__ flags, const u32* __restrict__ counts, const GcHeader* __restrict__ hdr, GcArrays a,
               int* __restrict__ kept_ids)
{
    if (hdr->ready != GC_READY || hdr->P != P) return;      // no completed count of this set on the workspace
    const u32 i = blockIdx.x * F3DG_BLOCK + threadIdx.x;
    if (i >= P || !compact_kept(flags, i)) return;
    const u64 row = compact_rank(flags, counts, i);
    if (row >= n_rows) return;                              // the caller's arrays end here
    kept_ids[row] = (int)i;
    for (int k = 0; k < a.n; k++) {
        const size_t rf = (size_t)a.row_floats[k];
        const float* s = a.src[k] + (size_t)i * rf;
        float* d = a.dst[k] + row * rf;
        for (size_t c = 0; c < rf; c++) d[c] = s[c];
    }
}

} // namespace

extern "C" int f3dg_contribution(void* stream, const void* workspace, size_t workspace_bytes, long long max_rendered, int n_views, int P, int W,
                                 int H, float tan_fovx, float tan_fovy, void* stats, float* final_T)
{
    if (!workspace || n_views <= 0 || P < 0 || W <= 0 || H <= 0 || max_rendered < 0) return F3DG_ERR_BAD_ARG;
    if (max_rendered > 0xFFFFFFF0ll || (long long)n_views * P > 0xFFFFFFF0ll || P > (int)F3DG_ID_MASK) return F3DG_ERR_BAD_ARG;
    if ((long long)n_views * W * H >= (1ll << 31)) return F3DG_ERR_BAD_ARG;        // the record's limit (above)
    if (P > 0 && (!stats || ((uintptr_t)stats & 31u))) return F3DG_ERR_BAD_ARG;
    const F3dgLayout L = f3dg_layout(P, W, H, n_views, max_rendered);
    if (workspace_bytes < L.total) return F3DG_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    const char* ws = static_cast<const char*>(workspace);
    // BLOCKING, 256 bytes: whose lists these are. The ids the kernel adds at come from them, so the shape must be the forward's
    F3dgHeader h;
    F3DG_HIP_CHECK(hipMemcpyAsync(&h, ws + L.header, sizeof h, hipMemcpyDeviceToHost, s));
    F3DG_HIP_CHECK(hipStreamSynchronize(s));
    if (h.n_sets > 1u) return F3DG_ERR_BAD_ARG;            // statistics per set are not served
    if (P == 0) {
        // a forward without Gaussians left no lists: every pixel's walk ends where it began
        if (final_T) {
            std::vector<float> ones((size_t)n_views * W * H, 1.0f);
            F3DG_HIP_CHECK(hipMemcpyAsync(final_T, ones.data(), ones.size() * sizeof(float), hipMemcpyHostToDevice, s));
            F3DG_HIP_CHECK(hipStreamSynchronize(s));
        }
        return F3DG_OK;
    }
    if (h.small_shape[0] != (unsigned)P || h.small_shape[1] != (unsigned)n_views || h.small_shape[2] != (unsigned)W || h.small_shape[3] != (unsigned)H ||
        h.capacity != (unsigned)max_rendered)
        return F3DG_ERR_STATE;
    const int tiles_x = (W + F3DG_TILE - 1) / F3DG_TILE, tiles_y = (H + F3DG_TILE - 1) / F3DG_TILE;
    const int T = tiles_x * tiles_y;
    const float focal_y = H / (2.0f * tan_fovy);
    const float focal_x = W / (2.0f * tan_fovx);
    const dim3 grid((unsigned)n_views * (unsigned)T * 4u);
#define CONTRIB_ARGS n_views, P, W, H, tiles_x, T, focal_x, focal_y, reinterpret_cast<const F3dgHeader*>(ws + L.header),                          \
        reinterpret_cast<const uint2*>(ws + L.ranges), reinterpret_cast<const unsigned*>(ws + L.vals[0]),                                         \
        reinterpret_cast<const unsigned*>(ws + L.small_list), reinterpret_cast<const F3dgRec*>(ws + L.rec),                                       \
        reinterpret_cast<const float4*>(ws + L.cull), static_cast<ContribRec*>(stats), final_T
    if (final_T) F3DG_KLAUNCH(contribution_kernel<true>, grid, dim3(64), 0, s, CONTRIB_ARGS);
    else F3DG_KLAUNCH(contribution_kernel<false>, grid, dim3(64), 0, s, CONTRIB_ARGS);
#undef CONTRIB_ARGS
    F3DG_HIP_CHECK(hipGetLastError());
    return F3DG_OK;
}

extern "C" size_t f3dg_gaussian_compact_workspace_bytes(long long P)
{
    if (gc_check_size(P) != F3DG_OK) return 0;
    return gc_layout((u32)P).total;
}

extern "C" int f3dg_gaussian_compact_count(void* stream, void* workspace, size_t workspace_bytes, long long P, const void* stats,
                                           const unsigned char* keep, long long min_touched, float min_max_weight, double min_sum_weight,
                                           long long* h_kept)
{
    if (!workspace || !h_kept || (!stats && !keep) || ((uintptr_t)workspace & 15u) || ((uintptr_t)stats & 31u)) return F3DG_ERR_BAD_ARG;
    if (min_touched < 0 || !(min_max_weight == min_max_weight) || !(min_sum_weight == min_sum_weight)) return F3DG_ERR_BAD_ARG;
    const int rc = gc_check_size(P);
    if (rc != F3DG_OK) return rc;
    const GcLayout L = gc_layout((u32)P);
    if (workspace_bytes < L.total) return F3DG_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    char* ws = static_cast<char*>(workspace);
    GcHeader* hdr = reinterpret_cast<GcHeader*>(ws + L.header);
    F3DG_HIP_CHECK(hipMemsetAsync(hdr, 0, sizeof(GcHeader), s));
    if (P == 0) {                                           // nothing is kept; the header says that no count is there to emit from
        F3DG_HIP_CHECK(hipStreamSynchronize(s));
        *h_kept = 0;
        return F3DG_OK;
    }
    u64* flags = reinterpret_cast<u64*>(ws + L.flags);
    u32* counts = reinterpret_cast<u32*>(ws + L.counts);
    F3DG_HIP_CHECK(compact_clear_padding(s, counts, L.p));
    F3DG_KLAUNCH(gc_count_kernel, dim3(L.p.n_blocks), dim3(F3DG_BLOCK), 0, s, (u32)P, static_cast<const ContribRec*>(stats), keep, (u64)min_touched,
                 min_max_weight, min_sum_weight, flags, counts);
    F3DG_KLAUNCH(gc_scan_kernel, dim3(1), dim3(F3DG_BLOCK), 0, s, counts, L.p.n_scan, (u32)P, hdr);
    F3DG_HIP_CHECK(hipGetLastError());
    GcHeader h;                                             // the one host read: the kept count
    F3DG_HIP_CHECK(hipMemcpyAsync(&h, hdr, sizeof(GcHeader), hipMemcpyDeviceToHost, s));
    F3DG_HIP_CHECK(hipStreamSynchronize(s));
    *h_kept = (long long)h.n_kept;
    return F3DG_OK;
}

extern "C" int f3dg_gaussian_compact_emit(void* stream, const void* workspace, size_t workspace_bytes, long long P, long long n_kept, int n_arrays,
                                          const void* const* srcs, void* const* dsts, const int* row_floats, int* kept_ids)
{
    if (!workspace || !kept_ids || n_kept <= 0 || n_arrays < 0 || n_arrays > F3DG_COMPACT_MAX_ARRAYS) return F3DG_ERR_BAD_ARG;
    if (n_arrays > 0 && (!srcs || !dsts || !row_floats)) return F3DG_ERR_BAD_ARG;
    if (((uintptr_t)workspace & 15u) || ((uintptr_t)kept_ids & 3u)) return F3DG_ERR_BAD_ARG;
    GcArrays a;
    memset(&a, 0, sizeof a);
    a.n = n_arrays;
    for (int k = 0; k < n_arrays; k++) {
        if (!srcs[k] || !dsts[k] || row_floats[k] <= 0 || ((uintptr_t)srcs[k] & 3u) || ((uintptr_t)dsts[k] & 3u)) return F3DG_ERR_BAD_ARG;
        a.src[k] = static_cast<const float*>(srcs[k]);
        a.dst[k] = static_cast<float*>(dsts[k]);
        a.row_floats[k] = row_floats[k];
    }
    const int rc = gc_check_size(P);
    if (rc != F3DG_OK) return rc;
    if (P == 0 || n_kept > P) return F3DG_ERR_BAD_ARG;      // nothing was counted / more rows than elements
    const GcLayout L = gc_layout((u32)P);
    if (workspace_bytes < L.total) return F3DG_ERR_WORKSPACE;
    const char* ws = static_cast<const char*>(workspace);
    F3DG_KLAUNCH(gc_emit_kernel, dim3(L.p.n_blocks), dim3(F3DG_BLOCK), 0, (hipStream_t)stream, (u32)P, (u64)n_kept,
                 reinterpret_cast<const u64*>(ws + L.flags), reinterpret_cast<const u32*>(ws + L.counts), reinterpret_cast<const GcHeader*>(ws + L.header), a,
                 kept_ids);
    F3DG_HIP_CHECK(hipGetLastError());
    return F3DG_OK;
}
