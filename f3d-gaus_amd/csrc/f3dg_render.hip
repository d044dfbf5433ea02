// f3dg_render.hip -- per-tile front-to-back GOF compositing (the roofline kernel of the path).
//
// Replaces renderCUDA<3> (reference RAST/cuda_rasterizer/forward.cu:409-612): for every pixel of a 16x16 tile, walk the tile's
// depth-sorted Gaussian list, intersect the pixel ray with each Gaussian's quadric (view2gaussian: Sigma', B, C), turn the minimum
// of the quadric along the ray into an alpha, and blend RGB, view-space normal, median depth, alpha and the 2DGS-style distortion
// term front to back. All views of a call are ONE launch; an XCD-aware id -> (view, tile) map keeps a view's records in one L2.
//
// The blend is a strict per-pixel recurrence whose float32 / float64 operation order is the reference's (the file is built with
// -ffp-contract=off): the exponent -(1/2)(C - B^2/4A) cancels 1e5..1e6 x and any re-association moves isolated pixels by 1e-2
// (SURVEY 0.9). There is no inter-pixel arithmetic, hence no MFMA.
//
// Two kernels, and two copies of that arithmetic ON PURPOSE:
//   render3s_fwd_kernel (the default of the general path): one wave64 per 8x8 pixel quadrant, no workgroup barriers, sliding
//       half-windows of staged records. See the comment above the kernel. Its blend arithmetic, in the reference's order and in the
//       fast inference mode, its fused trip and its write-out are those of f3dg_blend.h, shared with the multi-wave kernels of
//       f3dg_render4.hip / f3dg_render5.hip. These kernels only ever REMOVE (pixel, Gaussian) pairs that are a bare `continue` in the
//       reference (alpha < 1/255 proven by a conservative test), so their images are bit-identical within an arithmetic mode.
//   render_fwd_kernel (option reference_kernels): the plain transcription -- every pixel visits every entry of its tile's list in the
//       reference's arithmetic. It is the baseline every other compositing kernel is compared with bit for bit
//       (tests/test_raster_forward_gpu.py::test_pretest_is_conservative_bit_identical_outputs), so it shares NOTHING with them: its
//       pixel state, its blend_entry and its write-out stand next to it, written straight from the reference, and it uses neither
//       f3dg_blend.h nor f3dg_quad.h. A slip in the shared arithmetic therefore shows as a difference between two independent texts.
// t = -BB/(2*AA) is a double quotient of float-valued operands rounded to float: identical to ONE IEEE float32 divide (double
// rounding is innocuous for p = 24, q = 53 >= 2p + 2), so the float64 divide is not needed.
#include "f3dg_blend.h"
#include "f3dg_common.h"
#include "f3dg_ellipse.h"
#include "f3dg_quad.h"

#include <stdarg.h>
#include <stdio.h>
#include <string.h>

namespace {

// ---- the plain transcription (option reference_kernels): one workgroup per tile, one pixel per lane, every pixel visits every entry of
// the tile's list in the reference's arithmetic (blend_entry). Nothing is filtered: the baseline of the bit-identity tests. PixelState,
// blend_entry and the write-out at the kernel's end are its own (see the file header).
struct PixelState {
    float Tr;
    unsigned last_contributor, max_contributor;
    float C0, C1, C2, C3, C4, C5, C6, C7;
    float dist1, dist2, distortion;
};

// The reference's per-(pixel, Gaussian) arithmetic after the geometric terms (forward.cu:511-579), in its operation
// order. Returns true when the pixel saturates (`done = true`); `contributor` is the 1-based position in the tile list.
__device__ __forceinline__ bool blend_entry(PixelState& st, unsigned contributor, float n0, float n1, float n2, float aaf,
                                            float bhalf, float CC, float opac, float cr, float cg, float cb)
{
    const double AA = aaf;
    const float bbf = 2 * bhalf;
    const double BB = bbf;

    // ONE float64 division serves both uses: -BB / (2 * AA) is the correctly rounded quotient BB / AA scaled by -1/2
    // (exact), so t below has the bits of the reference's (float)(-BB / (2 * AA)).
    const double q = BB / AA;
    const float t = (float)(-0.5 * q);
    if (t <= F3DG_NEAR_PLANE)
        return false;

    const double min_value = -q * (BB / 4.) + CC;
    float power = (float)(-0.5f * min_value);
    if (power > 0.0f)
        power = 0.0f;

    const float alpha = fminf(0.99f, opac * expf(power));
    if (alpha < 1.0f / 255.0f)
        return false;
    const float Tr = st.Tr;
    const float test_T = Tr * (1 - alpha);
    if (test_T < 0.0001f)
        return true;

    {
        const float mapped_max_t = (float)((F3DG_FAR_PLANE * t - F3DG_FAR_PLANE * F3DG_NEAR_PLANE) / ((F3DG_FAR_PLANE - F3DG_NEAR_PLANE) * t));
        const float A = 1 - Tr;
        const float error = mapped_max_t * mapped_max_t * A + st.dist2 - 2 * mapped_max_t * st.dist1;
        st.distortion += error * alpha * Tr;
        st.dist1 += mapped_max_t * alpha * Tr;
        st.dist2 += mapped_max_t * mapped_max_t * alpha * Tr;
    }

    st.C0 += cr * alpha * Tr;
    st.C1 += cg * alpha * Tr;
    st.C2 += cb * alpha * Tr;
    {
        const float length = (float)sqrt(n0 * n0 + n1 * n1 + n2 * n2 + 1e-7);
        const float nn0 = -n0 / length, nn1 = -n1 / length, nn2 = -n2 / length;
        st.C3 += nn0 * alpha * Tr;
        st.C4 += nn1 * alpha * Tr;
        st.C5 += nn2 * alpha * Tr;
    }
    if (Tr > 0.5) {
        st.C6 = t;
        st.max_contributor = contributor;
    }
    st.C7 += alpha * Tr;

    st.Tr = test_T;
    st.last_contributor = contributor;
    return false;
}

#define F3DG_ROUND (F3DG_BLOCK - 1)     // list entries staged per round; LDS slot F3DG_ROUND holds the vote counters

template <bool SAVE_AUX>
__global__ void __launch_bounds__(F3DG_BLOCK, 8)
render_fwd_kernel(int V, int P, int W, int H, int tiles_x, int T, float focal_x, float focal_y,
                  const F3dgHeader* __restrict__ hdr, const uint2* __restrict__ ranges,
                  const unsigned* __restrict__ point_list, const F3dgRec* __restrict__ rec,
                  const float* __restrict__ background, int bg_per_view,
                  float* __restrict__ out_color, float* __restrict__ final_T, unsigned* __restrict__ n_contrib)
{
    unsigned view, tile;
    f3dg_xcd_map(blockIdx.x, (unsigned)V, (unsigned)T, view, tile);

    const unsigned tile_x = tile % (unsigned)tiles_x, tile_y = tile / (unsigned)tiles_x;
    // each wave owns an 8x8 pixel quadrant of the tile and each of its four 16-lane groups a 4x4 block of it
    const unsigned lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const unsigned grp = lane >> 4, gi = lane & 15u;
    const unsigned blk_x = (wave & 1u) * 2u + (grp & 1u), blk_y = (wave >> 1) * 2u + (grp >> 1);    // 4x4 block in tile
    const unsigned lx = blk_x * 4u + (gi & 3u), ly = blk_y * 4u + (gi >> 2);
    const unsigned pix_x = tile_x * F3DG_TILE + lx, pix_y = tile_y * F3DG_TILE + ly;
    const bool inside = pix_x < (unsigned)W && pix_y < (unsigned)H;
    const size_t HW = (size_t)H * W;
    const size_t pix_id = (size_t)W * pix_y + pix_x;
    const float pixf_x = (float)pix_x + 0.5f, pixf_y = (float)pix_y + 0.5f;
    const float ray_x = (float)((pixf_x - W / 2.) / focal_x);
    const float ray_y = (float)((pixf_y - H / 2.) / focal_y);

    uint2 range = ranges[(size_t)view * T + tile];
    if (hdr->overflow) range = make_uint2(0, 0);
    const int rounds = (int)((range.y - range.x + F3DG_ROUND - 1) / F3DG_ROUND);
    int toDo = (int)(range.y - range.x);

    // 255 staged records, structure-of-arrays by float4
    __shared__ float4 sq0[F3DG_BLOCK];            // v0 v1 v2 v3
    __shared__ float4 sq1[F3DG_BLOCK];            // v4 v5 v6 v7
    __shared__ float4 sq2[F3DG_BLOCK];            // v8 v9 opac K
    __shared__ float4 sq3[F3DG_BLOCK];            // r g b depth
    // block-wide count of finished pixels, double buffered by round parity, in the never-staged slot F3DG_ROUND
    int* done_cnt = reinterpret_cast<int*>(&sq3[F3DG_ROUND]);
    if (threadIdx.x == 0) { done_cnt[0] = 0; done_cnt[1] = 0; }
    __syncthreads();

    const F3dgRec* vrec = rec + (size_t)view * P;

    bool done = !inside;
    PixelState st;
    st.Tr = 1.0f;
    st.last_contributor = 0; st.max_contributor = (unsigned)-1;
    st.C0 = st.C1 = st.C2 = st.C3 = st.C4 = st.C5 = st.C6 = st.C7 = 0;
    st.dist1 = st.dist2 = st.distortion = 0;

    for (int i = 0; i < rounds; i++, toDo -= F3DG_ROUND) {
        {
            const unsigned long long dl = __ballot(done);
            if (lane == 0)
                atomicAdd(&done_cnt[i & 1], __popcll(dl));
        }
        __syncthreads();
        const int num_done = done_cnt[i & 1];
        if (threadIdx.x == 0)
            done_cnt[(i + 1) & 1] = 0;          // everyone has read it (round i - 1); next added to after the barrier below
        if (num_done == F3DG_BLOCK)
            break;

        const unsigned progress = (unsigned)i * F3DG_ROUND + threadIdx.x;
        if (threadIdx.x < F3DG_ROUND && range.x + progress < range.y) {
            const unsigned id = point_list[range.x + progress] & F3DG_ID_MASK;
            const float4* src = reinterpret_cast<const float4*>(vrec + id);
            sq0[threadIdx.x] = src[0];
            sq1[threadIdx.x] = src[1];
            sq2[threadIdx.x] = src[2];
            sq3[threadIdx.x] = src[3];
        }
        __syncthreads();

        const int count = min(F3DG_ROUND, toDo);
        const unsigned round_base = (unsigned)i * F3DG_ROUND;
        for (int j = 0; !done && j < count; j++) {
            const float4 q0 = sq0[j], q1 = sq1[j], q2 = sq2[j], q3 = sq3[j];
            const float n0 = q0.x * ray_x + q0.y * ray_y + q0.z;
            const float n1 = q0.y * ray_x + q0.w * ray_y + q1.x;
            const float n2 = q0.z * ray_x + q1.x * ray_y + q1.y;
            const float aaf = ray_x * n0 + ray_y * n1 + n2;
            const float bhalf = q1.z * ray_x + q1.w * ray_y + q2.x;
            done = blend_entry(st, round_base + (unsigned)j + 1u, n0, n1, n2, aaf, bhalf, q2.y, q2.z, q3.x, q3.y, q3.z);
        }
    }

    if (inside) {
        const float* bg = background + (bg_per_view ? 3 * view : 0);
        const float Tr = st.Tr;
        const float distortion_before_normalized = st.distortion;
        const float distortion = (float)(st.distortion / ((1 - Tr) * (1 - Tr) + 1e-7));

        if (SAVE_AUX) {
            float* fT = final_T + (size_t)view * 4 * HW;
            fT[pix_id] = Tr;
            fT[pix_id + HW] = st.dist1;
            fT[pix_id + 2 * HW] = st.dist2;
            fT[pix_id + 3 * HW] = distortion_before_normalized;
            unsigned* nc = n_contrib + (size_t)view * 2 * HW;
            nc[pix_id] = st.last_contributor;
            nc[pix_id + HW] = st.max_contributor;
        }
        float* out = out_color + (size_t)view * F3DG_OUT_CHANNELS * HW;
        out[0 * HW + pix_id] = st.C0 + Tr * bg[0];
        out[1 * HW + pix_id] = st.C1 + Tr * bg[1];
        out[2 * HW + pix_id] = st.C2 + Tr * bg[2];
        out[3 * HW + pix_id] = st.C3;
        out[4 * HW + pix_id] = st.C4;
        out[5 * HW + pix_id] = st.C5;
        out[6 * HW + pix_id] = st.C6;
        out[7 * HW + pix_id] = st.C7;
        out[8 * HW + pix_id] = distortion;
    }
}

// Work counters of the one-wave kernel (option render_count = 1; f3dg_debug_render_counts): [0] list entries staged (record gathers),
// [1] list entries scanned, [2] phase-2 trips (wave iterations), [3] slides, [4] lane-trips = (pixel, entry) pairs that entered phase 2
// ([4] / (64 [2]) = lane utilisation of phase 2), [5] waves, [6] / [7] the trips of slides that began with at most 8 / at most 24 of the
// quadrant's 64 pixels still unsaturated, [8] / [9] those slides. 64 rows against atomic contention; summed on the host.
__device__ unsigned long long g_f3dg_counts[64][16];
// =====================================================================================================================
// render3: ONE wave64 per 8x8 pixel quadrant of a tile -- no workgroup barriers, nothing shared between waves.
//
// A workgroup of four waves per tile (round 2's kernel) couples them through two __syncthreads per staging round: an instrumented build attributes 25-30 % of
// a wave's life to waiting at them (the quadrants of a tile have different amounts of work) and 20-40 % to the staged gathers, which
// all four waves sit out together; VALU issue reaches ~62 %. Here a workgroup is one wave that owns a quadrant from its first list
// entry to its last pixel's saturation and then retires; the SIMD's other waves (other quadrants, other tiles, up to 8 per SIMD) fill
// every wait, and a quadrant stops staging as soon as ITS 64 pixels are finished instead of the tile's 256.
//
//   scan     the tile's list is read 64 ids at a time (the next 64 are always in flight); an entry is kept when the quadrant's bit
//            of the mask that instance generation left above the id is set (F3DG_ID_BITS: the box of the conservative ellipse
//            reaches the quadrant). Kept (list position, id) pairs queue up in a 128-entry LDS ring until 64 are waiting.
//   stage    lane e takes queue entry e: its 64-byte record goes to LDS by four global_load_lds_dwordx4 (no VGPRs, no ds_write; the
//            LDS image [chunk][entry] is exactly the structure-of-arrays phase 2 wants), its ellipse stays in five registers.
//   phase 1  Gaussians across the lanes: lane e evaluates its entry's ellipse at the quadrant's 64 pixels; each comparison is a wave
//            ballot and lands, by two v_writelane, in the lane that owns the pixel (quad_ballots): 5 instructions per 64 tests, no
//            per-block lists, no ds_bpermute.
//   phase 2  pixels across the lanes: every pixel walks its own 64-bit pass mask in list order through the reference's recurrence
//            (f3dg_fused_trip of f3dg_blend.h); the bit index IS the LDS slot, so no per-block index list is read.
// The conservative filters only drop pairs that are a bare `continue` in the reference, so the images are bit-identical to the
// plain transcription within an arithmetic mode (tests/test_raster_forward_gpu.py). LDS: 4 KB of records + 1 KB of queue per wave.

// ---- render3 with a SLIDING window (the default) ----------------------------------------------------------------------------------
// With fixed 64-entry windows every lane waits at the end of a window for the lane with the most passing entries: the CPU model
// (tests/tools/wave1_model.py) puts the lane utilisation of phase 2 at 0.54. Here the 64 staged entries are two halves of 32; a slide
// retires the older half -- which every live pixel has finished -- stages 32 new entries in its place and tests them (lanes e and
// e + 32 share entry e and split the quadrant's rows: half_ballots), and phase 2 runs until the now-older half is finished by
// everybody, pixels that are through with it already working on the newer half. Same LDS (4 KB of records), same phase-1 cost per
// entry; the model gives 0.64 (15 % fewer phase-2 trips). Per pixel the sequence of blended entries is unchanged. The scan, the staging,
// phase 1 and the slide are F3dgHalfWindow (f3dg_quad.h), shared with render4 and render5.
// One quadrant wave per workgroup, 8 waves per SIMD (every variant fits 64 VGPRs and 5 KB of LDS).
template <bool SAVE_AUX, bool FAST, bool NORMAL = true, bool DIST = true, bool COUNT = false>
__global__ void __launch_bounds__(64, 8)
render3s_fwd_kernel(int V, int P, int W, int H, int tiles_x, int T, float focal_x, float focal_y,
                    const F3dgHeader* __restrict__ hdr, const uint2* __restrict__ ranges,
                    const unsigned* __restrict__ point_list, const F3dgRec* __restrict__ rec,
                    const float4* __restrict__ cull, const float* __restrict__ background, int bg_per_view,
                    float* __restrict__ out_color, float* __restrict__ final_T, unsigned* __restrict__ n_contrib)
{
    const F3dgQuad qd = f3dg_quad(V, T, tiles_x);
    const unsigned view = qd.view;
    const unsigned lane = threadIdx.x & 63u;
    const auto [pix_x, pix_y, inside, pix_id, ray_x, ray_y] = f3dg_quad_pixel(qd, lane, W, H, focal_x, focal_y);
    const size_t HW = (size_t)H * W;

    __shared__ float4 sR[4][64];                              // records, [16-byte chunk][slot]; slots 0..31 and 32..63 are the two halves of the window
    __shared__ unsigned sQ[F3DG_QUAD_RING];                   // ids of kept entries not staged yet, ring
    __shared__ unsigned sQpos[SAVE_AUX ? F3DG_QUAD_RING : 1]; // ... and their positions in the tile's list
    __shared__ unsigned sP[SAVE_AUX ? 64 : 1];                // list position of every staged slot (the reference's `contributor`)

    bool done = !inside;
    F3dgPixel st;
    f3dg_pixel_init(st);

    unsigned n_useful = 0;
    unsigned n_half_sep = 0, n_half_pair = 0;
    unsigned n_staged = 0, n_trips = 0, n_wave_trips = 0, n_slides = 0, n_t8 = 0, n_t24 = 0, n_s8 = 0, n_s24 = 0;    // COUNT (option render_count): what this wave did, summed into g_f3dg_counts at its end
    F3dgHalfWindow<SAVE_AUX> win(sR, sQ, sQpos, sP, qd, lane, P, T, hdr, ranges, point_list, rec, cull);
    unsigned long long& pass = win.pass;
    if (__ballot(!done) != 0ull)
    for (;;) {
        win.translate(win.flip, st.last_contributor, st.max_contributor);     // the older half retires
        if (!win.slide(done))
            break;                                // nothing left to stage, nothing left in the newer half
        if (COUNT) {        // staged entries that reach at least one pixel that is still alive (the others were gathered for nothing)
            n_staged += win.m;
            n_slides++;
            unsigned u = done ? 0u : (unsigned)win.fresh;
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) u |= (unsigned)__shfl_xor((int)u, o, 64);
            n_useful += (unsigned)__popc(u);
        }
        const unsigned xr = win.xr;

        // ---- phase 2: until every live pixel has finished the older half; pixels that have go on with the newer one
        // (a divergent loop: a pixel leaves it when its mask is empty -- it has nothing left in either half -- and the ballot, taken
        // over the pixels still inside, ends it for everybody once no older-half bit is left)
        const unsigned trips_before = n_trips;
        const unsigned live_now = COUNT ? (unsigned)__popcll(__ballot(!done)) : 0u;
        while (pass != 0ull && __ballot((unsigned)pass != 0u) != 0ull) {
            const unsigned j = (unsigned)__builtin_ctzll(pass) ^ xr;
            pass &= pass - 1;
            if (COUNT) n_trips++;
            done = f3dg_fused_trip<FAST, NORMAL, DIST>(st, sR, j, F3DG_SLOT_FLAG | j, ray_x, ray_y);
            if (done) pass = 0ull;
        }
        if (COUNT) {                // the loop ran as often as its busiest lane needed (lanes leave it, none re-enters)
            unsigned t = n_trips - trips_before;
            {
                // what TWO pixels per lane would buy, emulated at half scale: the wave's two 8 x 4 halves as separate 32-lane walks
                // (each lasts as long as its busiest pixel) against one 32-lane walk whose lane i takes pixel i and then pixel i + 32
                unsigned th = t, tp = t + (unsigned)__shfl_xor((int)t, 32, 64);
#pragma unroll
                for (int o = 16; o > 0; o >>= 1) {
                    th = max(th, (unsigned)__shfl_xor((int)th, o, 64));
                    tp = max(tp, (unsigned)__shfl_xor((int)tp, o, 64));
                }
                n_half_sep += th + (unsigned)__shfl_xor((int)th, 32, 64);
                n_half_pair += tp;
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) t = max(t, (unsigned)__shfl_xor((int)t, o, 64));
            n_wave_trips += t;
            if (live_now <= 8u) { n_t8 += t; n_s8++; }
            if (live_now <= 24u) { n_t24 += t; n_s24++; }
        }
        const unsigned long long live = __ballot(!done);
        if (live == 0ull)
            break;
    }
    win.translate(2u, st.last_contributor, st.max_contributor);
    if (COUNT && lane == 0) {
        unsigned long long* c = g_f3dg_counts[blockIdx.x & 63u];
        atomicAdd(&c[13], (unsigned long long)n_useful);
        atomicAdd(&c[14], (unsigned long long)n_half_sep);
        atomicAdd(&c[15], (unsigned long long)n_half_pair);
        atomicAdd(&c[0], (unsigned long long)n_staged);
        atomicAdd(&c[1], (unsigned long long)(win.cursor < win.n ? win.cursor : win.n));
        atomicAdd(&c[2], (unsigned long long)n_wave_trips);
        atomicAdd(&c[3], (unsigned long long)n_slides);
        atomicAdd(&c[5], 1ull);
        atomicAdd(&c[6], (unsigned long long)n_t8);
        atomicAdd(&c[7], (unsigned long long)n_t24);
        atomicAdd(&c[8], (unsigned long long)n_s8);
        atomicAdd(&c[9], (unsigned long long)n_s24);
    }
    if (COUNT) {
        unsigned t = n_trips;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) t += (unsigned)__shfl_xor((int)t, o, 64);
        if (lane == 0) atomicAdd(&g_f3dg_counts[blockIdx.x & 63u][4], (unsigned long long)t);
    }

    if (inside)
        f3dg_pixel_store<SAVE_AUX, NORMAL, DIST>(st, view, pix_id, HW, background, bg_per_view, out_color, final_T, n_contrib);
}

} // namespace

int f3dg_render_uses_fast(int save_aux) { return g_f3dg_render_fast == 2 || (g_f3dg_render_fast == 1 && !save_aux); }

// the compositing forward kernel the last f3dg_launch_render of this host thread launched (what `roofline.kernel` of bench.py prints)
thread_local const char* g_f3dg_last_render_kernel = "";
extern "C" const char* f3dg_debug_last_render_kernel(void) { return g_f3dg_last_render_kernel; }

void f3dg_note_render_kernel(const char* fmt, ...)
{
    thread_local char name[160] = "";       // (per host thread: the library is called from several)
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(name, sizeof name, fmt, ap);
    va_end(ap);
    g_f3dg_last_render_kernel = name;
}

int f3dg_read_render_counts(const void* symbol, int rows, unsigned long long* h_out, int reset)
{
    unsigned long long buf[64][16];
    F3DG_HIP_CHECK(hipMemcpyFromSymbol(buf, symbol, sizeof buf));
    if (h_out)
        for (int k = 0; k < 16; k++) {
            h_out[k] = 0;
            for (int r = 0; r < rows; r++) h_out[k] += buf[r][k];
        }
    if (reset) {
        memset(buf, 0, sizeof buf);
        F3DG_HIP_CHECK(hipMemcpyToSymbol(symbol, buf, sizeof buf));
    }
    return F3DG_OK;
}

namespace {

template <bool AUX, bool FAST, bool NORMAL, bool DIST, bool COUNT>
void launch3s(const F3dgRenderLaunch& a)
{
    F3DG_KLAUNCH((render3s_fwd_kernel<AUX, FAST, NORMAL, DIST, COUNT>), a.quadrants(), dim3(64), 0, a.s,
                 a.V, a.P, a.W, a.H, a.tiles_x, a.T, a.focal_x, a.focal_y, a.hdr, a.ranges, a.point_list, a.rec, a.cull, a.background, a.bg_per_view,
                 a.out_color, a.final_T, a.n_contrib);
}

template <bool AUX>
void launch_plain(const F3dgRenderLaunch& a)
{
    F3DG_KLAUNCH((render_fwd_kernel<AUX>), dim3((unsigned)a.V * (unsigned)a.T), dim3(F3DG_BLOCK), 0, a.s, a.V, a.P, a.W, a.H, a.tiles_x, a.T, a.focal_x, a.focal_y,
                 a.hdr, a.ranges, a.point_list, a.rec, a.background, a.bg_per_view, a.out_color, a.final_T, a.n_contrib);
}

const char* tf(int b) { return b ? "true" : "false"; }

} // namespace

// The compositing forward of a call. The arithmetic is the CALL's (f3dg_forward_sets resolves its flags against the process default and
// records the choice in the workspace header for the backward): fast arithmetic is for inference calls -- a SAVE_AUX forward feeds
// f3dg_backward, which rebuilds every pixel's transmittance back to front by dividing final_T by (1 - alpha) with ITS alphas: they must be
// the forward's to the bit, or the 1e-6 relative difference is amplified by 1 / (1 - alpha) per layer (measured at C5: compositing-stage
// gradients 2.5e-5 instead of 1.8e-6 off the oracle).
int f3dg_launch_render(hipStream_t s, int V, int P, int W, int H, float focal_x, float focal_y,
                       const F3dgHeader* hdr, const uint2* ranges, const unsigned* point_list, const F3dgRec* rec,
                       const float4* cull, const float* background, int bg_per_view, float* out_color,
                       float* final_T, unsigned* n_contrib, int save_aux, unsigned skip_channels, int fast_arg, int scan)
{
    const int tiles_x = (W + F3DG_TILE - 1) / F3DG_TILE, tiles_y = (H + F3DG_TILE - 1) / F3DG_TILE;
    const int T = tiles_x * tiles_y;
    const int fast = fast_arg < 0 ? f3dg_render_uses_fast(save_aux) : fast_arg;
    const F3dgRenderLaunch a = { s, V, P, W, H, tiles_x, T, focal_x, focal_y, hdr, ranges, point_list, rec, cull, background, bg_per_view,
                                 out_color, final_T, n_contrib, fast, save_aux, skip_channels, g_f3dg_render_count };
    const long long waves = (long long)V * T * 4;           // one wave per 8 x 8 pixel quadrant
    if (g_f3dg_reference_kernels) {
        // the plain transcription (the reference's arithmetic only: f3dg_forward_sets runs such a call with fast = 0)
        if (fast) return F3DG_ERR_BAD_ARG;
        if (save_aux) launch_plain<true>(a); else launch_plain<false>(a);
        f3dg_note_render_kernel("render_fwd_kernel<SAVE_AUX=%s, FAST=false>", tf(save_aux));
        F3DG_HIP_CHECK(hipGetLastError());
        return F3DG_OK;
    }
    // (1) small launches -- at most two waves per SIMD: one or two 256^2 views -- are latency chains nobody fills
    const bool small_launch = g_f3dg_render_lowocc && waves <= (g_f3dg_render_lowocc > 1 ? 1024ll * g_f3dg_render_lowocc : 2048ll);
    // (2) the split-pixel schedule of f3dg_render5.hip: fast inference launches that ask for it (F3DG_FLAG_SCAN, whatever their size) or,
    // with option render_scan 1, every such launch that is not small
    if (fast && !save_aux && g_f3dg_render_scan != 0 && (scan || g_f3dg_render_scan == 1))
        // small: one or two views, four lanes per pixel instead of helper-lane batches (render5p_fwd_kernel)
        return small_launch ? f3dg_launch_render5_small(a) : f3dg_launch_render5(a);
    if (small_launch) {
        // the multi-wave kernels of f3dg_render4.hip. Defaults by measurement at 65,536 pixel-ordered Gaussians (profiles/r05_final/
        // one_view.md): fast arithmetic -- producer + consumer waves, two entries per trip (render3p, 76.6 -> 57.9 us; two views 79.7 ->
        // 63.6 us per call); the reference's arithmetic -- consumer + three evaluator waves + producer for one view (render3q, 134 -> 100 us:
        // its LDS does not fit two quadrants per SIMD), render3p for two
        const bool one_view = waves <= 1024ll;
        const int split = g_f3dg_render_split >= 1 ? g_f3dg_render_split : fast ? 1 : one_view ? 3 : 1;
        const int unroll = g_f3dg_render_unroll >= 1 ? g_f3dg_render_unroll : fast ? 2 : 1;
        return f3dg_launch_render_small(a, unroll, split);
    }
    // (3) the rank-packed kernel of f3dg_render4.hip (option render_pack: 1 = every launch, -1 = the default: launches in the reference's
    // arithmetic, whose stateless part is 2.5 x as long -- measured -38 % on the real merged set, -6 % at C2; in fast arithmetic the packed
    // trips' hand-over costs what they save: 8.4-8.7 against 8.6 ms). A SAVE_AUX forward in the reference's
    // arithmetic takes it too (its auxiliary planes are bit-identical to render3s's).
    if (g_f3dg_render_pack == 1 || (g_f3dg_render_pack < 0 && !fast))
        return f3dg_launch_render4(a);
    // (4) render3s_fwd_kernel: one wave per quadrant, sliding half-windows
    const bool lean = a.lean();
    const bool count = a.count && !save_aux;        // (diagnostic: the same kernel with its work counters on)
    const char* extra = "";
    if (count) {
        if (fast) launch3s<false, true, true, true, true>(a); else launch3s<false, false, true, true, true>(a);
        extra = ", COUNT=true";
    } else if (lean) {
        if (fast) launch3s<false, true, false, false, false>(a); else launch3s<false, false, false, false, false>(a);
        extra = ", NORMAL=false, DIST=false";
    } else if (save_aux) {
        if (fast) launch3s<true, true, true, true, false>(a); else launch3s<true, false, true, true, false>(a);
    } else {
        if (fast) launch3s<false, true, true, true, false>(a); else launch3s<false, false, true, true, false>(a);
    }
    f3dg_note_render_kernel("render3s_fwd_kernel<SAVE_AUX=%s, FAST=%s, OCC=8, WPB=1%s>", tf(lean || count ? 0 : save_aux), tf(fast), extra);
    F3DG_HIP_CHECK(hipGetLastError());
    return F3DG_OK;
}

// debug: the work counters of the counting variant of the one-wave kernel (option render_count = 1), summed over all launches since
// the last reset: h_out8[16] = { staged, scanned, wave trips, slides, lane-trips, waves, trips with <= 8 / <= 24 live pixels, slides with <= 8 / <= 24, 0... }
extern "C" int f3dg_debug_render_counts(unsigned long long* h_out8, int reset) { return f3dg_read_render_counts(&g_f3dg_counts, 64, h_out8, reset); }

// debug: the phase-timing counters of earlier builds; no kernel is instrumented any more, so they are zeros
extern "C" int f3dg_debug_timing(unsigned long long* h_out8, int reset)
{
    (void)reset;
    if (h_out8) memset(h_out8, 0, 8 * sizeof(unsigned long long));
    return F3DG_OK;
}
