// f3dg_quad.h -- the front end of the quadrant kernels: a workgroup's 8x8 pixel quadrant and its lane's pixel, the tile's list range,
// and F3dgHalfWindow, the sliding half-window of the one-wave compositing forwards (render3s_fwd_kernel, render4_fwd_kernel,
// render5_fwd_kernel) up to and including phase 1. Phase 2 is the kernel's own loop around f3dg_fused_trip
// (f3dg_blend.h). Everything here is force-inlined. The plain reference kernels (render_fwd_kernel, integrate_pass1_kernel) do not use
// this header: the bit-identity tests compare every other path against them.
#pragma once
#include "f3dg_common.h"
#include "f3dg_ellipse.h"

#define F3DG_QUAD_RING 128          // ring of kept entries not staged yet
#define F3DG_SLOT_FLAG 0x80000000u  // a forward's contributor values are slots (flag | slot) until the window that holds the slot ends

// LDS written by some lanes of the wave is read by others
__device__ __forceinline__ void f3dg_wave_fence()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// v of the lane whose byte address (4 lane) is addr
__device__ __forceinline__ float f3dg_pull(int addr, float v)
{
    return __int_as_float(__builtin_amdgcn_ds_bpermute(addr, __float_as_int(v)));
}

// set bits of kb below this lane: a kept entry's offset in the ring
__device__ __forceinline__ unsigned f3dg_rank(unsigned long long kb)
{
    return __builtin_amdgcn_mbcnt_hi((unsigned)(kb >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)kb, 0u));
}

// the tile's range of the list; none after an overflow
__device__ __forceinline__ uint2 f3dg_tile_range(const F3dgHeader* hdr, const uint2* ranges, unsigned view, int T, unsigned tile)
{
    uint2 range = ranges[(size_t)view * T + tile];
    if (hdr->overflow) range = make_uint2(0, 0);
    return range;
}

// A workgroup is one (view, tile, quadrant) -- spread over the XCDs by f3dg_xcd_map; (qx0, qy0) is the quadrant's first pixel
struct F3dgQuad {
    unsigned view, tile, quad, qx0, qy0;
};
__device__ __forceinline__ F3dgQuad f3dg_quad(int V, int T, int tiles_x)
{
    F3dgQuad q;
    unsigned unit;
    f3dg_xcd_map(blockIdx.x, (unsigned)V, 4u * (unsigned)T, q.view, unit);
    q.tile = unit >> 2;
    q.quad = unit & 3u;
    const unsigned tile_x = q.tile % (unsigned)tiles_x, tile_y = q.tile / (unsigned)tiles_x;
    q.qx0 = tile_x * F3DG_TILE + (q.quad & 1u) * 8u;
    q.qy0 = tile_y * F3DG_TILE + (q.quad >> 1) * 8u;
    return q;
}

// pixel p (0..63, row-major) of the quadrant and its ray, in the reference's arithmetic (double): the bit-identity tests depend on it
struct F3dgQuadPixel {
    unsigned x, y;
    bool inside;
    size_t id;                    // y W + x
    float ray_x, ray_y;
};
__device__ __forceinline__ F3dgQuadPixel f3dg_quad_pixel(const F3dgQuad& q, unsigned p, int W, int H, float focal_x, float focal_y)
{
    F3dgQuadPixel px;
    px.x = q.qx0 + (p & 7u);
    px.y = q.qy0 + (p >> 3);
    px.inside = px.x < (unsigned)W && px.y < (unsigned)H;
    px.id = (size_t)W * px.y + px.x;
    const float pixf_x = (float)px.x + 0.5f, pixf_y = (float)px.y + 0.5f;
    px.ray_x = (float)((pixf_x - W / 2.) / focal_x);
    px.ray_y = (float)((pixf_y - H / 2.) / focal_y);
    return px;
}

// ---- the forward: a SLIDING window of two halves of 32 staged entries ------------------------------------------------------------------
//   scan     the tile's list is read front to back 64 ids at a time (the next 64 are always in flight); an entry is kept when the
//            quadrant's bit of the mask that instance generation left above the id is set (F3DG_ID_BITS). Kept ids queue up in an LDS
//            ring until 32 are pending;
//   stage    a slide retires the older half -- which every live pixel has finished -- and stages up to 32 entries in its place: lane e
//            takes entry e, its 64-byte record goes to LDS by four global_load_lds_dwordx4 (the image [chunk][slot] is what phase 2
//            reads), its ellipse stays in registers;
//   phase 1  lanes e and e + 32 test entry e against the quadrant's rows 0-3 and 4-7 (half_ballots): the pass bits land in the lanes
//            that own the pixels, and the fresh bits become the newer half of `pass`.
// With AUX (a kernel that writes the auxiliary planes) the ring keeps the list positions as well, and every staged slot its position
// (sP): contributor values are F3DG_SLOT_FLAG | slot until translate() turns them into 1-based list positions, when their half retires.
// LDS the kernel declares: float4 sR[4][64]; unsigned sQ[F3DG_QUAD_RING]; with AUX unsigned sQpos[F3DG_QUAD_RING], sP[64].
template <bool AUX>
struct F3dgHalfWindow {
    float4 (*sR)[64];
    unsigned *sQ, *sQpos, *sP;
    const unsigned* point_list;
    const F3dgRec* vrec;
    const float4* vcull;
    unsigned start, n, qbit, qx0, qy0, lane;
    unsigned cursor, qhead, qpend;    // wave-uniform: scan position, ring index of the first pending entry, pending entries
    unsigned flip;                    // physical half (slots 32 flip ..) that holds the OLDER half of the window
    unsigned xr;                      // logical slot j (0..31 older, 32..63 newer) lives in physical slot j ^ xr
    unsigned m;                       // entries the last slide staged
    int fresh;                        // the pass bits phase 1 of the last slide left in this lane
    unsigned idn;                     // the next 64 ids of the list
    unsigned long long pass;          // per pixel: bits 0..31 older half, 32..63 newer half, in list order

    __device__ __forceinline__ F3dgHalfWindow(float4 (*sR_)[64], unsigned* sQ_, unsigned* sQpos_, unsigned* sP_, const F3dgQuad& q, unsigned lane_,
                                              int P, int T, const F3dgHeader* hdr, const uint2* ranges, const unsigned* point_list_,
                                              const F3dgRec* rec, const float4* cull)
        : sR(sR_), sQ(sQ_), sQpos(sQpos_), sP(sP_), point_list(point_list_), vrec(rec + (size_t)q.view * P), vcull(cull + (size_t)q.view * P),
          qbit(1u << (F3DG_ID_BITS + q.quad)), qx0(q.qx0), qy0(q.qy0), lane(lane_), cursor(0), qhead(0), qpend(0), flip(0), xr(0), m(0),
          fresh(0), pass(0ull)
    {
        const uint2 range = f3dg_tile_range(hdr, ranges, q.view, T, q.tile);
        start = range.x;
        n = range.y - range.x;
        idn = lane < n ? point_list[start + lane] : 0u;
    }

    // slots -> 1-based list positions for the contributors held in one physical half (2: both)
    __device__ __forceinline__ void translate(unsigned half_or_all, unsigned& last_contributor, unsigned& max_contributor) const
    {
        if (AUX) {
            const unsigned a = last_contributor - F3DG_SLOT_FLAG, b = max_contributor - F3DG_SLOT_FLAG;
            if (a < 64u && (half_or_all == 2u || (a >> 5) == half_or_all)) last_contributor = sP[a] + 1u;
            if (b < 64u && (half_or_all == 2u || (b >> 5) == half_or_all)) max_contributor = sP[b] + 1u;
        }
    }

    // one slide, when every live pixel has finished the older half (bits 0..31 of `pass` are clear; with AUX the caller has translated
    // its contributors: translate(flip, ...)): scan, stage and test up to 32 entries in place of the older half, slide. false: nothing
    // was left to stage and nothing is left in the newer half
    __device__ __forceinline__ bool slide(bool done)
    {
        while (qpend < 32u && cursor < n) {
            const unsigned idm = idn, pos = cursor + lane;
            cursor += 64u;
            idn = cursor + lane < n ? point_list[start + cursor + lane] : 0u;
            const bool keep = pos < n && (idm & qbit) != 0u;
            const unsigned long long kb = __ballot(keep);
            if (keep) {
                const unsigned slot = (qhead + qpend + f3dg_rank(kb)) & (F3DG_QUAD_RING - 1);
                sQ[slot] = idm & F3DG_ID_MASK;
                if (AUX) sQpos[slot] = pos;
            }
            qpend += (unsigned)__popcll(kb);
        }
        m = qpend < 32u ? qpend : 32u;
        if (m == 0u && __ballot(pass != 0ull) == 0ull)
            return false;
        f3dg_wave_fence();

        // ---- stage m entries into the retired half; lanes e and e + 32 both take entry e
        const unsigned hl = lane & 31u;               // entry of a half this lane tests in phase 1 ...
        const unsigned row4 = (lane >> 5) * 4u;       // ... against the pixels of rows row4 .. row4 + 3
        const unsigned base = flip * 32u;
        float4 e4 = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        float ec = 0.0f;
        if (hl < m) {
            const unsigned id = sQ[(qhead + hl) & (F3DG_QUAD_RING - 1)];
            if (lane < 32u) {
                const float4* src = reinterpret_cast<const float4*>(vrec + id);
#pragma unroll
                for (int c = 0; c < 4; c++)
                    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(src + c),
                                                     (__attribute__((address_space(3))) void*)&sR[c][base], 16, 0, 0);
                if (AUX) sP[base + lane] = sQpos[(qhead + hl) & (F3DG_QUAD_RING - 1)];
            }
            e4 = vcull[id];
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        f3dg_wave_fence();
        if (hl < m) ec = sR[3][base + hl].w;
        qhead += m;
        qpend -= m;

        // ---- phase 1: the new entries against the quadrant's 64 pixels
        fresh = 0;
        if (m != 0u) {
            const float u0 = hl < m ? (float)qx0 - e4.x : __builtin_nanf("");     // NaN: every comparison below is false
            const float v0 = (float)(qy0 + row4) - e4.y;
            float dxx[8], adx[8], dyy[4], cdy[4];
#pragma unroll
            for (int q = 0; q < 8; q++) {
                dxx[q] = u0 + (float)q;
                adx[q] = e4.z * dxx[q];
            }
#pragma unroll
            for (int q = 0; q < 4; q++) {
                dyy[q] = v0 + (float)q;
                cdy[q] = ec * dyy[q] * dyy[q];
            }
            half_ballots<0>(fresh, fmaf(dxx[0], fmaf(e4.w, dyy[0], adx[0]), cdy[0]), dxx, adx, dyy, cdy, e4.w);
        }
        // ---- slide: the newer half becomes the older one, the fresh bits the newer one
        pass = (pass >> 32) | (done ? 0ull : ((unsigned long long)(unsigned)fresh << 32));
        flip ^= 1u;
        xr = flip << 5;
        return true;
    }
};

// ---- the backward: windows of 64 kept entries, BACK to front ---------------------------------------------------------------------------
// The list the workspace's forward left (a one-view forward with auxiliary planes may have taken the small-call path: its lists live in
// the per-tile slots) and the pixel's inputs (the forward's auxiliary planes, dL/dpixels); the scan from the deepest last contributor
// of the quadrant's pixels back to the list's first entry into a ring of (list position, id); a window's staging -- record by
// global_load_lds, 2D conic, projected centre -- and phase 1: lane e tests entry e against the 64 pixels (quad_ballots_any), every
// pixel gets its pass mask and the wave the mask of entries that can reach ANY of its pixels. Shared by render3_bwd_kernel and
// render5_bwd_kernel; what they do with a window's pairs is in f3dg_bwd_pair.h and in the kernels. The constructor takes the launch
// record's device part (F3dgBwdLaunch::Args, f3dg_common.h), the kernel's LDS, its quadrant and the lane's pixel.
// LDS the kernel declares: float4 sR[4][64] records, float4 sC[64] 2D conic + opacity * coef, uint2 sQ[F3DG_QUAD_RING]; the projected
// centre goes to float2 sX[64] or, with CENTRE_IN_CONIC, its x over sC[j].w (the record carries opacity * coef as well: word 10,
// sR[2][j].z) and its y to float sY[64].
template <bool CENTRE_IN_CONIC>
struct F3dgBwdWindow {
    float4 (*sR)[64];
    float4* sC;
    float2* sX;
    float* sY;
    uint2* sQ;
    const unsigned* point_list;
    const F3dgRec* vrec;
    const float4* vcull;
    const float2* means2D;
    const float4* conic;
    size_t vP;
    unsigned start, qbit, qx0, qy0, lane;
    bool alpha_fast;                  // the forward took the fast arithmetic: alpha is repeated with f3dg_fast_t_G
    // the pixel's inputs (0 outside the image)
    float T_final, final_D, final_A, dL_dreg;
    int last_contributor, max_contributor;
    float dpx0, dpx1, dpx2, dn0, dn1, dn2, dL_dmax_depth;
    float ddelx_dx, ddely_dy, bg_dot_dpixel;
    // the walk
    unsigned cursor, qhead, qcount;   // wave-uniform: list positions [0, cursor) are still to be scanned, ring head, kept entries in the ring
    unsigned idn;                     // the next 64 ids of the list (back to front: lane l reads position cursor - 1 - l)
    unsigned m;                       // entries of the window
    unsigned long long pass, any;     // phase 1: the pixel's pass mask; the entries that reach any pixel of the quadrant

    __device__ __forceinline__ F3dgBwdWindow(const F3dgBwdLaunch::Args& a, float4 (*sR_)[64], float4* sC_, float2* sX_, float* sY_, uint2* sQ_,
                                             const F3dgQuad& q, bool inside, size_t pix_id, unsigned lane_)
        : sR(sR_), sC(sC_), sX(sX_), sY(sY_), sQ(sQ_), means2D(a.means2D), conic(a.conic), qx0(q.qx0), qy0(q.qy0), lane(lane_), qhead(0),
          qcount(0), m(0), pass(0ull), any(0ull)
    {
        F3dgHeader* const hdr = a.hdr;
        const int W = a.W, H = a.H;
        uint2 range = a.ranges[(size_t)q.view * a.T + q.tile];
        // no lists to walk after an overflow -- and none that belong to this call when the workspace's last forward kept no auxiliary
        // planes (an inference call): all gradients stay zero, the header says why
        point_list = hdr->small_path != 0u ? a.small_list : a.point_list_general;
        if (hdr->overflow || hdr->save_aux == 0u) {
            range = make_uint2(0, 0);
            if (!hdr->overflow && blockIdx.x == 0 && threadIdx.x == 0) hdr->bwd_stale = 1u;
        }
        start = range.x;
        alpha_fast = hdr->alpha_fast != 0;

        vP = (size_t)q.view * a.P;
        vrec = a.rec + vP;
        vcull = a.cull + vP;
        const size_t HW = (size_t)H * W;
        const float* fT = a.final_T + (size_t)q.view * 4 * HW;
        const unsigned* nc = a.n_contrib + (size_t)q.view * 2 * HW;
        const float* dpix = a.dL_dpixels + (size_t)q.view * F3DG_OUT_CHANNELS * HW;
        const float* bg = a.background + (a.bg_per_view ? 3 * q.view : 0);
        T_final = inside ? fT[pix_id] : 0;
        final_D = inside ? fT[pix_id + HW] : 0;
        final_A = 1 - T_final;
        dL_dreg = inside ? dpix[8 * HW + pix_id] : 0;
        last_contributor = inside ? (int)nc[pix_id] : 0;
        max_contributor = inside ? (int)nc[pix_id + HW] : 0;
        dpx0 = dpx1 = dpx2 = dn0 = dn1 = dn2 = dL_dmax_depth = 0;
        if (inside) {
            dpx0 = dpix[pix_id]; dpx1 = dpix[HW + pix_id]; dpx2 = dpix[2 * HW + pix_id];
            dn0 = dpix[3 * HW + pix_id]; dn1 = dpix[4 * HW + pix_id]; dn2 = dpix[5 * HW + pix_id];
            dL_dmax_depth = dpix[6 * HW + pix_id];
        }
        ddelx_dx = (float)(0.5 * W);
        ddely_dy = (float)(0.5 * H);
        bg_dot_dpixel = bg[0] * dpx0 + bg[1] * dpx1 + bg[2] * dpx2;

        // entries at or behind a pixel's last contributor are skipped by the reference one by one (backward.cu:745-746): the wave starts
        // at the deepest last contributor of ITS 64 pixels
        const int wave_last = min((int)__builtin_amdgcn_readfirstlane((int)__reduce_max_sync(~0ull, last_contributor)),
                                  (int)(range.y - range.x));
        qbit = 1u << (F3DG_ID_BITS + q.quad);
        cursor = (unsigned)wave_last;
        idn = lane < cursor ? point_list[start + cursor - 1u - lane] : 0u;
    }

    // (list position from the front, id) of window slot j
    __device__ __forceinline__ uint2 entry(unsigned j) const { return sQ[(qhead + j) & (F3DG_QUAD_RING - 1)]; }

    // the next window: scan until 64 entries are kept, stage them, phase 1. false: the list is done
    __device__ __forceinline__ bool next()
    {
        while (qcount < 64u && cursor != 0u) {
            const unsigned idm = idn;
            const bool valid = lane < cursor;
            const unsigned pos = cursor - 1u - lane;
            cursor = cursor > 64u ? cursor - 64u : 0u;
            idn = lane < cursor ? point_list[start + cursor - 1u - lane] : 0u;
            const bool keep = valid && (idm & qbit) != 0u;
            const unsigned long long kb = __ballot(keep);
            if (keep) sQ[(qhead + qcount + f3dg_rank(kb)) & (F3DG_QUAD_RING - 1)] = make_uint2(pos, idm & F3DG_ID_MASK);
            qcount += (unsigned)__popcll(kb);
        }
        if (qcount == 0u)
            return false;
        m = qcount < 64u ? qcount : 64u;
        f3dg_wave_fence();

        float4 e4 = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        float ec = 0.0f;
        float2 m2 = make_float2(0.0f, 0.0f);
        if (lane < m) {
            const unsigned id = entry(lane).y;
            const float4* src = reinterpret_cast<const float4*>(vrec + id);
#pragma unroll
            for (int c = 0; c < 4; c++)
                __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(src + c),
                                                 (__attribute__((address_space(3))) void*)&sR[c][0], 16, 0, 0);
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(conic + vP + id),
                                             (__attribute__((address_space(3))) void*)&sC[0], 16, 0, 0);
            e4 = vcull[id];
            if (CENTRE_IN_CONIC) m2 = means2D[vP + id];
            else sX[lane] = means2D[vP + id];
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        if (lane < m) {
            ec = sR[3][lane].w;
            if (CENTRE_IN_CONIC) {
                sC[lane].w = m2.x;        // (after the wait: the conic's global_load_lds writes the same 16 bytes)
                sY[lane] = m2.y;
            }
        }
        f3dg_wave_fence();

        // ---- phase 1: lane e tests entry e against the 64 pixels of the quadrant
        int pass_lo = 0, pass_hi = 0;
        any = 0ull;
        {
            const float u0 = lane < m ? (float)qx0 - e4.x : __builtin_nanf("");
            const float v0 = (float)qy0 - e4.y;
            float dxx[8], adx[8], dyy[8], cdy[8];
#pragma unroll
            for (int q = 0; q < 8; q++) {
                dxx[q] = u0 + (float)q;
                adx[q] = e4.z * dxx[q];
                dyy[q] = v0 + (float)q;
                cdy[q] = ec * dyy[q] * dyy[q];
            }
            quad_ballots_any<0>(pass_lo, pass_hi, any, fmaf(dxx[0], fmaf(e4.w, dyy[0], adx[0]), cdy[0]), dxx, adx, dyy, cdy, e4.w);
        }
        pass = ((unsigned long long)(unsigned)pass_hi << 32) | (unsigned)pass_lo;
        return true;
    }

    // the window is done: its ring slots and LDS are rewritten by the next one
    __device__ __forceinline__ void retire()
    {
        qhead += m;
        qcount -= m;
        f3dg_wave_fence();
    }
};
