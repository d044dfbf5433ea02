// f3dg_backward5.hip -- compositing backward with DENSE batches of (pixel, entry) pairs (option bwd_dense; the counterpart of the
// split-pixel forward of f3dg_render5.hip).
//
// render3_bwd_kernel (f3dg_backward.hip) walks the entries that reach any pixel of a quadrant in lock-step: every step costs the wave the
// whole loop body of backward.cu:745-950 -- alpha again, the 17 partials, a transposed reduction over the 64 lanes -- for the pixels the
// entry contributes to: 24 of 64 at C5, 7.7 of 64 on pixel-aligned predicted sets. Here a window's contributing pairs are compacted
// ENTRY-major (a scalar loop over the entries: the ballot of the pixels an entry reaches, every such pixel lane writes its pair at ring
// position tail + mbcnt) and processed 64 to a batch, one pair per lane:
//   * the pair's pixel constants (ray, dL/dpixel, the pixel's totals) come by ds_bpermute from the lane that owns the pixel, its record from
//     the staged window; alpha is recomputed exactly as the forward did (f3dg_bwd_pair_eval);
//   * the per-pixel recurrence -- T rebuilt back to front (a correctly rounded reciprocal per pair, a multiply per layer), the colour /
//     normal blended behind the entry -- lives in LDS
//     (one float4 per pixel) and is advanced entry after entry: the lanes of one entry's run update the slots of their pixels together,
//     successive runs of the batch follow each other. The six recurrences accum_rec[c] / accum_normal[k] of backward.cu are ONE here:
//     they only ever meet dL/dpixel as a dot product and dL/dpixel is constant per pixel;
//   * the 17 partials are summed over the pixels of an entry by segmented scans along its run (f3dg_segscan.h) and added to memory by the
//     run's last lane.
// The arithmetic of a pair is f3dg_bwd_pair.h, shared with render3_bwd_kernel; this kernel's own are the folded recurrence, the
// reciprocal-and-multiply rebuild of T, its rounding of the background term and the order of the per-entry sums (a tree over the run
// instead of a transposed butterfly over the wave): compositing-stage gradients within 1e-5 of the oracle as before
// (tests/test_raster_backward_gpu.py runs with either kernel).
#include "f3dg_common.h"
#include "f3dg_ellipse.h"
#include "f3dg_quad.h"
#include "f3dg_segscan.h"
#include "f3dg_bwd_pair.h"

int g_f3dg_bwd_dense = 1;             // option bwd_dense: 1 (default) = render5_bwd_kernel, 0 = render3_bwd_kernel (the lock-step walk)

namespace {

#define F3DG_B5_STAGE 6             // runs whose totals go through LDS together (12: 8.5 ms at C5, 6: 8.0, 3: 8.2 -- LDS decides the occupancy)
#define F3DG_B5_OCC 5               // 96 VGPRs, 8 KB of LDS: five waves per SIMD

template <int OCC>
__global__ void __launch_bounds__(64, OCC)
render5_bwd_kernel(const F3dgBwdLaunch::Args a)
{
    const F3dgQuad qd = f3dg_quad(a.V, a.T, a.tiles_x);
    const unsigned lane = threadIdx.x;
    const auto [pix_x, pix_y, inside, pix_id, ray_x, ray_y] = f3dg_quad_pixel(qd, lane, a.W, a.H, a.focal_x, a.focal_y);

    __shared__ float4 sR[4][64];          // records of the window, [16-byte chunk][entry] (global_load_lds image)
    __shared__ float4 sC[64];             // 2D conic (x, y, z) and, over the opacity * coef the record carries as well, the projected centre's x
    __shared__ float sY[64];              // the projected centre's y
    __shared__ uint2 sQ[F3DG_QUAD_RING];  // (list position, Gaussian id) of the kept entries, ring
    __shared__ unsigned short sK[128];    // (owning lane << 6) | window slot: the pairs of the batches, entry-major, ring
    __shared__ __attribute__((aligned(16))) float sOut[F3DG_B5_STAGE][20];     // the 17 totals + Gaussian id of up to twelve runs on their way to one-element-per-lane
    __shared__ float4 sS[64];             // per pixel: (T in front of its last blended entry, blended dot behind it, that entry's alpha, its dot)

    F3dgBwdWindow<true> w(a, sR, sC, nullptr, sY, sQ, qd, inside, pix_id, lane);
    const unsigned qx0 = qd.qx0, qy0 = qd.qy0;
    unsigned n_pairs = 0;                 // contributing (pixel, Gaussian) pairs of this wave

    // the pixel's running state of backward.cu:745-810, folded: every accumulated colour / normal only ever meets dL/dpixel as a dot product,
    // and dL/dpixel is constant per pixel, so the six recurrences accum_rec[c] / accum_normal[k] are ONE: A <- alpha' u' + (1 - alpha') A with
    // u = c . dL/dC + n . dL/dN of the entry blended last (alpha', u')
    sS[lane] = make_float4(w.T_final, 0.0f, 0.0f, 0.0f);
    const unsigned el_run = lane / 20u, el = lane - 20u * el_run;      // lane 20 r + c adds element c of the r-th run of a group of three
    const float TfBg = w.T_final * w.bg_dot_dpixel;
    // one 128-byte record per (view, Gaussian) takes all 17 sums of an entry: ten float64 (view2gaussian) at byte 0, seven float32 (colour,
    // mean2D, opacity) at byte 80 -- an atomic event touches ONE line (three 64-byte requests at most) instead of four arrays;
    // preprocess_bwd_kernel hands the float32 ones to the caller's arrays
    double* const gacc = a.dL_dv2g_acc + w.vP * 16;
    while (w.next()) {
        // ---- the window's contributing (pixel, entry) pairs, ENTRY-major (back to front: window slot order), 64 to a batch
        unsigned long long todo = w.any;
        unsigned qh = 0u, qt = 0u;                        // wave-uniform ring counters of this window
        const int slot_pos = (int)w.entry(lane).x;       // lane j: list position of window slot j (read back with v_readlane: no LDS round trip per entry)
        do {
            while (todo != 0ull && qt - qh < 64u) {
                const int j = __builtin_ctzll(todo);
                todo &= todo - 1ull;
                const int contributor = __builtin_amdgcn_readlane(slot_pos, j);      // 0-based position from the front
                const bool mine = inside && ((w.pass >> j) & 1ull) != 0ull && contributor < w.last_contributor;
                const unsigned long long rowmask = __ballot(mine);
                if (rowmask == 0ull)
                    continue;
                const unsigned r = __builtin_amdgcn_mbcnt_hi((unsigned)(rowmask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)rowmask, 0u));
                if (mine) sK[(qt + r) & 127u] = (unsigned short)((lane << 6) | (unsigned)j);
                qt += (unsigned)__popcll(rowmask);
            }
            const unsigned nb = qt - qh < 64u ? qt - qh : 64u;
            if (nb == 0u)
                break;
            f3dg_wave_fence();

            // ---- one batch: lane q takes pair q of the ring
            const unsigned kk = (unsigned)sK[(qh + lane) & 127u];
            const bool valid = lane < nb;
            const unsigned k = valid ? (unsigned)kk : (unsigned)__builtin_amdgcn_readfirstlane((int)kk);      // (lanes beyond the batch repeat pair 0, inactive)
            const unsigned own = (k >> 6) & 63u;
            const int j = (int)(k & 63u);
            // the runs of the batch: consecutive pairs of one entry (a window slot appears in one run only). A lane's distance to the first
            // lane of its run is what the segmented scans below need
            const int jprev = __builtin_amdgcn_update_dpp(-1, j, 0x138 /* wave_shr:1 */, 0xf, 0xf, false);
            const unsigned long long heads_all = __ballot(valid && j != jprev);
            const unsigned long long upto = heads_all & (~0ull >> (63u - lane));
            const unsigned rr = valid ? lane - (63u - (unsigned)__builtin_clzll(upto | 1ull)) : 0u;
            const int oaddr = (int)(own << 2);
            // the pair's pixel constants, from the lane that owns the pixel
            F3dgBwdPixel px;
            px.ray_x = f3dg_pull(oaddr, ray_x); px.ray_y = f3dg_pull(oaddr, ray_y);
            px.dpx[0] = f3dg_pull(oaddr, w.dpx0); px.dpx[1] = f3dg_pull(oaddr, w.dpx1); px.dpx[2] = f3dg_pull(oaddr, w.dpx2);
            px.dn[0] = f3dg_pull(oaddr, w.dn0); px.dn[1] = f3dg_pull(oaddr, w.dn1); px.dn[2] = f3dg_pull(oaddr, w.dn2);
            px.dL_dmax_depth = f3dg_pull(oaddr, w.dL_dmax_depth); px.dL_dreg = f3dg_pull(oaddr, w.dL_dreg);
            px.final_A = f3dg_pull(oaddr, w.final_A); px.final_D = f3dg_pull(oaddr, w.final_D);
            const float p_TfBg = f3dg_pull(oaddr, TfBg);
            px.max_contributor = __builtin_amdgcn_ds_bpermute(oaddr, w.max_contributor);
            px.pix_x = (float)(qx0 + (own & 7u)); px.pix_y = (float)(qy0 + (own >> 3));
            const uint2 pe = w.entry((unsigned)j);
            const int contributor = (int)pe.x;

            const float4 q2 = sR[2][j];
            const F3dgBwdPair pr = f3dg_bwd_pair_eval(sR[0][j], sR[1][j], q2, px.ray_x, px.ray_y, w.alpha_fast, valid);
            const bool active = pr.live;
            const float alpha = pr.alpha;
            n_pairs += (unsigned)__popcll(__ballot(active));

            // ---- gradient terms only from here: float32 with one reciprocal each, FMA contraction allowed (as render3_bwd_kernel)
            float g[18];
#pragma unroll
            for (int c = 0; c < 18; c++) g[c] = 0.0f;
            {
#pragma clang fp contract(fast)
                const float4 q3 = sR[3][j];
                float4 con = sC[j];
                const float2 xy = make_float2(con.w, sY[j]);
                con.w = q2.z;
                float nn0, nn1, nn2;
                f3dg_bwd_pair_normal(pr, nn0, nn1, nn2);
                const float c0 = q3.x, c1 = q3.y, c2 = q3.z;
                const float u = c0 * px.dpx[0] + c1 * px.dpx[1] + c2 * px.dpx[2] + nn0 * px.dn[0] + nn1 * px.dn[1] + nn2 * px.dn[2];
                const float oma = 1.f - alpha;

                // ---- the recurrence, entry after entry (a pixel has at most one pair per entry, so the lanes of a run never share a
                // state slot; successive runs of the batch do)
                float Tr = 0.0f, A = 0.0f;
                // T is rebuilt back to front as the reference does (backward.cu:803, T = T / (1 - alpha)), with the division taken off the
                // serial chain: one correctly rounded reciprocal per pair up front, a multiply per run (<= 1 ulp from the quotient per layer;
                // C5 8.1 -> 7.8 ms; the gradient tests, incl. the ill-conditioned B2, hold their bars)
                const float inv_oma_ieee = 1.0f / oma;
                unsigned long long heads = heads_all;
                while (heads != 0ull) {
                    const unsigned a0 = (unsigned)__builtin_ctzll(heads);
                    heads &= heads - 1ull;
                    const unsigned b0 = heads != 0ull ? (unsigned)__builtin_ctzll(heads) : nb;
                    if (active && lane >= a0 && lane < b0) {
                        const float4 st = sS[own];
                        Tr = st.x * inv_oma_ieee;
                        A = st.z * st.w + (1.f - st.z) * st.y;
                        sS[own] = make_float4(Tr, A, alpha, u);
                    }
                    f3dg_wave_fence();
                }

                if (active) {
                    const float inv_oma = __builtin_amdgcn_rcpf(oma);      // background term only
                    float dL_dalpha = (u - A) * Tr;
                    dL_dalpha += (-inv_oma) * p_TfBg;
                    f3dg_bwd_pair_partials<false>(g, px, pr, con, xy, w.ddelx_dx, w.ddely_dy, contributor, Tr, dL_dalpha);
                }

                // ---- the 17 partials of an entry summed over its pixels: segmented scans along the entry's run, totals in its last lane
                const SegFlags sf = seg_flags(rr, lane);
                {
                    float v8[8] = { g[0], g[1], g[2], g[3], g[4], g[5], g[6], g[7] };
                    seg_sums(v8, sf);
#pragma unroll
                    for (int c = 0; c < 8; c++) g[c] = v8[c];
                }
                {
                    float v8[8] = { g[8], g[9], g[10], g[11], g[12], g[13], g[14], g[15] };
                    seg_sums(v8, sf);
#pragma unroll
                    for (int c = 0; c < 8; c++) g[8 + c] = v8[c];
                }
                {
                    float v2[2] = { g[16], g[17] };
                    seg_sums(v2, sf);
                    g[16] = v2[0];
                }
                const bool last = valid && (lane + 1u == nb || ((heads_all >> ((lane + 1u) & 63u)) & 1ull) != 0ull);
                // ---- to memory. One lane adding its run's 17 totals is 17 atomic instructions with one address each (measured: three times
                // the write transactions of render3_bwd_kernel, whose four row-end lanes add neighbouring elements in one instruction, and
                // the kernel waits for the atomic units: 28 ms at C5). So the totals of up to twelve runs at a time go through LDS and come back, three runs per instruction, one
                // ELEMENT per lane -- lane 20 r + c holds element c of run r: colour 0..2, mean2D 3..5, opacity 6, view2gaussian 7..16 (the record's float32 and float64 halves) -- and
                // one float32 and one float64 atomic instruction add runs of neighbouring addresses.
                const unsigned nruns = (unsigned)__popcll(heads_all);
                const unsigned ord = __builtin_amdgcn_mbcnt_hi((unsigned)(heads_all >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)heads_all, 0u)) +
                                     ((valid && j != jprev) ? 1u : 0u) - 1u;       // which run of the batch this lane belongs to
                for (unsigned base = 0u; base < nruns; base += F3DG_B5_STAGE) {
                    if (last && ord - base < (unsigned)F3DG_B5_STAGE) {
                        float* o = sOut[ord - base];
                        *reinterpret_cast<float4*>(o) = make_float4(g[0], g[1], g[2], g[3]);
                        *reinterpret_cast<float4*>(o + 4) = make_float4(g[4], g[5], g[6], g[7]);
                        *reinterpret_cast<float4*>(o + 8) = make_float4(g[8], g[9], g[10], g[11]);
                        *reinterpret_cast<float4*>(o + 12) = make_float4(g[12], g[13], g[14], g[15]);
                        *reinterpret_cast<float2*>(o + 16) = make_float2(g[16], __int_as_float((int)pe.y));
                    }
                    f3dg_wave_fence();
                    const unsigned staged = nruns - base < (unsigned)F3DG_B5_STAGE ? nruns - base : (unsigned)F3DG_B5_STAGE;
                    for (unsigned r3 = 0u; r3 < staged; r3 += 3u) {       // three runs per pair of atomic instructions, no waiting in between
                        const unsigned rsel = r3 + el_run;
                        if (el < 17u && el_run < 3u && rsel < staged) {
                            const float v = sOut[rsel][el];
                            const size_t id = (size_t)(unsigned)__float_as_int(sOut[rsel][17]);
                            double* rec = gacc + id * 16;
                            if (el < 7u)
                                unsafeAtomicAdd(reinterpret_cast<float*>(rec + 10) + el, v);
                            else
                                unsafeAtomicAdd(rec + (el - 7u), (double)v);
                        }
                    }
                    f3dg_wave_fence();     // the next round overwrites the slots
                }
            }
            qh += nb;
            f3dg_wave_fence();     // the next compaction overwrites ring slots this batch has read
        } while (todo != 0ull || qt != qh);
        w.retire();
    }
    if (lane == 0 && n_pairs)
        atomicAdd(&a.hdr->bwd_pairs, (unsigned long long)n_pairs);
}


} // namespace

int f3dg_launch_render5_bwd(const F3dgBwdLaunch& a)
{
    F3DG_KLAUNCH((render5_bwd_kernel<F3DG_B5_OCC>), a.quadrants(), dim3(64), 0, a.s, a.k);
    F3DG_HIP_CHECK(hipGetLastError());
    return F3DG_OK;
}
