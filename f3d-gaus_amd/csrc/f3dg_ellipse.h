// f3dg_ellipse.h -- device helpers around the conservative alpha >= 1/255 ellipse of a (view, Gaussian) record
// (f3dg_preprocess.hip: conservative_ellipse), shared by the compositing kernels (forward and backward) and the shared-ray pass of integrate
// (f3dg_integrate.hip: integrate_pass1_rays_kernel).
#ifndef F3DG_ELLIPSE_H
#define F3DG_ELLIPSE_H
#include "f3dg_common.h"

namespace {

// Phase 1 of render3 (one wave64 per 8x8 pixel quadrant): lane e holds list entry e of the window and evaluates its ellipse at
// pixel P = 8 * row + column of the quadrant (and, recursively, at the following ones); the comparison IS the ballot "which entries
// can reach pixel P", and two v_writelane_b32 hand its halves to lane P -- the lane that blends pixel P -- so that after the 64
// steps every lane holds the 64-bit pass mask of its own pixel. One comparison = one wave ballot (v_cmp writes a lane mask);
// v_writelane_b32 ignores EXEC and takes the SGPR halves as data. gfx950 needs two wait states between a VALU write of an SGPR / VCC
// and a VALU read of it, which the compiler cannot see inside inline assembly: the two FMAs that evaluate the NEXT pixel's ellipse
// value are placed in that gap (s_nop for the last pixel), so the sequence costs no extra issue slots.
template <int P>
__device__ __forceinline__ void quad_ballots(int& lo, int& hi, float Ep, const float (&dxx)[8], const float (&adx)[8],
                                             const float (&dyy)[8], const float (&cdy)[8], float eb)
{
    if constexpr (P < 63) {
        float En;
        asm("v_cmp_ge_f32 vcc, 1.0, %[ep]\n\t"
            "v_fma_f32 %[en], %[eb], %[dy], %[ax]\n\t"
            "v_fma_f32 %[en], %[dx], %[en], %[cy]\n\t"
            "v_writelane_b32 %[lo], vcc_lo, %[l]\n\t"
            "v_writelane_b32 %[hi], vcc_hi, %[l]"
            : [lo] "+v"(lo), [hi] "+v"(hi), [en] "=&v"(En)
            : [ep] "v"(Ep), [eb] "v"(eb), [dy] "v"(dyy[(P + 1) >> 3]), [ax] "v"(adx[(P + 1) & 7]), [dx] "v"(dxx[(P + 1) & 7]),
              [cy] "v"(cdy[(P + 1) >> 3]), [l] "n"(P)
            : "vcc");
        quad_ballots<P + 1>(lo, hi, En, dxx, adx, dyy, cdy, eb);
    } else {
        asm("v_cmp_ge_f32 vcc, 1.0, %[ep]\n\t"
            "s_nop 1\n\t"
            "v_writelane_b32 %[lo], vcc_lo, %[l]\n\t"
            "v_writelane_b32 %[hi], vcc_hi, %[l]\n\t"
            "s_nop 0"
            : [lo] "+v"(lo), [hi] "+v"(hi)
            : [ep] "v"(Ep), [l] "n"(P)
            : "vcc");
    }
}

// Half-window variant (render3's sliding window): 32 entries, lanes e and e + 32 both hold entry e; lane e evaluates the pixels of
// rows 0..3 (pixel P = 8 * row + column), lane e + 32 those of rows 4..7 (pixel P + 32) with its own dyy / cdy, so one comparison
// carries both ballots: vcc_lo = entries reaching pixel P, vcc_hi = entries reaching pixel P + 32, each 32 bits wide.
template <int P>
__device__ __forceinline__ void half_ballots(int& m, float Ep, const float (&dxx)[8], const float (&adx)[8],
                                             const float (&dyy)[4], const float (&cdy)[4], float eb)
{
    if constexpr (P < 31) {
        float En;
        asm("v_cmp_ge_f32 vcc, 1.0, %[ep]\n\t"
            "v_fma_f32 %[en], %[eb], %[dy], %[ax]\n\t"
            "v_fma_f32 %[en], %[dx], %[en], %[cy]\n\t"
            "v_writelane_b32 %[m], vcc_lo, %[l0]\n\t"
            "v_writelane_b32 %[m], vcc_hi, %[l1]"
            : [m] "+v"(m), [en] "=&v"(En)
            : [ep] "v"(Ep), [eb] "v"(eb), [dy] "v"(dyy[(P + 1) >> 3]), [ax] "v"(adx[(P + 1) & 7]), [dx] "v"(dxx[(P + 1) & 7]),
              [cy] "v"(cdy[(P + 1) >> 3]), [l0] "n"(P), [l1] "n"(P + 32)
            : "vcc");
        half_ballots<P + 1>(m, En, dxx, adx, dyy, cdy, eb);
    } else {
        asm("v_cmp_ge_f32 vcc, 1.0, %[ep]\n\t"
            "s_nop 1\n\t"
            "v_writelane_b32 %[m], vcc_lo, %[l0]\n\t"
            "v_writelane_b32 %[m], vcc_hi, %[l1]\n\t"
            "s_nop 0"
            : [m] "+v"(m)
            : [ep] "v"(Ep), [l0] "n"(P), [l1] "n"(P + 32)
            : "vcc");
    }
}

// The same with a wave-level summary: `any` collects the OR of the 64 ballots, i.e. the mask of the window's entries that can reach
// at least one pixel of the quadrant (the compositing backward walks entries in lock-step and skips the others outright).
template <int P>
__device__ __forceinline__ void quad_ballots_any(int& lo, int& hi, unsigned long long& any, float Ep, const float (&dxx)[8],
                                                 const float (&adx)[8], const float (&dyy)[8], const float (&cdy)[8], float eb)
{
    if constexpr (P < 63) {
        float En;
        asm("v_cmp_ge_f32 vcc, 1.0, %[ep]\n\t"
            "v_fma_f32 %[en], %[eb], %[dy], %[ax]\n\t"
            "v_fma_f32 %[en], %[dx], %[en], %[cy]\n\t"
            "v_writelane_b32 %[lo], vcc_lo, %[l]\n\t"
            "v_writelane_b32 %[hi], vcc_hi, %[l]\n\t"
            "s_or_b64 %[any], %[any], vcc"
            : [lo] "+v"(lo), [hi] "+v"(hi), [any] "+s"(any), [en] "=&v"(En)
            : [ep] "v"(Ep), [eb] "v"(eb), [dy] "v"(dyy[(P + 1) >> 3]), [ax] "v"(adx[(P + 1) & 7]), [dx] "v"(dxx[(P + 1) & 7]),
              [cy] "v"(cdy[(P + 1) >> 3]), [l] "n"(P)
            : "vcc", "scc");
        quad_ballots_any<P + 1>(lo, hi, any, En, dxx, adx, dyy, cdy, eb);
    } else {
        asm("v_cmp_ge_f32 vcc, 1.0, %[ep]\n\t"
            "s_nop 1\n\t"
            "v_writelane_b32 %[lo], vcc_lo, %[l]\n\t"
            "v_writelane_b32 %[hi], vcc_hi, %[l]\n\t"
            "s_or_b64 %[any], %[any], vcc"
            : [lo] "+v"(lo), [hi] "+v"(hi), [any] "+s"(any)
            : [ep] "v"(Ep), [l] "n"(P)
            : "vcc", "scc");
    }
}

} // namespace

#endif
