// f3dg_frames.hip -- the orbit video's frames, composed on the device (reference visualize.py:403-416: colorize, torch.cat of the five
// panels, torchvision's make_grid, (255 * clip(x, 0, 1)).astype(uint8)). One kernel reads the float32 planes where render_orbit left
// them and writes finished 8-bit HWC frames: 28 B read and 15 B written per dynamic image-pixel, nothing in between. Contract and
// layout: include/f3dg.h (f3dg_compose_frames), DESIGN.md section 3e-ter.
#include "f3dg_common.h"

namespace {

struct PanelTable { f3dg_panel p[F3DG_MAX_PANELS]; };       // by value in the kernel arguments

// A source pointer read from the LDS copy of the panel table is a generic pointer to the compiler: its loads would be flat loads, which
// count on lgkmcnt as well, so the wait for the NEXT pixel's LDS read would wait for this pixel's memory loads. Say that it is global.
#if defined(__HIP_DEVICE_COMPILE__)
typedef const __attribute__((address_space(1))) float* global_floats;
#else
typedef const float* global_floats;
#endif

__device__ __forceinline__ unsigned cv8(float v) { return (unsigned)(255.0f * fminf(fmaxf(v, 0.0f), 1.0f)); }      // pack_frames' rule, NaN -> 0

// A lane produces one 16-byte chunk of the output byte stream (byte b of a frame is channel b % 3 of grid pixel b / 3) and stores it
// as one 16-byte store, the form of pack_frames_host_kernel: a chunk always touches exactly 6 consecutive pixels of the stream
// (ceil((ch + 16) / 3) for ch = 0, 1, 2), which may lie in different panels, cells, rows or frames. Divisions are kept off the pixel:
// a lane divides once for its first (frame, byte in frame) and steps it by the grid stride's (step_f, step_rem) afterwards; a chunk
// decodes its first pixel (three 32-bit divisions, one more for the row) and walks the other five with increments.
// Memory latency is what the kernel waits for, so a chunk issues the loads of all six pixels before it converts the first.
//   x + cellw - pad = colp * cellw + lx: cell column + 1 and the position in the cell; lx >= PW is padding (colp = 0: the left edge);
//   lx = q * W + px: panel and column in it (q, px mean nothing while lx >= PW: they are reset where the next cell begins).
__global__ void __launch_bounds__(F3DG_BLOCK)
compose_frames_kernel(size_t n_bytes, unsigned n_frames, unsigned frame_bytes, size_t step_f, unsigned step_rem, unsigned Hg, unsigned Wg,
                      unsigned H, unsigned W, unsigned PW, unsigned pad, unsigned xmaps, unsigned n_images, int n_panels, PanelTable tab,
                      const unsigned char* __restrict__ lut, const float* __restrict__ ranges, float invalid_val,
                      unsigned char* __restrict__ dst)
{
    __shared__ unsigned s_lut[256];                  // r | g << 8 | b << 16
    __shared__ f3dg_panel s_panel[F3DG_MAX_PANELS];
    __shared__ float s_vmin[F3DG_MAX_PANELS], s_vmax[F3DG_MAX_PANELS];
    static_assert(F3DG_BLOCK == 256, "one thread stages one entry of the 256-entry colour table");
    if (lut) {
        const unsigned t = threadIdx.x;
        s_lut[t] = (unsigned)lut[3 * t] | ((unsigned)lut[3 * t + 1] << 8) | ((unsigned)lut[3 * t + 2] << 16);
    }
    if (threadIdx.x == 0) {
#pragma unroll
        for (int q = 0; q < F3DG_MAX_PANELS; q++) {
            if (q < n_panels) {
                s_panel[q] = tab.p[q];
                if (tab.p[q].kind == F3DG_PANEL_COLORMAP) {
                    s_vmin[q] = ranges[2 * tab.p[q].range_index];
                    s_vmax[q] = ranges[2 * tab.p[q].range_index + 1];
                }
            }
        }
    }
    __syncthreads();

    const unsigned cellh = H + pad, cellw = PW + pad;
    const size_t n_chunks = (n_bytes + 15) / 16, stride = (size_t)gridDim.x * F3DG_BLOCK;
    size_t c = (size_t)blockIdx.x * F3DG_BLOCK + threadIdx.x;
    size_t f0 = (16 * c) / frame_bytes;                                   // frame and byte in it of the chunk's first byte
    size_t rem0 = 16 * c - f0 * frame_bytes;                              // (a frame is < 4 GB: checked on the host)
    for (; c < n_chunks; c += stride) {
        const size_t b0 = 16 * c;
        size_t f = f0;
        const unsigned rem = (unsigned)rem0;
        const unsigned gp = rem / 3u, ch = rem - 3u * gp;
        unsigned y = gp / Wg, x = gp - y * Wg;
        unsigned row = 0u, ly = 0u;
        bool yok;
        auto decode_y = [&]() {
            yok = y >= pad;
            if (yok) {
                const unsigned yy = y - pad;
                row = yy / cellh;
                ly = yy - row * cellh;
                yok = ly < H;                                             // else: the padding rows under a cell
            }
        };
        decode_y();
        const unsigned xs = x + cellw - pad;
        unsigned colp = xs / cellw, lx = xs - colp * cellw, q = lx / W, px = lx - q * W;
        // first the loads of all 6 pixels (up to 18 in flight, nothing waits on them here), then the conversions: a pixel at a
        // time, a lane would sit out one memory latency per pixel
        float v0[6], v1[6], v2[6];
        unsigned meta[6];                                                 // kind | planes == 3 ? 4 : 0 | q << 3; ~0: padding, a cell with no image
#pragma unroll
        for (int i = 0; i < 6; i++) {
            meta[i] = ~0u;
            v0[i] = v1[i] = v2[i] = 0.0f;
            const unsigned k = row * xmaps + colp - 1u;
            if (f < n_frames && yok && lx < PW && k < n_images) {
                const f3dg_panel P = s_panel[q];
                global_floats s = (global_floats)(P.src + (size_t)k * P.image_stride + f * P.frame_stride + (size_t)ly * W + px);
                meta[i] = (unsigned)P.kind | (P.planes == 3 ? 4u : 0u) | (q << 3);
                v0[i] = s[0];
                if (P.planes == 3) { v1[i] = s[P.plane_stride]; v2[i] = s[2 * P.plane_stride]; }
            }
            // the next pixel of the stream
            ++lx;
            if (++px == W) { px = 0u; ++q; }
            if (lx == cellw) { lx = 0u; ++colp; q = 0u; px = 0u; }
            if (++x == Wg) {                                              // next row: back to the left edge (no edge when pad = 0)
                x = 0u;
                colp = pad ? 0u : 1u;
                lx = pad ? cellw - pad : 0u;
                q = pad ? (unsigned)n_panels : 0u;
                px = 0u;
                if (++y == Hg) { y = 0u; f++; }
                decode_y();
            }
        }
        unsigned S[5] = {0u, 0u, 0u, 0u, 0u};                            // the 18 bytes of the chunk's 6 pixels
#pragma unroll
        for (int i = 0; i < 6; i++) {
            unsigned rgb = 0u;
            if (meta[i] != ~0u) {
                const unsigned kind = meta[i] & 3u;
                if (kind == F3DG_PANEL_COLORMAP) {
                    const float d = v0[i], vmin = s_vmin[meta[i] >> 3], vmax = s_vmax[meta[i] >> 3];
                    const float t = vmin != vmax ? (d - vmin) / (vmax - vmin) : d * 0.0f;
                    if (d == invalid_val) rgb = 128u | (128u << 8) | (128u << 16);
                    else if (t != t) rgb = 0u;
                    else if (t < 0.0f) rgb = s_lut[0];
                    else if (t >= 1.0f) rgb = s_lut[255];
                    else rgb = s_lut[(int)(t * 256.0f)];
                } else {
                    float r = v0[i], g = (meta[i] & 4u) ? v1[i] : r, b = (meta[i] & 4u) ? v2[i] : r;
                    if (kind == F3DG_PANEL_SIGNED) { r = (r + 1.0f) / 2.0f; g = (g + 1.0f) / 2.0f; b = (b + 1.0f) / 2.0f; }
                    rgb = cv8(r) | (cv8(g) << 8) | (cv8(b) << 16);
                }
            }
            // pixel i sits at bit 24 * i of the 160-bit stream S
            S[(24 * i) >> 5] |= rgb << ((24 * i) & 31);
            if (((24 * i) & 31) > 8) S[((24 * i) >> 5) + 1] |= rgb >> (32 - ((24 * i) & 31));
        }
        unsigned w[4];
#pragma unroll
        for (int j = 0; j < 4; j++)
            w[j] = (unsigned)(((((unsigned long long)S[j + 1]) << 32) | S[j]) >> (8u * ch));
        if (b0 + 16 <= n_bytes) {
            *reinterpret_cast<uint4*>(dst + b0) = make_uint4(w[0], w[1], w[2], w[3]);
        } else {
            for (int j = 0; b0 + j < n_bytes; j++) dst[b0 + j] = (unsigned char)(w[j >> 2] >> (8 * (j & 3)));
        }
        f0 += step_f;
        rem0 += step_rem;
        if (rem0 >= frame_bytes) { rem0 -= frame_bytes; f0++; }
    }
}

// frame geometry of make_grid(tensor[n_images, 3, H, n_panels * W], nrow, padding): a single image is returned bare
struct Geom { long long pad, xmaps, ymaps, Hg, Wg; };

bool geometry(int n_images, int H, int W, int nrow, int padding, int n_panels, Geom& g)
{
    if (n_images < 1 || H < 1 || W < 1 || nrow < 1 || padding < 0 || n_panels < 1 || n_panels > F3DG_MAX_PANELS) return false;
    g.pad = n_images == 1 ? 0 : padding;
    g.xmaps = nrow < n_images ? nrow : n_images;
    g.ymaps = (n_images + g.xmaps - 1) / g.xmaps;
    g.Hg = g.ymaps * (H + g.pad) + g.pad;
    g.Wg = g.xmaps * ((long long)n_panels * W + g.pad) + g.pad;
    return g.Hg < (1ll << 31) && g.Wg < (1ll << 31) && 3 * g.Hg * g.Wg < (1ll << 32);
}

} // namespace

extern "C" int f3dg_compose_frames_size(int n_frames, int n_images, int H, int W, int nrow, int padding, int n_panels,
                                        int* frame_h, int* frame_w, size_t* n_bytes)
{
    Geom g;
    if (n_frames < 0 || !geometry(n_images, H, W, nrow, padding, n_panels, g)) return F3DG_ERR_BAD_ARG;
    if (frame_h) *frame_h = (int)g.Hg;
    if (frame_w) *frame_w = (int)g.Wg;
    if (n_bytes) *n_bytes = (size_t)n_frames * (size_t)(3 * g.Hg * g.Wg);
    return F3DG_OK;
}

extern "C" int f3dg_compose_frames(void* stream, int n_frames, int n_images, int H, int W, int nrow, int padding, int n_panels,
                                   const f3dg_panel* panels, const unsigned char* lut, const float* ranges, float invalid_val,
                                   unsigned char* dst, int dst_is_host, int max_workgroups)
{
    Geom g;
    if (!dst || !panels || n_frames < 0 || !geometry(n_images, H, W, nrow, padding, n_panels, g)) return F3DG_ERR_BAD_ARG;
    PanelTable tab = {};
    for (int q = 0; q < n_panels; q++) {
        const f3dg_panel& p = panels[q];
        if (!p.src) return F3DG_ERR_BAD_ARG;
        switch (p.kind) {
        case F3DG_PANEL_RGB: if (p.planes != 3) return F3DG_ERR_BAD_ARG; break;
        case F3DG_PANEL_SIGNED: if (p.planes != 3 && p.planes != 1) return F3DG_ERR_BAD_ARG; break;
        case F3DG_PANEL_COLORMAP: if (p.planes != 1 || !lut || !ranges || p.range_index < 0) return F3DG_ERR_BAD_ARG; break;
        default: return F3DG_ERR_BAD_ARG;
        }
        tab.p[q] = p;
    }
    if ((uintptr_t)dst & 15u) return F3DG_ERR_BAD_ARG;
    if (n_frames == 0) return F3DG_OK;
    if (dst_is_host) {                                   // pinned, device-accessible host memory only
        hipPointerAttribute_t at;
        if (hipPointerGetAttributes(&at, dst) != hipSuccess || at.type != hipMemoryTypeHost) {
            (void)hipGetLastError();
            return F3DG_ERR_BAD_ARG;
        }
    }
    const size_t frame_bytes = (size_t)(3 * g.Hg * g.Wg), n_bytes = frame_bytes * (size_t)n_frames;
    const size_t need = ((n_bytes + 15) / 16 + F3DG_BLOCK - 1) / F3DG_BLOCK;
    // a few workgroups move a PCIe-bound stream (f3dg_pack_frames_host); in HBM, eight 4-wave workgroups per CU walk the stream
    size_t grid = max_workgroups > 0 ? (size_t)max_workgroups : (dst_is_host ? 64 : 2048);
    if (grid > need) grid = need;
    const size_t step = 16 * grid * F3DG_BLOCK;          // bytes between a lane's chunks
    F3DG_KLAUNCH(compose_frames_kernel, dim3((unsigned)grid), dim3(F3DG_BLOCK), 0, (hipStream_t)stream, n_bytes, (unsigned)n_frames,
                 (unsigned)frame_bytes, step / frame_bytes, (unsigned)(step % frame_bytes), (unsigned)g.Hg, (unsigned)g.Wg, (unsigned)H, (unsigned)W, (unsigned)(n_panels * W), (unsigned)g.pad,
                 (unsigned)g.xmaps, (unsigned)n_images, n_panels, tab, lut, ranges, invalid_val, dst);
    F3DG_HIP_CHECK(hipGetLastError());
    return F3DG_OK;
}
