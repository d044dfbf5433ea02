// f3dg_groupnorm.h -- what the backbone kernels between the convolutions share: the forward (f3dg_groupnorm.hip) and its adjoint
// (f3dg_groupnorm_bwd.hip) load the same 16-byte packets, evaluate the same SiLU, take a thread's channel constants and form the
// pre-activation z with the same two functions (gn_chan, gn_z), and walk a channels-last sample with the same loop (gn_nhwc_walk). One
// definition each: the z the backward recomputes is the forward's by construction, not by two pieces of text that agree.
#pragma once
#include "f3dg_common.h"

namespace {

constexpr int GN_THREADS = 1024;

// bf16 <-> f32 (round to nearest even; NaN kept quiet)
__device__ __forceinline__ float bf16_to_f32(unsigned short h) { return __uint_as_float((unsigned)h << 16); }
__device__ __forceinline__ unsigned short f32_to_bf16(float f)
{
    const unsigned u = __float_as_uint(f);
    if ((u & 0x7FFFFFFFu) > 0x7F800000u) return (unsigned short)((u >> 16) | 0x40u);
    return (unsigned short)((u + 0x7FFFu + ((u >> 16) & 1u)) >> 16);
}

// 16-byte packets: 4 floats or 8 bf16
template <typename T> struct Packet;
template <> struct Packet<float> {
    static constexpr int N = 4;
    float v[4];
    __device__ __forceinline__ void load(const float* p) { const float4 q = *reinterpret_cast<const float4*>(p); v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w; }
    __device__ __forceinline__ void store(float* p) const { *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]); }
};
template <> struct Packet<unsigned short> {
    static constexpr int N = 8;
    float v[8];
    __device__ __forceinline__ void load(const unsigned short* p)
    {
        const uint4 q = *reinterpret_cast<const uint4*>(p);
        const unsigned w[4] = { q.x, q.y, q.z, q.w };
#pragma unroll
        for (int i = 0; i < 4; i++) { v[2 * i] = __uint_as_float(w[i] << 16); v[2 * i + 1] = __uint_as_float(w[i] & 0xFFFF0000u); }
    }
    __device__ __forceinline__ void store(unsigned short* p) const
    {
        unsigned w[4];
#pragma unroll
        for (int i = 0; i < 4; i++) w[i] = (unsigned)f32_to_bf16(v[2 * i]) | ((unsigned)f32_to_bf16(v[2 * i + 1]) << 16);
        *reinterpret_cast<uint4*>(p) = make_uint4(w[0], w[1], w[2], w[3]);
    }
};
// 8 float16 (the fp16 option of the backbone: 10 mantissa bits at the bf16 MFMA rate; T = _Float16)
template <> struct Packet<_Float16> {
    static constexpr int N = 8;
    float v[8];
    __device__ __forceinline__ void load(const _Float16* p)
    {
        const uint4 q = *reinterpret_cast<const uint4*>(p);
        const unsigned w[4] = { q.x, q.y, q.z, q.w };
#pragma unroll
        for (int i = 0; i < 4; i++) {
            v[2 * i] = (float)__builtin_bit_cast(_Float16, (unsigned short)(w[i] & 0xFFFFu));
            v[2 * i + 1] = (float)__builtin_bit_cast(_Float16, (unsigned short)(w[i] >> 16));
        }
    }
    __device__ __forceinline__ void store(_Float16* p) const
    {
        unsigned w[4];
#pragma unroll
        for (int i = 0; i < 4; i++)
            w[i] = (unsigned)__builtin_bit_cast(unsigned short, (_Float16)v[2 * i]) | ((unsigned)__builtin_bit_cast(unsigned short, (_Float16)v[2 * i + 1]) << 16);
        *reinterpret_cast<uint4*>(p) = make_uint4(w[0], w[1], w[2], w[3]);
    }
};
// SiLU. float32 activations: expf and an IEEE division (the backbone's float32 parity bar is 2e-5 of the reference fixture).
// bfloat16 activations: the result is rounded to 8 bits, so hardware exp2 / reciprocal (~1 ulp of float32 each) are invisible and the
// ~30 instructions per element of the accurate form -- which made the kernel VALU-bound -- become 5.
template <typename T> __device__ __forceinline__ float silu_of(float v)
{
    if constexpr (sizeof(T) == 2)
        return v * __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(-1.4426950408889634f * v));
    else
        return v / (1.0f + expf(-v));
}
__device__ __forceinline__ float to_f32(float x) { return x; }
__device__ __forceinline__ float to_f32(unsigned short x) { return bf16_to_f32(x); }
__device__ __forceinline__ void from_f32(float& d, float x) { d = x; }
__device__ __forceinline__ void from_f32(unsigned short& d, float x) { d = f32_to_bf16(x); }
__device__ __forceinline__ float to_f32(_Float16 x) { return (float)x; }
__device__ __forceinline__ void from_f32(_Float16& d, float x) { d = (_Float16)x; }

// pixels per workgroup: 512 where a sample has enough of them to fill the device. Below 128 x 128 pixels a run of 512 left the backbone's 64^2 / 32^2
// layers 8 / 2 workgroups per sample, each thread walking up to 256 pixels one load latency after the other. A function of HW alone: the
// order of the additions, and so the result of a sample, does not depend on the batch it is in.
constexpr int gn_nhwc_pix(int HW) { return HW >= 16384 ? 512 : 64; }
constexpr int GN_NHWC_MAXC = 1024;
constexpr int GN_NHWC_UNROLL = 4;     // independent 16-byte loads in flight per thread

// what every GroupNorm entry point, forward and backward, refuses before any HIP call and before anything is written. PN: values per
// 16-byte packet of the activations; given: every required pointer is there; need / have: the scratch (need = 0: none); p16 / p8: the
// addresses that must lie on the 16- / 8-byte grid, OR-ed together. F3DG_OK with N == 0 means "nothing to do".
inline int gn_check_args(int N, int C, int HW, int groups, int nhwc, int PN, bool given, size_t have, size_t need, uintptr_t p16, uintptr_t p8)
{
    if (N < 0 || C <= 0 || HW <= 0 || groups <= 0 || C % groups != 0 || !given) return F3DG_ERR_BAD_ARG;
    // the channels-last scratch grew when the statistics became atomics-free (a partial pair per workgroup): the caller says how much it
    // handed over, an allocation sized by an older header is refused instead of being written past its end
    if (N > 0 && have < need) return F3DG_ERR_WORKSPACE;
    if (nhwc && (C % PN != 0 || C / PN > 256 || C > GN_NHWC_MAXC)) return F3DG_ERR_BAD_ARG;   // whole 16-byte packets per pixel, one packet column per thread
    if (N == 0) return F3DG_OK;
    if ((p16 & 15u) || (p8 & 7u)) return F3DG_ERR_BAD_ARG;                                     // 16-byte loads / stores, float2 / double words
    return F3DG_OK;
}

// the fixed butterfly over the 64 lanes of a wave: the same association every run, every lane ends with the total
__device__ __forceinline__ double gn_wave_sum(double v)
{
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}

// the channel, counted from the slab's first, of packet / element i of an NCHW slab whose channel planes hold `per` of them. idx32: the
// slab has fewer than 2^31 elements and the division is a 32-bit one (a 64-bit one costs more than the packet's arithmetic)
__device__ __forceinline__ int gn_nchw_chan(size_t i, int per, bool idx32) { return idx32 ? (int)((unsigned)i / (unsigned)per) : (int)(i / per); }

// per-channel constants of the apply stage and of the backward: pre_bias - mean, rstd, weight * rstd, bias. st = (mean, rstd) of the channel's group.
// (x + pre_bias) - mean is taken as x + (pre_bias - mean): rounded once per channel, by as much as x + pre_bias would be per element
struct GnChan { float pbm, rstd, sc, sh; };
__device__ __forceinline__ GnChan gn_chan(int c, float2 st, const float* __restrict__ pre_bias, const float* __restrict__ weight, const float* __restrict__ bias)
{
    GnChan ch;
    ch.pbm = (pre_bias ? pre_bias[c] : 0.0f) - st.x;
    ch.rstd = st.y;
    ch.sc = weight[c] * st.y;
    ch.sh = bias[c];
    return ch;
}
// the pre-activation: the mean comes off before the scale (forming bias - mean * weight * rstd instead rounds at the size of |mean| / std)
__device__ __forceinline__ float gn_z(float x, const GnChan& ch) { return (x + ch.pbm) * ch.sc + ch.sh; }

// ---- channels-last: x is [N][HW][C], a workgroup of 256 takes a run of gn_nhwc_pix(HW) pixels of sample blockIdx.y with ALL channels,
// thread (row, col) owns the 16-byte packet `col` of the pixels row, row + rows, ... of the run (rows = 256 / (C / PN); threads with
// row >= rows idle)
struct GnNhwcRun { int col, row, n, p0, p1; };
template <int PN> __device__ __forceinline__ GnNhwcRun gn_nhwc_run(int C, int HW)
{
    const int ppp = C / PN;                                   // packets per pixel
    GnNhwcRun r;
    r.col = threadIdx.x % ppp; r.row = threadIdx.x / ppp;
    r.n = blockIdx.y;
    r.p0 = blockIdx.x * gn_nhwc_pix(HW);
    r.p1 = min(r.p0 + gn_nhwc_pix(HW), HW);
    return r;
}
// (sample, group)'s constants of the thread's PN channels
template <int PN>
__device__ __forceinline__ void gn_nhwc_chan(GnChan (&ch)[PN], const GnNhwcRun& r, int Cg, int groups, const float* __restrict__ pre_bias,
                                             const float* __restrict__ weight, const float* __restrict__ bias, const float2* __restrict__ stats)
{
#pragma unroll
    for (int k = 0; k < PN; k++) ch[k] = gn_chan(r.col * PN + k, stats[(size_t)r.n * groups + (r.col * PN + k) / Cg], pre_bias, weight, bias);
}
// the walk: GN_NHWC_UNROLL guarded loads of the thread's packet from each of the NIN tensors, then body(q, off) for each loaded pixel in
// order -- q[j] the packet of in[j], off the pixel's element offset from in[j]. in[j] points at the thread's packet of the sample's pixel 0.
template <typename T, int NIN, typename F>
__device__ __forceinline__ void gn_nhwc_walk(const GnNhwcRun& r, int rows, int C, const T* const (&in)[NIN], F body)
{
    for (int p = r.p0 + r.row; p < r.p1; p += rows * GN_NHWC_UNROLL) {
        Packet<T> q[GN_NHWC_UNROLL][NIN];
#pragma unroll
        for (int u = 0; u < GN_NHWC_UNROLL; u++)
            if (p + u * rows < r.p1) {
#pragma unroll
                for (int j = 0; j < NIN; j++) q[u][j].load(in[j] + (size_t)(p + u * rows) * C);
            }
#pragma unroll
        for (int u = 0; u < GN_NHWC_UNROLL; u++)
            if (p + u * rows < r.p1) body(q[u], (size_t)(p + u * rows) * C);
    }
}
// per-channel totals over the rows: every (row, channel) has its own LDS word per plane (rows * C <= 256 * PN), channel c is summed by
// thread c over the rows 0 .. rows - 1 in that order, in A, and handed to out(c, totals). v0, vs...: a thread's PN values of each plane,
// an array per plane. (Kept as the separate arrays the kernels sum into, and the callables here and in the walk taken by value: with the
// planes in one two-dimensional array, or the captures behind a reference, the compiler schedules the moments kernel's sum chains one
// after the other instead of interleaved -- four s_nop per pixel, 8 % of the three launches at 16 x 512 x 32 x 32 (profiles/backbone_refactor.md).)
template <typename A, typename F, typename E, int PN, typename... V>
__device__ __forceinline__ void gn_rows_to_channels(int C, int rows, int row, int col, F out, const E (&v0)[PN], const V&... vs)
{
    constexpr int NP = 1 + sizeof...(V);
    __shared__ E lds[NP][256 * PN];
    if (row < rows) {
        const E* const v[NP] = { v0, vs... };
#pragma unroll
        for (int k = 0; k < PN; k++)
#pragma unroll
            for (int j = 0; j < NP; j++) lds[j][row * C + col * PN + k] = v[j][k];
    }
    __syncthreads();
    for (int c = threadIdx.x; c < C; c += blockDim.x) {
        A t[NP];
#pragma unroll
        for (int j = 0; j < NP; j++) t[j] = (A)0;
        for (int r = 0; r < rows; r++) {
#pragma unroll
            for (int j = 0; j < NP; j++) t[j] += (A)lds[j][r * C + c];
        }
        out(c, t);
    }
}

} // namespace
