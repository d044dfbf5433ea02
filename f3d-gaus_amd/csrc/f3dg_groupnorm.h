// f3dg_groupnorm.h -- what the backbone kernels between the convolutions share: the forward (f3dg_groupnorm.hip) and its adjoint
// (f3dg_groupnorm_bwd.hip) load the same 16-byte packets, evaluate the same SiLU, and cut a channels-last sample into the same pixel
// runs. One definition each, so that the backward recomputes the forward's z to the bit.
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

} // namespace
