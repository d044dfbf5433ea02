// f3dg_groupnorm.hip -- what the SongUNet backbone of the predictor needs between MIOpen's convolutions:
//   * fused GroupNorm (+ SiLU), NCHW and channels-last, float32, bfloat16 and float16 activations, optionally with the bias of the
//     convolution that produced the input folded in (f3dg_group_norm_silu_forward, reference src/gaussian_predictor.py:250-262 GroupNorm,
//     :318-323 `silu(norm(x))`);
//   * the residual join of a block (f3dg_residual_join_forward, :325-327): second convolution's bias + skip path (+ its bias) + skip_scale.
//
// The backbone calls GroupNorm 78 times per pass, each followed by SiLU in the residual blocks. On PyTorch-ROCm that is three
// bandwidth-bound kernels per call (row moments, scale/shift, silu: five passes over the tensor); the NCHW kernel is ONE:
// a workgroup owns one (sample, group) slab of Cg x H x W contiguous floats, accumulates sum and sum of squares in
// float64, and re-reads the slab (<= 1 MiB: L2-resident) to write silu(weight * (x - mean) * rstd + bias). Two HBM
// passes (one read, one write) instead of five. The channels-last pair of kernels is described where it is defined.
#include "f3dg_common.h"
#include "f3dg_groupnorm.h"

namespace {

// The statistics. One pass gives the variance as E[v^2] - E[v]^2, and in float32 sums that difference loses log2(1 + (mean / std)^2) bits:
// summing v and v^2 themselves, a slab whose mean lies ten standard deviations from zero came out 20x less accurate than torch's float32
// GroupNorm on the device in the channels-last kernels (3x NCHW), thirty 55x (10x), a constant slab 30x (12x) outside the suite's bound
// (tests/test_backbone_kernels_gpu.py). The variance does not see a shift, so the sums are taken of v - K with a pivot K that every thread
// and workgroup of a (sample, group) reads from the same place: the slab's FIRST value (+ its pre_bias). The float sums then hold
// deviations of the size of the spread, the partials are combined in float64 as before, mean = K + E[v - K]; the order of the additions,
// and with it run-to-run bit-identity, is unchanged. The apply stage takes the mean off before it scales --
// (x + (pre_bias - mean)) * (weight * rstd) + bias -- instead of forming bias - mean * weight * rstd, which rounds at the size of
// |mean| / std. (pre_bias - mean is rounded once per channel, by as much as x + pre_bias would be per element; without a pre_bias it is
// exact.) A non-finite K poisons its own slab only, which a non-finite value anywhere in the slab does anyway.
//
// T = float, unsigned short holding bfloat16, or _Float16 (the bf16 / fp16 options of the backbone: statistics and arithmetic stay float32 / float64).
// pre_bias (nullable, [C] float32): added to x on the way in -- the bias of the convolution that produced x, which PyTorch-ROCm would
// otherwise apply as a separate read + write pass behind MIOpen's kernel (108 such passes per backbone pass, profiles/r04_final/unet.md).
template <typename T>
__global__ void __launch_bounds__(GN_THREADS)
group_norm_silu_kernel(int C, int HW, int groups, const T* __restrict__ x, const float* __restrict__ pre_bias, const float* __restrict__ weight,
                       const float* __restrict__ bias, float eps, int apply_silu, T* __restrict__ y, float2* __restrict__ stats_out)
{
    constexpr int PN = Packet<T>::N;
    const int g = blockIdx.x % groups;
    const int n = blockIdx.x / groups;
    const int Cg = C / groups;
    const size_t slab = (size_t)Cg * HW;
    const T* xs = x + ((size_t)n * C + (size_t)g * Cg) * HW;
    T* ys = y + ((size_t)n * C + (size_t)g * Cg) * HW;

    // ---- moments of v - K, K = the slab's first value: float partial sums per thread over short runs, folded into float64
    const float K = to_f32(xs[0]) + (pre_bias ? pre_bias[g * Cg] : 0.0f);
    double s1 = 0.0, s2 = 0.0;
    const bool vec = HW % PN == 0;                                // true for every layer of the backbone at 256^2 / 32^2
    const size_t np = vec ? slab / PN : 0;
    const int hwp = vec ? HW / PN : 1;
    const bool idx32 = slab <= 0x7FFFFFFFu;                       // the channel of a packet / element by a 32-bit division (a 64-bit one costs more than the packet's arithmetic)
    for (size_t i = threadIdx.x; i < np; i += GN_THREADS) {
        Packet<T> p;
        p.load(xs + i * PN);
        const float pb = pre_bias ? pre_bias[g * Cg + gn_nchw_chan(i, hwp, idx32)] : 0.0f;
        float a = 0.0f, b = 0.0f;
#pragma unroll
        for (int k = 0; k < PN; k++) { const float v = (p.v[k] + pb) - K; a += v; b = __builtin_fmaf(v, v, b); }      // (the fused multiply-add pays for the subtraction)
        s1 += (double)a;
        s2 += (double)b;
    }
    for (size_t i = np * PN + threadIdx.x; i < slab; i += GN_THREADS) {
        const float v = (to_f32(xs[i]) + (pre_bias ? pre_bias[g * Cg + gn_nchw_chan(i, HW, idx32)] : 0.0f)) - K;
        s1 += v; s2 += (double)(v * v);
    }
    s1 = gn_wave_sum(s1);
    s2 = gn_wave_sum(s2);
    __shared__ double w1[GN_THREADS / 64], w2[GN_THREADS / 64];
    __shared__ float s_mean, s_rstd;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) { w1[wave] = s1; w2[wave] = s2; }
    __syncthreads();
    if (threadIdx.x == 0) {
        double a = 0.0, b = 0.0;
        for (int w = 0; w < GN_THREADS / 64; w++) { a += w1[w]; b += w2[w]; }
        const double d = a / (double)slab;                        // mean - K
        double var = b / (double)slab - d * d;
        if (var < 0.0) var = 0.0;
        s_mean = (float)((double)K + d);
        s_rstd = (float)(1.0 / sqrt(var + (double)eps));
        if (stats_out) stats_out[blockIdx.x] = make_float2(s_mean, s_rstd);       // [n][g]: what the backward (f3dg_groupnorm_bwd.hip) normalises with
    }
    __syncthreads();
    const float2 st = make_float2(s_mean, s_rstd);

    // ---- normalise, affine, (silu): the slab is re-read from L2
    if (vec) {
        for (size_t i = threadIdx.x; i < np; i += GN_THREADS) {
            const GnChan ch = gn_chan(g * Cg + gn_nchw_chan(i, hwp, idx32), st, pre_bias, weight, bias);
            Packet<T> p;
            p.load(xs + i * PN);
#pragma unroll
            for (int k = 0; k < PN; k++) {
                float v = gn_z(p.v[k], ch);
                if (apply_silu) v = silu_of<T>(v);
                p.v[k] = v;
            }
            p.store(ys + i * PN);
        }
    } else {
        for (size_t i = threadIdx.x; i < slab; i += GN_THREADS) {
            float v = gn_z(to_f32(xs[i]), gn_chan(g * Cg + gn_nchw_chan(i, HW, idx32), st, pre_bias, weight, bias));
            if (apply_silu) v = silu_of<T>(v);
            from_f32(ys[i], v);
        }
    }
}

// ---- channels-last (NHWC) variant ---------------------------------------------------------------------------------------------------
// MIOpen's fastest convolutions on gfx950 are its NHWC kernels; handed NCHW tensors it wraps them in batched_transpose launches
// (15 % of a bf16 pass of the backbone, profiles/r04_final/unet.md), and torch's GroupNorm converts a channels_last tensor back, so the
// layout only pays if GroupNorm keeps it. x is [N][HW][C]: a group's Cg channels are 8..64 bytes of every pixel's C-vector, so a
// workgroup takes a run of pixels with ALL channels (whole lines), and the moments of a (sample, group) are summed across workgroups:
//   gn_nhwc_moments_kernel: the walk of f3dg_groupnorm.h (thread (row, col) owns the 16-byte packet `col` of the pixels row, row + rows,
//       ...): float sums per channel over at most gn_nhwc_pix(HW) / rows pixels, per-channel totals over the rows in LDS, per-group totals
//       in float64 written to partial[n][g][block] = (sum, sum of squares); gn_nhwc_finish_kernel adds the blocks in order -> (mean, rstd)
//       per (sample, group);
//   gn_nhwc_apply_kernel: the same walk; the constants of the thread's PN channels once, then one pass: silu(gn_z(x)).
// Two reads (the second from L2 / MALL) and one write, as the NCHW kernel.

// the pivot of (sample n, group g): the first value of the slab, as the moments and the finish kernel both read it
template <typename T>
__device__ __forceinline__ float gn_nhwc_pivot(const T* __restrict__ x, const float* __restrict__ pre_bias, int n, int C, int HW, int Cg, int g)
{
    return to_f32(x[((size_t)n * HW) * C + (size_t)g * Cg]) + (pre_bias ? pre_bias[g * Cg] : 0.0f);
}

template <typename T, int KP>
__global__ void __launch_bounds__(256)
gn_nhwc_moments_kernel(int C, int HW, int groups, int rows, const T* __restrict__ x, const float* __restrict__ pre_bias, double* __restrict__ moments)
{
    constexpr int PN = Packet<T>::N;
    const GnNhwcRun r = gn_nhwc_run<PN>(C, HW);
    const int col = r.col, row = r.row, n = r.n;
    const int Cg = C / groups;
    float a[PN], b[PN], pb[PN];
#pragma unroll
    for (int k = 0; k < PN; k++) { a[k] = 0.0f; b[k] = 0.0f; pb[k] = (pre_bias && row < rows) ? pre_bias[col * PN + k] : 0.0f; }
    if (row < rows) {
        // K = gn_nhwc_pivot of each of the thread's channels' group (pixel 0 of the sample, first channel of the group): the sums are of (x + pb) - K
        // KP pivots per packet: 1 (the packet inside one group, Cg a multiple of PN), 2 (two whole groups: Cg = 4 and 8-wide packets, the
        // 16-bit backbone's 128-channel layers) or PN (any other Cg: a pivot is loaded where the packet enters a group). Chosen by the
        // launch: a thread has as few as 8 trips of the walk to spread this set-up over
        float K[KP];
        if constexpr (KP < PN) {
            const int g = KP == 1 ? (col * PN) / Cg : col * KP;
#pragma unroll
            for (int j = 0; j < KP; j++) K[j] = gn_nhwc_pivot(x, pre_bias, n, C, HW, Cg, g + j);
        } else {
            int g = (col * PN) / Cg, rr = col * PN - g * Cg;
            float Kg = gn_nhwc_pivot(x, pre_bias, n, C, HW, Cg, g);
#pragma unroll
            for (int k = 0; k < PN; k++) {
                K[k] = Kg;
                if (++rr == Cg && k + 1 < PN) { rr = 0; g++; Kg = gn_nhwc_pivot(x, pre_bias, n, C, HW, Cg, g); }
            }
        }
        const T* const in[1] = { x + ((size_t)n * HW) * C + (size_t)col * PN };
        gn_nhwc_walk(r, rows, C, in, [&](const Packet<T> (&q)[1], size_t) {
#pragma unroll
            for (int k = 0; k < PN; k++) { const float v = (q[0].v[k] + pb[k]) - K[k * KP / PN]; a[k] += v; b[k] = __builtin_fmaf(v, v, b[k]); }
        });
    }
    __shared__ float ca[GN_NHWC_MAXC], cb[GN_NHWC_MAXC];
    gn_rows_to_channels<float>(C, rows, row, col, [&](int c, const float (&t)[2]) { ca[c] = t[0]; cb[c] = t[1]; }, a, b);
    __syncthreads();
    // per-group totals in float64, one (sum, sum of squares) pair per WORKGROUP: partial[n][g][block]. No atomics -- the second stage
    // (gn_nhwc_finish_kernel) adds a sample's blocks up in block order, so the statistics, and with them the whole backbone pass, are
    // bit-reproducible from run to run (until round 5 the blocks added into 8 atomic slots in arrival order)
    for (int g = threadIdx.x; g < groups; g += blockDim.x) {
        double s1 = 0.0, s2 = 0.0;
        for (int c = g * Cg; c < (g + 1) * Cg; c++) { s1 += (double)ca[c]; s2 += (double)cb[c]; }
        double* part = moments + 2 * (((size_t)n * groups + g) * gridDim.x + blockIdx.x);       // [n][g][block]: the second stage reads a (sample, group)'s blocks contiguously
        part[0] = s1;
        part[1] = s2;
    }
}

// second stage: ONE WAVE per (sample, group) adds its nb partial pairs -- lane l takes blocks l, l + 64, ... in order, then a fixed
// butterfly over the lanes: the same association every run -- and leaves mean and 1 / sqrt(var + eps) as two floats behind the partials
// (stats[n][g]): the apply kernel's threads read them instead of each recomputing them in float64. (One THREAD per pair, the first
// version, walked 128 strided pairs serially: 12 us per launch, 78 launches per pass.)
template <typename T>
__global__ void __launch_bounds__(256)
gn_nhwc_finish_kernel(int N, int C, int HW, int groups, int nb, double cnt, float eps, const T* __restrict__ x, const float* __restrict__ pre_bias,
                      const double* __restrict__ partial, float2* __restrict__ stats)
{
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= N * groups) return;
    const int lane = threadIdx.x & 63;
    const int n = i / groups, g = i % groups;
    const float K = gn_nhwc_pivot(x, pre_bias, n, C, HW, C / groups, g);      // (loaded while the partials are on their way)
    double m1 = 0.0, m2 = 0.0;
    for (int b = lane; b < nb; b += 64) {
        const double* p = partial + 2 * (((size_t)n * groups + g) * nb + b);
        m1 += p[0]; m2 += p[1];
    }
    m1 = gn_wave_sum(m1);
    m2 = gn_wave_sum(m2);
    if (lane == 0) {
        const double d = m1 / cnt;                                // mean - K: the partials are sums of v - K
        double var = m2 / cnt - d * d;
        if (var < 0.0) var = 0.0;
        stats[i] = make_float2((float)((double)K + d), (float)(1.0 / sqrt(var + (double)eps)));
    }
}

template <typename T>
__global__ void __launch_bounds__(256)
gn_nhwc_apply_kernel(int C, int HW, int groups, int rows, const T* __restrict__ x, const float* __restrict__ pre_bias, const float2* __restrict__ stats,
                     const float* __restrict__ weight, const float* __restrict__ bias, int apply_silu, T* __restrict__ y)
{
    constexpr int PN = Packet<T>::N;
    const GnNhwcRun r = gn_nhwc_run<PN>(C, HW);
    if (r.row >= rows) return;
    GnChan ch[PN];
    gn_nhwc_chan(ch, r, C / groups, groups, pre_bias, weight, bias, stats);
    const size_t base = ((size_t)r.n * HW) * C + (size_t)r.col * PN;
    const T* const in[1] = { x + base };
    gn_nhwc_walk(r, rows, C, in, [&](Packet<T> (&q)[1], size_t off) {
#pragma unroll
        for (int k = 0; k < PN; k++) {
            float v = gn_z(q[0].v[k], ch[k]);
            if (apply_silu) v = silu_of<T>(v);
            q[0].v[k] = v;
        }
        q[0].store(y + base + off);
    });
}

template <typename T>
int launch_gn(void* stream, int nhwc, int N, int C, int HW, int groups, const void* x_, const float* pre_bias, const float* weight, const float* bias,
              float eps, int apply_silu, void* y_, float2* stats_out, void* scratch, size_t scratch_bytes)
{
    constexpr int PN = Packet<T>::N;
    const T* x = static_cast<const T*>(x_);
    T* y = static_cast<T*>(y_);
    const int rc = gn_check_args(N, C, HW, groups, nhwc, PN, x && weight && bias && y && (!nhwc || scratch), scratch_bytes,
                                 nhwc ? f3dg_group_norm_nhwc_scratch_bytes(N, HW, groups) : 0, (uintptr_t)x | (uintptr_t)y, 0);
    if (rc != F3DG_OK || N == 0) return rc;
    hipStream_t s = (hipStream_t)stream;
    if (!nhwc) {
        F3DG_KLAUNCH(group_norm_silu_kernel<T>, dim3((unsigned)(N * groups)), dim3(GN_THREADS), 0, s, C, HW, groups, x, pre_bias, weight, bias, eps,
                     apply_silu, y, stats_out);
        F3DG_HIP_CHECK(hipGetLastError());
        return F3DG_OK;
    }
    double* moments = static_cast<double*>(scratch);
    const int ppp = C / PN, rows = 256 / ppp;
    const int nb = (HW + gn_nhwc_pix(HW) - 1) / gn_nhwc_pix(HW);
    // (mean, rstd) per (sample, group): behind the partials, or where the caller keeps them for the backward
    float2* stats = stats_out ? stats_out : reinterpret_cast<float2*>(moments + 2 * (size_t)N * nb * groups);
    const dim3 grid((unsigned)nb, (unsigned)N);
    const int Cg = C / groups;
    if (Cg % PN == 0)
        F3DG_KLAUNCH((gn_nhwc_moments_kernel<T, 1>), grid, dim3(256), 0, s, C, HW, groups, rows, x, pre_bias, moments);
    else if (2 * Cg == PN)
        F3DG_KLAUNCH((gn_nhwc_moments_kernel<T, 2>), grid, dim3(256), 0, s, C, HW, groups, rows, x, pre_bias, moments);
    else
        F3DG_KLAUNCH((gn_nhwc_moments_kernel<T, PN>), grid, dim3(256), 0, s, C, HW, groups, rows, x, pre_bias, moments);
    F3DG_KLAUNCH(gn_nhwc_finish_kernel<T>, dim3((unsigned)((N * groups + 3) / 4)), dim3(256), 0, s, N, C, HW, groups, nb, (double)(C / groups) * (double)HW,
                 eps, x, pre_bias, moments, stats);
    F3DG_KLAUNCH(gn_nhwc_apply_kernel<T>, grid, dim3(256), 0, s, C, HW, groups, rows, x, pre_bias, stats, weight, bias, apply_silu, y);
    F3DG_HIP_CHECK(hipGetLastError());
    return F3DG_OK;
}

// ---- the residual join of a block -------------------------------------------------------------------------------------------------
// y = ((a + bias_a[c]) + (b + bias_b[c])) * scale, the three elementwise passes behind a residual block's second convolution
// (reference src/gaussian_predictor.py:325-327: `x = conv1(...)` [+ bias], `x = x + skip(orig)` [+ bias], `x = x * skip_scale`) in one:
// same float32 operations in the same order, rounded to the activation type once. nhwc = 0: [N][C][HW], channel = (i / HW) % C;
// nhwc = 1: [N][HW][C], channel = i % C. Either bias may be null. y may be a or b.
template <typename T>
__global__ void __launch_bounds__(256)
residual_join_kernel(size_t n_packets, int C, int HW, int nhwc, int packet_in_channel, const T* __restrict__ a, const float* __restrict__ bias_a,
                     const T* __restrict__ b, const float* __restrict__ bias_b, float scale, T* __restrict__ y)
{
    constexpr int PN = Packet<T>::N;
    const size_t first = (size_t)blockIdx.x * 256 + threadIdx.x, stride = (size_t)gridDim.x * 256;
    if (nhwc) {
        // channels-last: C is a multiple of PN and the launch makes the stride a multiple of the packets per pixel, so a thread meets the
        // same PN channels in every iteration: its 2 PN bias values are loaded once (as 2 PN loads per packet they were what bounded
        // the first version of this kernel: 19 memory instructions per packet of which 3 moved data)
        const int c0 = (int)((first * PN) % (size_t)C);
        float ba[PN], bb[PN];
#pragma unroll
        for (int k = 0; k < PN; k++) { ba[k] = bias_a ? bias_a[c0 + k] : 0.0f; bb[k] = bias_b ? bias_b[c0 + k] : 0.0f; }
        for (size_t i = first; i < n_packets; i += stride) {
            Packet<T> pa, pb;
            pa.load(a + i * PN);
            pb.load(b + i * PN);
#pragma unroll
            for (int k = 0; k < PN; k++) {
                const float va = bias_a ? pa.v[k] + ba[k] : pa.v[k];
                const float vb = bias_b ? pb.v[k] + bb[k] : pb.v[k];
                pa.v[k] = (va + vb) * scale;
            }
            pa.store(y + i * PN);
        }
        return;
    }
    for (size_t i = first; i < n_packets; i += stride) {
        Packet<T> pa, pb;
        pa.load(a + i * PN);
        pb.load(b + i * PN);
        const size_t e0 = i * PN;
        // NCHW with HW a multiple of PN: a packet stays inside a channel plane; otherwise element by element
        const int c0 = (int)((e0 / (size_t)HW) % (size_t)C);
        const float ba0 = bias_a ? bias_a[c0] : 0.0f, bb0 = bias_b ? bias_b[c0] : 0.0f;
#pragma unroll
        for (int k = 0; k < PN; k++) {
            float ba = ba0, bb = bb0;
            if (!packet_in_channel) {
                const int c = (int)(((e0 + k) / (size_t)HW) % (size_t)C);
                ba = bias_a ? bias_a[c] : 0.0f; bb = bias_b ? bias_b[c] : 0.0f;
            }
            const float va = bias_a ? pa.v[k] + ba : pa.v[k];
            const float vb = bias_b ? pb.v[k] + bb : pb.v[k];
            pa.v[k] = (va + vb) * scale;
        }
        pa.store(y + i * PN);
    }
}

template <typename T>
int launch_join(void* stream, int nhwc, int N, int C, int HW, const void* a_, const float* bias_a, const void* b_, const float* bias_b, float scale, void* y_)
{
    constexpr int PN = Packet<T>::N;
    const T* a = static_cast<const T*>(a_);
    const T* b = static_cast<const T*>(b_);
    T* y = static_cast<T*>(y_);
    if (N < 0 || C <= 0 || HW <= 0 || !a || !b || !y) return F3DG_ERR_BAD_ARG;
    const size_t total = (size_t)N * C * HW;
    if (total == 0) return F3DG_OK;
    if (total % PN != 0 || (((uintptr_t)a | (uintptr_t)b | (uintptr_t)y) & 15u)) return F3DG_ERR_BAD_ARG;
    if (nhwc && C % PN != 0) return F3DG_ERR_BAD_ARG;
    const size_t np = total / PN;
    // channels-last: blocks * 256 must be a multiple of the packets per pixel (C / PN), which the kernel relies on
    unsigned blocks = (unsigned)((np + 255) / 256 < 16383 ? (np + 255) / 256 : 16383);
    if (nhwc) {
        const unsigned ppp = (unsigned)(C / PN);
        unsigned m = ppp;                       // smallest block count whose 256-fold is a multiple of ppp: ppp / gcd(ppp, 256)
        for (unsigned t = 256; t > 1 && (m % 2u) == 0; t >>= 1) m >>= 1;
        blocks = ((blocks + m - 1) / m) * m;
    }
    F3DG_KLAUNCH(residual_join_kernel<T>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, np, C, HW, nhwc, HW % PN == 0 ? 1 : 0, a, bias_a, b, bias_b, scale, y);
    F3DG_HIP_CHECK(hipGetLastError());
    return F3DG_OK;
}

} // namespace

// bytes of the scratch of the channels-last GroupNorm: the workgroups' partial sums + the (mean, rstd) pairs
extern "C" size_t f3dg_group_norm_nhwc_scratch_bytes(int N, int HW, int groups)
{
    if (N <= 0 || HW <= 0 || groups <= 0) return 0;
    const size_t nb = (size_t)(HW + gn_nhwc_pix(HW) - 1) / gn_nhwc_pix(HW);
    return sizeof(double) * 2 * (size_t)N * nb * groups + sizeof(float2) * (size_t)N * groups;
}

// 16-bit activations travel as unsigned short (bfloat16) or _Float16
static int gn_forward(void* stream, int dtype, int nhwc, int N, int C, int HW, int groups, const void* x, const float* pre_bias, const float* weight,
                      const float* bias, float eps, int apply_silu, void* y, float* stats, void* scratch, size_t scratch_bytes)
{
    if (dtype < F3DG_F32 || dtype > F3DG_F16 || ((uintptr_t)stats & 7u)) return F3DG_ERR_BAD_ARG;
    const auto launch = dtype == F3DG_F32 ? launch_gn<float> : dtype == F3DG_BF16 ? launch_gn<unsigned short> : launch_gn<_Float16>;
    return launch(stream, nhwc, N, C, HW, groups, x, pre_bias, weight, bias, eps, apply_silu, y, reinterpret_cast<float2*>(stats), scratch, scratch_bytes);
}

extern "C" int f3dg_group_norm_silu_forward(void* stream, int dtype, int nhwc, int N, int C, int HW, int groups, const void* x, const float* pre_bias,
                                            const float* weight, const float* bias, float eps, int apply_silu, void* y, float* stats, void* scratch,
                                            size_t scratch_bytes)
{
    // this entry point keeps the statistics of a float32 call only, as it always has; f3dg_group_norm_silu_forward_stats keeps them in every type
    if (stats && dtype != F3DG_F32) return F3DG_ERR_BAD_ARG;
    return gn_forward(stream, dtype, nhwc, N, C, HW, groups, x, pre_bias, weight, bias, eps, apply_silu, y, stats, scratch, scratch_bytes);
}

// the same launch with the (mean, rstd) pairs kept for f3dg_group_norm_silu_backward_dtype, in every type: the templated kernels hand
// stats_out through, y is the plain forward's to the bit
extern "C" int f3dg_group_norm_silu_forward_stats(void* stream, int dtype, int nhwc, int N, int C, int HW, int groups, const void* x, const float* pre_bias,
                                                  const float* weight, const float* bias, float eps, int apply_silu, void* y, float* stats, void* scratch,
                                                  size_t scratch_bytes)
{
    if (!stats) return F3DG_ERR_BAD_ARG;
    return gn_forward(stream, dtype, nhwc, N, C, HW, groups, x, pre_bias, weight, bias, eps, apply_silu, y, stats, scratch, scratch_bytes);
}

extern "C" int f3dg_residual_join_forward(void* stream, int dtype, int nhwc, int N, int C, int HW, const void* a, const float* bias_a, const void* b,
                                          const float* bias_b, float scale, void* y)
{
    if (dtype < F3DG_F32 || dtype > F3DG_F16) return F3DG_ERR_BAD_ARG;
    const auto launch = dtype == F3DG_F32 ? launch_join<float> : dtype == F3DG_BF16 ? launch_join<unsigned short> : launch_join<_Float16>;
    return launch(stream, nhwc, N, C, HW, a, bias_a, b, bias_b, scale, y);
}
