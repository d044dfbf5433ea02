// f3dg_groupnorm_bwd.hip -- the adjoints of f3dg_groupnorm.hip, float32, bfloat16 and float16 activations, both layouts: what training
// through the backbone needs between MIOpen's convolutions (f3dg_group_norm_silu_backward[_dtype], f3dg_residual_join_backward[_dtype]).
//
// GroupNorm (+ SiLU), recomputed from x: with v = x + pre_bias, xh = (v - mean) * rstd, z = weight * xh + bias, m = Cg * HW,
//   dz = dy * s * (1 + z * (1 - s)), s = sigmoid(z)                 (dz = dy without SiLU)
//   A[n][c] = sum_hw dz,  B[n][c] = sum_hw dz * xh,  X[n][c] = sum_hw xh
//   s1[n][g] = sum_c weight[c] A / m,  s2[n][g] = sum_c weight[c] B / m
//   dx = rstd * (dz * weight - s1 - xh * s2)
//   dweight[c] = sum_n B,  dbias[c] = sum_n A,  dpre_bias[c] = sum_{n, hw} dx = sum_n rstd * (weight[c] A - HW s1 - s2 X)
// (mean, rstd) are the forward's own, kept by f3dg_group_norm_silu_forward; z is formed by the forward's own function from the forward's
// own constants (gn_z, gn_chan of f3dg_groupnorm.h) and the sigmoid with the forward's expf and IEEE division. Every sum is taken in
// float32 over short runs (a packet in NCHW, a thread's pixels of a run channels-last, as the forward's moments) and combined in float64
// in a fixed order: no floating-point atomics anywhere, the gradients are bit-identical from run to run.
// Nothing but x is needed from the forward: neither its output nor the normalised pre-activation is kept.
//
// T = float, unsigned short holding bfloat16, or _Float16, as in the forward: x, dy and dx are T (16-byte packets of 4 or 8 values), the
// parameters, the statistics and every parameter gradient float32. A 16-bit value is widened exactly on the way in, all arithmetic and
// all sums are those of the float32 kernel, and dx is rounded to T once on the way out (from_f32: to nearest even, an fp16 result
// beyond the type's range becomes +-Inf, which is how a loss scaler sees an overflow). Nothing is rounded before it enters a sum.
#include "f3dg_common.h"
#include "f3dg_groupnorm.h"

namespace {

// dz and xh of one element
__device__ __forceinline__ void gn_bwd_elem(float x, float dy, const GnChan& ch, int apply_silu, float& dz, float& xh)
{
    xh = (x + ch.pbm) * ch.rstd;
    dz = dy;
    if (apply_silu) {
        const float z = gn_z(x, ch);
        const float s = 1.0f / (1.0f + expf(-z));
        dz = dy * (s * (1.0f + z * (1.0f - s)));
    }
}

// scratch of a call, in doubles: nc [N][C][3] = (A, B, X); sg [N][groups][2] = (s1, s2); channels-last only: part [N][nb][3][C]
struct GnBwdScratch {
    double* nc;
    double* sg;
    double* part;
};

// ---- NCHW: one workgroup per (sample, group) slab -------------------------------------------------------------------------------------
// Stage 1 walks the slab channel by channel (a channel's HW values are contiguous): float sums per packet, float64 per thread, a fixed
// butterfly per wave, the 16 waves added in order by thread 0, which also carries s1 and s2. Stage 2 re-reads x and dy and writes dx. The
// re-read comes from L2 only where the two slabs fit beside those of the XCD's other workgroups: at 256^2 (2 x 1 MiB per slab) a counter
// pass shows both reads leaving the L2, 20 B per element in all, as the channels-last kernels move (profiles/backbone_train.md).
template <typename T>
__global__ void __launch_bounds__(GN_THREADS)
gn_bwd_nchw_kernel(int C, int HW, int groups, const T* __restrict__ x, const float* __restrict__ pre_bias, const float* __restrict__ weight,
                   const float* __restrict__ bias, const float2* __restrict__ stats, int apply_silu, const T* __restrict__ dy,
                   T* __restrict__ dx, double* __restrict__ nc, double* __restrict__ sg)
{
    constexpr int PN = Packet<T>::N, NW = GN_THREADS / 64;
    const int g = blockIdx.x % groups;
    const int n = blockIdx.x / groups;
    const int Cg = C / groups;
    const float2 st = stats[blockIdx.x];
    const float rstd = st.y;
    const size_t base = ((size_t)n * C + (size_t)g * Cg) * HW;
    const bool vec = HW % PN == 0;                                // every channel plane then starts on a 16-byte boundary
    const int hwp = HW / PN;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    __shared__ double wsum[2][3][NW];                             // two sets, taken in turn: one barrier per channel
    __shared__ float s_s1, s_s2;
    double S1 = 0.0, S2 = 0.0;                                    // (thread 0)
    for (int j = 0; j < Cg; j++) {
        const int c = g * Cg + j;
        const GnChan ch = gn_chan(c, st, pre_bias, weight, bias);
        const float wc = weight[c];
        const T* xs = x + base + (size_t)j * HW;
        const T* ds = dy + base + (size_t)j * HW;
        double a = 0.0, b = 0.0, xx = 0.0;
        if (vec) {
            for (int i = threadIdx.x; i < hwp; i += GN_THREADS) {
                Packet<T> px, pd;
                px.load(xs + (size_t)i * PN);
                pd.load(ds + (size_t)i * PN);
                float fa = 0.0f, fb = 0.0f, fx = 0.0f;
#pragma unroll
                for (int k = 0; k < PN; k++) {
                    float dz, xh;
                    gn_bwd_elem(px.v[k], pd.v[k], ch, apply_silu, dz, xh);
                    fa += dz; fb = __builtin_fmaf(dz, xh, fb); fx += xh;
                }
                a += (double)fa; b += (double)fb; xx += (double)fx;
            }
        } else {
            for (int i = threadIdx.x; i < HW; i += GN_THREADS) {
                float dz, xh;
                gn_bwd_elem(to_f32(xs[i]), to_f32(ds[i]), ch, apply_silu, dz, xh);
                a += (double)dz; b += (double)(dz * xh); xx += (double)xh;
            }
        }
        a = gn_wave_sum(a); b = gn_wave_sum(b); xx = gn_wave_sum(xx);
        const int set = j & 1;
        if (lane == 0) { wsum[set][0][wave] = a; wsum[set][1][wave] = b; wsum[set][2][wave] = xx; }
        __syncthreads();
        if (threadIdx.x == 0) {
            double A = 0.0, B = 0.0, X = 0.0;
            for (int w = 0; w < NW; w++) { A += wsum[set][0][w]; B += wsum[set][1][w]; X += wsum[set][2][w]; }
            double* o = nc + ((size_t)n * C + c) * 3;
            o[0] = A; o[1] = B; o[2] = X;
            S1 += (double)wc * A;
            S2 += (double)wc * B;
        }
    }
    if (threadIdx.x == 0) {
        const double m = (double)Cg * (double)HW;
        sg[(size_t)blockIdx.x * 2] = S1 / m;
        sg[(size_t)blockIdx.x * 2 + 1] = S2 / m;
        s_s1 = (float)(S1 / m);
        s_s2 = (float)(S2 / m);
    }
    if (!dx) return;
    __syncthreads();
    const float s1 = s_s1, s2 = s_s2;
    const size_t slab = (size_t)Cg * HW;
    const bool idx32 = slab <= 0x7FFFFFFFu;
    if (vec) {
        const size_t np = slab / PN;
        for (size_t i = threadIdx.x; i < np; i += GN_THREADS) {
            const int c = g * Cg + gn_nchw_chan(i, hwp, idx32);
            const GnChan ch = gn_chan(c, st, pre_bias, weight, bias);
            const float wc = weight[c];
            Packet<T> px, pd;
            px.load(x + base + i * PN);
            pd.load(dy + base + i * PN);
#pragma unroll
            for (int k = 0; k < PN; k++) {
                float dz, xh;
                gn_bwd_elem(px.v[k], pd.v[k], ch, apply_silu, dz, xh);
                px.v[k] = rstd * ((dz * wc - s1) - xh * s2);
            }
            px.store(dx + base + i * PN);
        }
    } else {
        for (size_t i = threadIdx.x; i < slab; i += GN_THREADS) {
            const int c = g * Cg + gn_nchw_chan(i, HW, idx32);
            const float wc = weight[c];
            float dz, xh;
            gn_bwd_elem(to_f32(x[base + i]), to_f32(dy[base + i]), gn_chan(c, st, pre_bias, weight, bias), apply_silu, dz, xh);
            from_f32(dx[base + i], rstd * ((dz * wc - s1) - xh * s2));
        }
    }
}

// ---- channels-last: the forward's pixel-run mapping -----------------------------------------------------------------------------------
// gn_bwd_nhwc_partial_kernel: thread (row, col) owns the packet `col` of the pixels row, row + rows, ... of its workgroup's run: float
//     sums of dz, dz * xh and xh per channel over at most gn_nhwc_pix(HW) / rows pixels (gn_nhwc_walk), the rows added in float64 ->
//     part[n][block][3][C];
// gn_bwd_nhwc_finish_kernel: ONE WAVE per (sample, group) adds the blocks of each of its channels -- lane l takes blocks l, l + 64, ...
//     in order, then a fixed butterfly -- and leaves (A, B, X) per (n, c) and (s1, s2) per (n, g);
// gn_bwd_nhwc_apply_kernel: the same mapping as the first, one pass: dx.
template <typename T>
__global__ void __launch_bounds__(256)
gn_bwd_nhwc_partial_kernel(int C, int HW, int groups, int rows, const T* __restrict__ x, const float* __restrict__ pre_bias,
                           const float* __restrict__ weight, const float* __restrict__ bias, const float2* __restrict__ stats, int apply_silu,
                           const T* __restrict__ dy, double* __restrict__ part)
{
    constexpr int PN = Packet<T>::N;
    const GnNhwcRun r = gn_nhwc_run<PN>(C, HW);
    float a[PN], b[PN], xx[PN];
#pragma unroll
    for (int k = 0; k < PN; k++) { a[k] = 0.0f; b[k] = 0.0f; xx[k] = 0.0f; }
    if (r.row < rows) {
        GnChan ch[PN];
        gn_nhwc_chan(ch, r, C / groups, groups, pre_bias, weight, bias, stats);
        const size_t base = ((size_t)r.n * HW) * C + (size_t)r.col * PN;
        const T* const in[2] = { x + base, dy + base };
        gn_nhwc_walk(r, rows, C, in, [&](const Packet<T> (&q)[2], size_t) {
#pragma unroll
            for (int k = 0; k < PN; k++) {
                float dz, xh;
                gn_bwd_elem(q[0].v[k], q[1].v[k], ch[k], apply_silu, dz, xh);
                a[k] += dz; b[k] = __builtin_fmaf(dz, xh, b[k]); xx[k] += xh;
            }
        });
    }
    double* o = part + ((size_t)r.n * gridDim.x + blockIdx.x) * 3 * (size_t)C;
    gn_rows_to_channels<double>(C, rows, r.row, r.col, [&](int c, const double (&t)[3]) { o[c] = t[0]; o[C + c] = t[1]; o[2 * C + c] = t[2]; }, a, b, xx);
}

__global__ void __launch_bounds__(256)
gn_bwd_nhwc_finish_kernel(int N, int C, int HW, int groups, int nb, const float* __restrict__ weight, const double* __restrict__ part,
                          double* __restrict__ nc, double* __restrict__ sg)
{
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= N * groups) return;
    const int lane = threadIdx.x & 63;
    const int n = i / groups, g = i % groups, Cg = C / groups;
    double S1 = 0.0, S2 = 0.0;
    for (int j = 0; j < Cg; j++) {
        const int c = g * Cg + j;
        double t[3] = { 0.0, 0.0, 0.0 };
        for (int b = lane; b < nb; b += 64) {
            const double* p = part + ((size_t)n * nb + b) * 3 * (size_t)C + c;
            t[0] += p[0]; t[1] += p[C]; t[2] += p[2 * (size_t)C];
        }
#pragma unroll
        for (int k = 0; k < 3; k++) t[k] = gn_wave_sum(t[k]);
        if (lane == 0) {
            double* o = nc + ((size_t)n * C + c) * 3;
            o[0] = t[0]; o[1] = t[1]; o[2] = t[2];
        }
        const double wc = (double)weight[c];
        S1 += wc * t[0];
        S2 += wc * t[1];
    }
    if (lane == 0) {
        const double m = (double)Cg * (double)HW;
        sg[(size_t)i * 2] = S1 / m;
        sg[(size_t)i * 2 + 1] = S2 / m;
    }
}

template <typename T>
__global__ void __launch_bounds__(256)
gn_bwd_nhwc_apply_kernel(int C, int HW, int groups, int rows, const T* __restrict__ x, const float* __restrict__ pre_bias,
                         const float* __restrict__ weight, const float* __restrict__ bias, const float2* __restrict__ stats, int apply_silu,
                         const T* __restrict__ dy, const double* __restrict__ sg, T* __restrict__ dx)
{
    constexpr int PN = Packet<T>::N;
    const GnNhwcRun r = gn_nhwc_run<PN>(C, HW);
    if (r.row >= rows) return;
    const int Cg = C / groups;
    GnChan ch[PN];
    gn_nhwc_chan(ch, r, Cg, groups, pre_bias, weight, bias, stats);
    float wc[PN], s1[PN], s2[PN];
#pragma unroll
    for (int k = 0; k < PN; k++) {
        const int c = r.col * PN + k;
        const double* s = sg + ((size_t)r.n * groups + c / Cg) * 2;
        wc[k] = weight[c];
        s1[k] = (float)s[0];
        s2[k] = (float)s[1];
    }
    const size_t base = ((size_t)r.n * HW) * C + (size_t)r.col * PN;
    const T* const in[2] = { x + base, dy + base };
    gn_nhwc_walk(r, rows, C, in, [&](Packet<T> (&q)[2], size_t off) {
#pragma unroll
        for (int k = 0; k < PN; k++) {
            float dz, xh;
            gn_bwd_elem(q[0].v[k], q[1].v[k], ch[k], apply_silu, dz, xh);
            q[0].v[k] = ch[k].rstd * ((dz * wc[k] - s1[k]) - xh * s2[k]);
        }
        q[0].store(dx + base + off);
    });
}

// ---- second stage, both layouts: the per-(n, c) sums over n, in order, one thread per channel ------------------------------------------
__global__ void __launch_bounds__(256)
gn_bwd_params_kernel(int N, int C, int HW, int groups, const float* __restrict__ weight, const float2* __restrict__ stats, const double* __restrict__ nc,
                     const double* __restrict__ sg, float* __restrict__ dweight, float* __restrict__ dbias, float* __restrict__ dpre_bias)
{
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= C) return;
    const int g = c / (C / groups);
    const double wc = (double)weight[c];
    double dw = 0.0, db = 0.0, dp = 0.0;
    for (int n = 0; n < N; n++) {
        const double* t = nc + ((size_t)n * C + c) * 3;
        const double* s = sg + ((size_t)n * groups + g) * 2;
        const double A = t[0], B = t[1], X = t[2];
        dw += B;
        db += A;
        dp += (double)stats[(size_t)n * groups + g].y * ((wc * A - (double)HW * s[0]) - s[1] * X);
    }
    if (dweight) dweight[c] = (float)dw;
    if (dbias) dbias[c] = (float)db;
    if (dpre_bias) dpre_bias[c] = (float)dp;
}

size_t gn_bwd_scratch_doubles(int N, int C, int HW, int groups, int nhwc)
{
    const size_t nb = (size_t)(HW + gn_nhwc_pix(HW) - 1) / gn_nhwc_pix(HW);
    return 3 * (size_t)N * C + 2 * (size_t)N * groups + (nhwc ? 3 * (size_t)N * nb * C : 0);
}

// ---- the residual join's adjoint --------------------------------------------------------------------------------------------------
// y = ((a + bias_a) + (b + bias_b)) * scale: da = db = grad_y * scale, written ONCE; dbias_a = dbias_b = its per-channel sum. One pass over
// grad_y: a workgroup writes its piece of grad_y * scale, rounded to T once, and the float64 sum per channel of the float32 products
// themselves -- for T = float what it wrote -- (part[segment][C]); a wave per channel then adds the segments in a fixed order.
//   NCHW: a segment is up to JOIN_BWD_CHUNK consecutive values of one (n, c) plane;
//   channels-last: a segment is a run of JOIN_BWD_PIX pixels of the N * HW, all channels, thread (row, col) as in the GroupNorm kernels.
constexpr int JOIN_BWD_CHUNK = 4096;
constexpr int JOIN_BWD_PIX = 256;

template <typename T>
__global__ void __launch_bounds__(256)
join_bwd_nchw_kernel(int C, int HW, int cpp, int vec, const T* gy, float scale, T* gab, double* __restrict__ part)
{
    constexpr int PN = Packet<T>::N;
    const int c = blockIdx.x % C;
    const int seg = blockIdx.x / C;
    const int n = seg / cpp, k0 = (seg % cpp) * JOIN_BWD_CHUNK;
    const int k1 = min(k0 + JOIN_BWD_CHUNK, HW);
    const size_t base = ((size_t)n * C + c) * HW;
    double s = 0.0;
    if (vec) {                                                    // HW a multiple of the packet: planes and chunks start on 16-byte boundaries
        for (int i = k0 + threadIdx.x * PN; i < k1; i += 256 * PN) {
            Packet<T> p;
            p.load(gy + base + i);
            float f = 0.0f;
#pragma unroll
            for (int k = 0; k < PN; k++) { p.v[k] = p.v[k] * scale; f += p.v[k]; }
            p.store(gab + base + i);
            s += (double)f;
        }
    } else {
        for (int i = k0 + threadIdx.x; i < k1; i += 256) {
            const float v = to_f32(gy[base + i]) * scale;
            from_f32(gab[base + i], v);
            s += (double)v;
        }
    }
    if (!part) return;
    s = gn_wave_sum(s);
    __shared__ double ws[4];
    if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) part[(size_t)seg * C + c] = ((ws[0] + ws[1]) + ws[2]) + ws[3];
}

template <typename T>
__global__ void __launch_bounds__(256)
join_bwd_nhwc_kernel(int C, size_t P, int rows, const T* gy, float scale, T* gab, double* __restrict__ part)
{
    constexpr int PN = Packet<T>::N;
    const int ppp = C / PN;
    const int col = threadIdx.x % ppp, row = threadIdx.x / ppp;
    const size_t p0 = (size_t)blockIdx.x * JOIN_BWD_PIX;
    const size_t p1 = p0 + JOIN_BWD_PIX < P ? p0 + JOIN_BWD_PIX : P;
    double s[PN];
#pragma unroll
    for (int k = 0; k < PN; k++) s[k] = 0.0;
    if (row < rows) {
        for (size_t p = p0 + row; p < p1; p += rows) {
            Packet<T> q;
            q.load(gy + p * C + (size_t)col * PN);
#pragma unroll
            for (int k = 0; k < PN; k++) { q.v[k] = q.v[k] * scale; s[k] += (double)q.v[k]; }
            q.store(gab + p * C + (size_t)col * PN);
        }
    }
    if (!part) return;
    gn_rows_to_channels<double>(C, rows, row, col, [&](int c, const double (&t)[1]) { part[(size_t)blockIdx.x * C + c] = t[0]; }, s);
}

__global__ void __launch_bounds__(256)
join_bwd_finish_kernel(int C, size_t nseg, const double* __restrict__ part, float* __restrict__ gbias)
{
    const int c = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (c >= C) return;
    const int lane = threadIdx.x & 63;
    double t = 0.0;
    for (size_t s = lane; s < nseg; s += 64) t += part[s * C + c];
    t = gn_wave_sum(t);
    if (lane == 0) gbias[c] = (float)t;
}

size_t join_bwd_segments(int N, int HW, int nhwc)
{
    if (nhwc) return ((size_t)N * HW + JOIN_BWD_PIX - 1) / JOIN_BWD_PIX;
    return (size_t)N * ((HW + JOIN_BWD_CHUNK - 1) / JOIN_BWD_CHUNK);
}

template <typename T>
int launch_gn_bwd(void* stream, int N, int C, int HW, int groups, int nhwc, const void* x_, const float* pre_bias, const float* weight, const float* bias,
                  const float* stats, int apply_silu, const void* grad_y_, void* grad_x_, float* grad_weight, float* grad_bias, float* grad_pre_bias,
                  void* scratch, size_t scratch_bytes)
{
    constexpr int PN = Packet<T>::N;
    const T* x = static_cast<const T*>(x_);
    const T* grad_y = static_cast<const T*>(grad_y_);
    T* grad_x = static_cast<T*>(grad_x_);
    const size_t need = (N > 0 && C > 0 && HW > 0 && groups > 0) ? sizeof(double) * gn_bwd_scratch_doubles(N, C, HW, groups, nhwc) : 0;
    const int rc = gn_check_args(N, C, HW, groups, nhwc, PN, x && weight && bias && stats && grad_y && scratch, scratch_bytes, need,
                                 (uintptr_t)x | (uintptr_t)grad_y | (uintptr_t)grad_x, (uintptr_t)stats | (uintptr_t)scratch);
    if (rc != F3DG_OK || N == 0) return rc;
    if ((long long)N * groups > 0x7FFFFFFFll || (nhwc && N > 65535)) return F3DG_ERR_BAD_ARG;
    hipStream_t s = (hipStream_t)stream;
    const float2* st = reinterpret_cast<const float2*>(stats);
    GnBwdScratch w;
    w.nc = static_cast<double*>(scratch);
    w.sg = w.nc + 3 * (size_t)N * C;
    w.part = w.sg + 2 * (size_t)N * groups;
    if (!nhwc) {
        F3DG_KLAUNCH(gn_bwd_nchw_kernel<T>, dim3((unsigned)(N * groups)), dim3(GN_THREADS), 0, s, C, HW, groups, x, pre_bias, weight, bias, st, apply_silu,
                     grad_y, grad_x, w.nc, w.sg);
    } else {
        const int ppp = C / PN, rows = 256 / ppp;
        const int nb = (HW + gn_nhwc_pix(HW) - 1) / gn_nhwc_pix(HW);
        const dim3 grid((unsigned)nb, (unsigned)N);
        F3DG_KLAUNCH(gn_bwd_nhwc_partial_kernel<T>, grid, dim3(256), 0, s, C, HW, groups, rows, x, pre_bias, weight, bias, st, apply_silu, grad_y, w.part);
        F3DG_KLAUNCH(gn_bwd_nhwc_finish_kernel, dim3((unsigned)((N * groups + 3) / 4)), dim3(256), 0, s, N, C, HW, groups, nb, weight, w.part, w.nc, w.sg);
        if (grad_x)
            F3DG_KLAUNCH(gn_bwd_nhwc_apply_kernel<T>, grid, dim3(256), 0, s, C, HW, groups, rows, x, pre_bias, weight, bias, st, apply_silu, grad_y, w.sg, grad_x);
    }
    if (grad_weight || grad_bias || grad_pre_bias)
        F3DG_KLAUNCH(gn_bwd_params_kernel, dim3((unsigned)((C + 255) / 256)), dim3(256), 0, s, N, C, HW, groups, weight, st, w.nc, w.sg, grad_weight,
                     grad_bias, grad_pre_bias);
    F3DG_HIP_CHECK(hipGetLastError());
    return F3DG_OK;
}

template <typename T>
int launch_join_bwd(void* stream, int N, int C, int HW, int nhwc, const void* grad_y_, float scale, void* grad_ab_, float* grad_bias, void* scratch,
                    size_t scratch_bytes)
{
    constexpr int PN = Packet<T>::N;
    const T* grad_y = static_cast<const T*>(grad_y_);
    T* grad_ab = static_cast<T*>(grad_ab_);
    if (N < 0 || C <= 0 || HW <= 0 || !grad_y || !grad_ab) return F3DG_ERR_BAD_ARG;
    const size_t total = (size_t)N * C * HW;
    if (total == 0) return F3DG_OK;
    if (total % PN != 0 || (((uintptr_t)grad_y | (uintptr_t)grad_ab) & 15u)) return F3DG_ERR_BAD_ARG;
    if (nhwc && (C % PN != 0 || C / PN > 256 || C > GN_NHWC_MAXC)) return F3DG_ERR_BAD_ARG;
    const size_t nseg = join_bwd_segments(N, HW, nhwc);
    if (grad_bias) {
        if (!scratch || ((uintptr_t)scratch & 7u)) return F3DG_ERR_BAD_ARG;
        if (scratch_bytes < sizeof(double) * nseg * (size_t)C) return F3DG_ERR_WORKSPACE;
    }
    if (nseg * (nhwc ? 1 : (size_t)C) > 0x7FFFFFFFull) return F3DG_ERR_BAD_ARG;
    hipStream_t s = (hipStream_t)stream;
    double* part = grad_bias ? static_cast<double*>(scratch) : nullptr;
    if (nhwc)
        F3DG_KLAUNCH(join_bwd_nhwc_kernel<T>, dim3((unsigned)nseg), dim3(256), 0, s, C, (size_t)N * HW, 256 / (C / PN), grad_y, scale, grad_ab, part);
    else
        F3DG_KLAUNCH(join_bwd_nchw_kernel<T>, dim3((unsigned)(nseg * C)), dim3(256), 0, s, C, HW, (HW + JOIN_BWD_CHUNK - 1) / JOIN_BWD_CHUNK, HW % PN == 0 ? 1 : 0,
                     grad_y, scale, grad_ab, part);
    if (grad_bias)
        F3DG_KLAUNCH(join_bwd_finish_kernel, dim3((unsigned)((C + 3) / 4)), dim3(256), 0, s, C, nseg, part, grad_bias);
    F3DG_HIP_CHECK(hipGetLastError());
    return F3DG_OK;
}

} // namespace

// (neither scratch depends on the activation type: the partial sums are float64 per channel whatever the packets hold)
extern "C" size_t f3dg_group_norm_silu_backward_scratch_bytes(int N, int C, int HW, int groups, int nhwc)
{
    if (N <= 0 || C <= 0 || HW <= 0 || groups <= 0) return 0;
    return sizeof(double) * gn_bwd_scratch_doubles(N, C, HW, groups, nhwc);
}

extern "C" int f3dg_group_norm_silu_backward_dtype(void* stream, int dtype, int N, int C, int HW, int groups, int nhwc, const void* x, const float* pre_bias,
                                                   const float* weight, const float* bias, const float* stats, int apply_silu, const void* grad_y,
                                                   void* grad_x, float* grad_weight, float* grad_bias, float* grad_pre_bias, void* scratch,
                                                   size_t scratch_bytes)
{
    if (dtype < F3DG_F32 || dtype > F3DG_F16) return F3DG_ERR_BAD_ARG;
    const auto launch = dtype == F3DG_F32 ? launch_gn_bwd<float> : dtype == F3DG_BF16 ? launch_gn_bwd<unsigned short> : launch_gn_bwd<_Float16>;
    return launch(stream, N, C, HW, groups, nhwc, x, pre_bias, weight, bias, stats, apply_silu, grad_y, grad_x, grad_weight, grad_bias, grad_pre_bias, scratch,
                  scratch_bytes);
}

extern "C" int f3dg_group_norm_silu_backward(void* stream, int N, int C, int HW, int groups, int nhwc, const float* x, const float* pre_bias,
                                             const float* weight, const float* bias, const float* stats, int apply_silu, const float* grad_y,
                                             float* grad_x, float* grad_weight, float* grad_bias, float* grad_pre_bias, void* scratch,
                                             size_t scratch_bytes)
{
    return f3dg_group_norm_silu_backward_dtype(stream, F3DG_F32, N, C, HW, groups, nhwc, x, pre_bias, weight, bias, stats, apply_silu, grad_y, grad_x,
                                               grad_weight, grad_bias, grad_pre_bias, scratch, scratch_bytes);
}

extern "C" size_t f3dg_residual_join_backward_scratch_bytes(int N, int C, int HW, int nhwc)
{
    if (N <= 0 || C <= 0 || HW <= 0) return 0;
    return sizeof(double) * join_bwd_segments(N, HW, nhwc) * (size_t)C;
}

extern "C" int f3dg_residual_join_backward_dtype(void* stream, int dtype, int N, int C, int HW, int nhwc, const void* grad_y, float scale, void* grad_ab,
                                                 float* grad_bias, void* scratch, size_t scratch_bytes)
{
    if (dtype < F3DG_F32 || dtype > F3DG_F16) return F3DG_ERR_BAD_ARG;
    const auto launch = dtype == F3DG_F32 ? launch_join_bwd<float> : dtype == F3DG_BF16 ? launch_join_bwd<unsigned short> : launch_join_bwd<_Float16>;
    return launch(stream, N, C, HW, nhwc, grad_y, scale, grad_ab, grad_bias, scratch, scratch_bytes);
}

extern "C" int f3dg_residual_join_backward(void* stream, int N, int C, int HW, int nhwc, const float* grad_y, float scale, float* grad_ab,
                                           float* grad_bias, void* scratch, size_t scratch_bytes)
{
    return f3dg_residual_join_backward_dtype(stream, F3DG_F32, N, C, HW, nhwc, grad_y, scale, grad_ab, grad_bias, scratch, scratch_bytes);
}
