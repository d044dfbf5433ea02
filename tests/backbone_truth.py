"""Float64 truth, test data and bounds for the backbone's kernels between the convolutions (csrc/f3dg_groupnorm.hip): GroupNorm (+ SiLU)
with the producing convolution's bias folded in, and the residual join. The truth is torch's own operators evaluated in float64;
tests/test_backbone_truth.py pins it to a plain two-pass evaluation written out in numpy and shows that a correct float32 implementation
stays inside the bounds the device tests (tests/test_backbone_kernels_gpu.py) use.

The data is built so that one tensor holds many (sample, group) slabs with DIFFERENT offsets: a one-pass variance E[x^2] - mean^2 loses
log2(1 + (mean / std)^2) bits, so |mean| / std is the quantity the sweep turns."""
import math

import numpy as np
import torch
import torch.nn.functional as F

RATIOS = (0.5, 10.0, 30.0, 100.0)
KINDS = ("near_constant", "constant")
EPS = 1e-6                      # the residual blocks' GroupNorm eps
JITTER = 0.2
FLOOR = 2e-6                    # floor of the float32 bound, times max(1, max|ref|): the suite's existing one for these kernels
MARGIN = 2.0                    # ... and its existing margin over torch's float32 error: a different, equally sound summation order

# shapes at which each path of the kernels is live (the GPU sweep and the CPU check of the bounds share them)
NCHW_SHAPES = ((2, 64, 8, 8),           # packets; the slab (2 * 64 elements) is shorter than the workgroup
               (1, 128, 48, 48),        # packets; nine trips per thread
               (2, 36, 7, 5))           # HW = 35: the scalar path in every type
# channels-last: a workgroup takes gn_nhwc_pix(HW) pixels with all channels -- 512 from 128 x 128 pixels on, 64 below -- as rows = 256 / (packets
# per pixel) rows of threads
NHWC_SHAPES = ((1, 128, 64, 64),        # rows = 8, 64 workgroups
               (1, 1024, 9, 9),         # rows = 1: a thread walks all 64 pixels of its workgroup
               (2, 384, 20, 13),        # 96 / 48 packets per pixel: idle threads, a last workgroup of 4 pixels
               (1, 8, 40, 40),          # 2 / 1 packets per pixel, rows = 128 / 256: more rows than a workgroup has pixels
               (1, 16, 192, 192))       # runs of 512 pixels, 72 workgroups per sample: the second trip of the finish kernel
# ... and the longest float32 runs the kernel makes, 64 pixels per thread in runs of 512 (device sweep only: 2 M elements)
NHWC_LONG_RUN = (1, 128, 128, 128)


def default_groups(C):
    """The group count gaussian_predictor.GroupNorm derives from the channel count."""
    return min(32, C // 4)


def contents():
    """(label, ratio, kind) of the conditioning sweep."""
    return [("ratio%g" % r, r, "normal") for r in RATIOS] + [(k, 0.0, k) for k in KINDS]


def _per_channel(v, like):
    return v.double().reshape(1, -1, *([1] * (like.dim() - 2)))


def truth(x, pre_bias, weight, bias, groups, eps, silu):
    """silu(group_norm(x + pre_bias[None, :, None, None])) in float64; x [N, C, ...] of any float type (upcast exactly), pre_bias None or [C]."""
    t = x.double()
    if pre_bias is not None:
        t = t + _per_channel(pre_bias, t)
    # GroupNorm does not see a shift of a whole slab: taking the slab's mean off first keeps float64's own rounding (2^-53 |mean| / std
    # per element, 1e-12 on the near-constant data) out of the truth
    s = t.reshape(t.shape[0], groups, -1)
    t = (s - s.mean(-1, keepdim=True)).reshape(t.shape)
    y = F.group_norm(t, groups, weight.double(), bias.double(), eps)
    return F.silu(y) if silu else y


def torch32(x, pre_bias, weight, bias, groups, eps, silu):
    """The yardstick: the same expression with torch's float32 operators on x's exact float32 upcast (NCHW-contiguous)."""
    t = x.float().contiguous()
    if pre_bias is not None:
        t = t + pre_bias.float().reshape(1, -1, *([1] * (t.dim() - 2)))
    y = F.group_norm(t, groups, weight.float(), bias.float(), eps)
    return F.silu(y) if silu else y


def truth_two_pass(x, pre_bias, weight, bias, groups, eps, silu):
    """The definition written out in numpy float64: mean (corrected once), then the mean of squared deviations, per (sample, group)."""
    t = x.double().numpy()
    N, C = t.shape[:2]
    if pre_bias is not None:
        t = t + pre_bias.double().numpy().reshape((1, C) + (1,) * (t.ndim - 2))
    s = t.reshape(N, groups, -1)
    mean = s.sum(-1, keepdims=True) / s.shape[-1]
    mean = mean + (s - mean).sum(-1, keepdims=True) / s.shape[-1]               # (the rounding of the first sum, taken back)
    var = ((s - mean) ** 2).sum(-1, keepdims=True) / s.shape[-1]
    y = ((s - mean) / np.sqrt(var + eps)).reshape(t.shape)
    cs = (1, C) + (1,) * (t.ndim - 2)
    y = y * weight.double().numpy().reshape(cs) + bias.double().numpy().reshape(cs)
    if silu:
        y = y / (1.0 + np.exp(-y))
    return torch.from_numpy(y)


def join_truth(a, bias_a, b, bias_b, scale):
    """((a + bias_a) + (b + bias_b)) * scale in float64; either bias may be None."""
    ta, tb = a.double(), b.double()
    if bias_a is not None:
        ta = ta + _per_channel(bias_a, ta)
    if bias_b is not None:
        tb = tb + _per_channel(bias_b, tb)
    return (ta + tb) * float(scale)


def make_case(shape, ratio, seed, kind="normal", groups=None):
    """float32 x [N, C, ...] whose (sample, group) slabs each have std 1 and mean +-ratio, sign and a jitter of +-20 % drawn per slab
    (kind "normal"); mean 8 and std 1e-3 ("near_constant"); or every element of a slab equal, a different value per slab ("constant").
    Returns a dict: x, weight in [0.5, 1.5], bias in [-0.5, 0.5], pre_bias ~ N(0, 0.3) (all float32, on the host), groups, and
    slab_ratio [N, groups], the |mean| / std each slab was given (normal kind)."""
    N, C = shape[:2]
    G = groups or default_groups(C)
    L = (C // G) * int(np.prod(shape[2:]))
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(N, G, L, generator=g, dtype=torch.float64)
    z = (z - z.mean(-1, keepdim=True)) / z.std(-1, unbiased=False, keepdim=True)
    sign = torch.randint(0, 2, (N, G, 1), generator=g).double() * 2 - 1
    jit = 1 + JITTER * (2 * torch.rand(N, G, 1, generator=g, dtype=torch.float64) - 1)
    if kind == "normal":
        x = z + sign * ratio * jit
    elif kind == "near_constant":
        x = 8.0 + 1e-3 * z
    elif kind == "constant":
        x = (sign * (1 + 7 * torch.rand(N, G, 1, generator=g, dtype=torch.float64))).expand(N, G, L)
    else:
        raise ValueError(kind)
    x = x.reshape(N, G, C // G, *shape[2:]).reshape(*shape).float().contiguous()
    return {"x": x, "groups": G,
            "weight": (0.5 + torch.rand(C, generator=g)).float(),
            "bias": (torch.rand(C, generator=g) - 0.5).float(),
            "pre_bias": (0.3 * torch.randn(C, generator=g)).float(),
            "slab_ratio": (ratio * jit).reshape(N, G)}


_FORMAT = {torch.bfloat16: (7, -126), torch.float16: (10, -14)}         # stored mantissa bits, exponent of the smallest normal


def spacing(t, dtype):
    """Distance between neighbouring values of bfloat16 / float16 at |t| (float64 tensor), subnormals included: 2^(e - mantissa bits)
    with e = floor(log2 |t|), held at the smallest normal's exponent below it."""
    bits, emin = _FORMAT[dtype]
    _, e = torch.frexp(t.double().abs())                # |t| = m 2^e, m in [0.5, 1)
    e = torch.where(t == 0, torch.full_like(e, emin), e - 1).clamp(min=emin)
    return torch.ldexp(torch.ones_like(t, dtype=torch.float64), e - bits)


def bound32(e32, ref):
    """max(2 E32, floor): what the float32 stage may be off by, E32 torch's float32 max abs error on the same case."""
    return max(MARGIN * e32, FLOOR * max(1.0, float(ref.abs().max())))


def worst(y, ref, e32, dtype):
    """(error, bound, ratio) of the element that comes closest to (or exceeds most) its bound. float32: the max abs error against
    bound32. 16-bit: per element bound32 + half the type's spacing at max(|y|, |ref|) -- the float32 stage plus ONE rounding of the
    result, evaluated where the element lies."""
    y, ref = y.double(), ref.double()
    err = (y - ref).abs()
    b = torch.full_like(err, bound32(e32, ref))
    if dtype in _FORMAT:
        b = b + 0.5 * spacing(torch.maximum(y.abs(), ref.abs()), dtype)
    r = torch.where(torch.isfinite(err), err / b, torch.full_like(err, math.inf))
    i = int(r.argmax())
    return float(err.flatten()[i]), float(b.flatten()[i]), float(r.flatten()[i])


def ulp32(t):
    """float32 spacing at |t| (float64 tensor)."""
    _, e = torch.frexp(t.double().abs())
    e = torch.where(t == 0, torch.full_like(e, -126), e - 1).clamp(min=-126)
    return torch.ldexp(torch.ones_like(t, dtype=torch.float64), e - 23)
