"""Float64 gradient truth, restatements and yardsticks for the backward of the backbone's kernels between the convolutions
(csrc/f3dg_groupnorm_bwd.hip). Data, forward truth and the bound rule are tests/backbone_truth.py's; this module adds what a gradient
check needs on top:

  grad_truth      autograd of ``T.truth`` in float64 -- THE truth
  grad_formulas   the backward formulas of include/f3dg.h written out in numpy float64 (pins the truth)
  grad_restated32 the same formulas in float32 elementwise arithmetic with float64 sums, mean taken off before the scale: what a sound
                  kernel computes, up to the order of the additions
  grad_torch32    autograd of ``T.torch32``: torch's float32 operators, the yardstick whose error E32 sets the bound
"""
import numpy as np
import torch

import backbone_truth as T

NAMES = ("dx", "dweight", "dbias", "dpre_bias")


def cotangent(shape, seed):
    """grad_y ~ N(0, 1), float32, seeded."""
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float32)


def _autograd(fn, x, pre_bias, weight, bias, groups, eps, silu, gy, dtype):
    leaves = [x.detach().to(dtype).requires_grad_(), weight.detach().to(dtype).requires_grad_(), bias.detach().to(dtype).requires_grad_()]
    pb = None if pre_bias is None else pre_bias.detach().to(dtype).requires_grad_()
    if pb is not None:
        leaves.append(pb)
    y = fn(leaves[0], pb, leaves[1], leaves[2], groups, eps, silu)
    g = torch.autograd.grad(y, leaves, gy.to(device=y.device, dtype=y.dtype))
    out = {"dx": g[0], "dweight": g[1], "dbias": g[2]}
    if pb is not None:
        out["dpre_bias"] = g[3]
    return out


def grad_truth(x, pre_bias, weight, bias, groups, eps, silu, gy):
    """{name: float64 gradient} of sum(T.truth(...) * gy); dpre_bias only with a pre_bias. On x's device."""
    return _autograd(T.truth, x, pre_bias, weight, bias, groups, eps, silu, gy, torch.float64)


def grad_torch32(x, pre_bias, weight, bias, groups, eps, silu, gy):
    """The same through torch's float32 operators (T.torch32), on x's device."""
    return _autograd(T.torch32, x, pre_bias, weight, bias, groups, eps, silu, gy, torch.float32)


def _formulas(x, pre_bias, weight, bias, groups, eps, silu, gy, ft):
    """The backward formulas; elementwise arithmetic in numpy type ``ft``, every sum in float64."""
    N, C = x.shape[:2]
    cs = (1, C) + (1,) * (x.ndim - 2)
    red = (0,) + tuple(range(2, x.ndim))
    v = x.astype(ft)
    if pre_bias is not None:
        v = v + pre_bias.astype(ft).reshape(cs)
    s = v.reshape(N, groups, -1)
    m = s.shape[-1]
    mean = (s.astype(np.float64).sum(-1, keepdims=True) / m)
    mean = mean + (s.astype(np.float64) - mean).sum(-1, keepdims=True) / m
    var = ((s.astype(np.float64) - mean) ** 2).sum(-1, keepdims=True) / m
    r = (1.0 / np.sqrt(var + eps)).astype(ft)
    xh = ((s - mean.astype(ft)) * r).reshape(x.shape)          # the mean off first, then the scale
    w = weight.astype(ft).reshape(cs)
    dz = gy.astype(ft)
    if silu:
        z = xh * w + bias.astype(ft).reshape(cs)
        sg = (ft(1) / (ft(1) + np.exp(-z))).astype(ft)
        dz = dz * (sg * (ft(1) + z * (ft(1) - sg)))
    A = dz.astype(np.float64).reshape(N, C, -1).sum(-1)                                  # [N, C]
    B = (dz * xh).astype(np.float64).reshape(N, C, -1).sum(-1)
    w64 = weight.astype(np.float64)
    s1 = ((w64 * A).reshape(N, groups, -1).sum(-1) / m).astype(ft)                      # [N, groups]
    s2 = ((w64 * B).reshape(N, groups, -1).sum(-1) / m).astype(ft)
    per_group = lambda t: np.repeat(t, C // groups, axis=1).reshape((N, C) + (1,) * (x.ndim - 2))
    dx = per_group(r.reshape(N, groups)) * ((dz * w - per_group(s1)) - xh * per_group(s2))
    out = {"dx": dx, "dweight": B.sum(0), "dbias": A.sum(0)}
    if pre_bias is not None:
        out["dpre_bias"] = dx.astype(np.float64).sum(red)
    return {k: torch.from_numpy(np.asarray(t, dtype=np.float64)) for k, t in out.items()}


def grad_formulas(x, pre_bias, weight, bias, groups, eps, silu, gy):
    f = lambda t: None if t is None else t.detach().cpu().double().numpy()
    return _formulas(f(x), f(pre_bias), f(weight), f(bias), groups, eps, silu, f(gy), np.float64)


def grad_restated32(x, pre_bias, weight, bias, groups, eps, silu, gy):
    f = lambda t: None if t is None else t.detach().cpu().float().numpy()
    return _formulas(f(x), f(pre_bias), f(weight), f(bias), groups, eps, silu, f(gy), np.float32)


def compare(got, ref, yard):
    """[(name, error, bound, ratio)] for every gradient of ``ref``: error = max|got - ref|, bound = T.bound32(E32, ref), E32 the error of
    ``yard`` (torch's float32 autograd on the same case)."""
    rows = []
    for k in NAMES:
        if k not in ref:
            continue
        r = ref[k].double().cpu()
        e32 = float((yard[k].double().cpu() - r).abs().max())
        err = float((got[k].double().cpu().reshape(r.shape) - r).abs().max())
        bnd = T.bound32(e32, r)
        rows.append((k, err, bnd, err / bnd))
    return rows


def gn_backward_scratch_bytes(N, C, HW, groups, nhwc):
    """The scratch of f3dg_group_norm_silu_backward as include/f3dg.h describes it: (A, B, X) per (sample, channel), (s1, s2) per (sample,
    group), and channels-last a triple per workgroup and channel -- a workgroup takes 512 pixels from 128 x 128 on, 64 below."""
    pix = 512 if HW >= 16384 else 64
    nb = (HW + pix - 1) // pix
    return 8 * (3 * N * C + 2 * N * groups + (3 * N * nb * C if nhwc else 0))


def join_backward_scratch_bytes(N, C, HW, nhwc):
    """One float64 per segment and channel: NCHW a segment is up to 4096 values of one plane, channels-last a run of 256 of the N * HW pixels."""
    nseg = (N * HW + 255) // 256 if nhwc else N * ((HW + 4095) // 4096)
    return 8 * nseg * C
