"""Float64 truth for the fused image loss (f3dg_ssim_forward / f3dg_ssim_backward, f3dgaus_amd.losses), written from the definition in
include/f3dg.h: a direct 121-tap windowed sum over the zero-padded image with the window float32(outer(g, g)) as the reference builds
it (utils/loss_utils.py:23-31: ``_1D_window.mm(_1D_window.t()).float()``), everything else in float64. Gradients come from torch
float64 autograd through it. tests/test_ssim_truth.py pins this helper to the reference's own float64 results (tests/golden/ssim/*.npz,
written by tests/tools/gen_ssim_golden.py)."""
import math
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ssim")
SHAPES = ((2, 3, 7, 5), (1, 3, 37, 21), (2, 1, 33, 70), (2, 3, 64, 64))
CONTENTS = ("random", "near", "smooth", "flat")
PADDING_SHAPE = (1, 1, 13, 12)            # a = 1, b = 0.5: the extra fixture of the padding test
# The constants are the reference's Python floats (utils/loss_utils.py:55-56): its float64 evaluation uses them as they are, its float32
# evaluation -- and the kernel -- their float32 roundings. (With the rounded ones this helper is 4e-9 from the reference's float64 map.)
C1 = 0.01 ** 2
C2 = 0.03 ** 2
ULP = 2.0 ** -23                     # float32 spacing at 1


def case_name(shape, content):
    return "%s_%dx%dx%dx%d" % ((content,) + tuple(shape))


def cases():
    return [case_name(s, c) for s in SHAPES for c in CONTENTS]


def taps():
    """g[i] = float32(exp(-(i - 5)^2 / 4.5)) divided by their float32 sum, i = 0..10 -- float32 [11]."""
    g = torch.tensor([math.exp(-(i - 5) ** 2 / 4.5) for i in range(11)], dtype=torch.float32)
    return g / g.sum()


def window64():
    """The 11 x 11 window: float32(outer(g, g)), as float64."""
    g = taps().unsqueeze(1)
    return g.mm(g.t()).float().double()


def _windowed(x, w):
    """Direct windowed sum: out[..., y, x] = sum_{i,j} w[i, j] * xpad[..., y + i, x + j], zero padding 5. x float64 [..., H, W]."""
    H, W = x.shape[-2:]
    xp = torch.nn.functional.pad(x, (5, 5, 5, 5))
    out = torch.zeros_like(x)
    for i in range(11):
        for j in range(11):
            out = out + w[i, j] * xp[..., i:i + H, j:j + W]
    return out


def ssim_map64(a, b):
    """The SSIM map of float64 tensors [..., H, W] (differentiable). With float32 tensors it is the reference's float32 evaluation
    restated: the same 121 float32 window entries, the same float32 expression (the order of the 121 additions is this loop's)."""
    w = window64().to(a.dtype)
    mu1, mu2 = _windowed(a, w), _windowed(b, w)
    s1 = _windowed(a * a, w) - mu1 * mu1
    s2 = _windowed(b * b, w) - mu2 * mu2
    s12 = _windowed(a * b, w) - mu1 * mu2
    return ((2 * mu1 * mu2 + C1) * (2 * s12 + C2)) / ((mu1 * mu1 + mu2 * mu2 + C1) * (s1 + s2 + C2))


def truth(a, b, dL_dmap=None, plane_weights=None, dtype=torch.float64):
    """a, b: float32 (or float64) tensors / arrays [..., H, W]. ``dtype=torch.float32``: the reference's float32 evaluation restated
    (for E_ref of cotangents the fixtures do not hold). Returns a dict of numpy arrays in ``dtype``:
    map; sums [n_planes, 3] (of m, |a - b|, (a - b)^2 per plane); mean (of the map); grad_mean (d mean / d a);
    grad (d L / d a for L = sum(dL_dmap * map) + sum_planes w . sums, when either cotangent is given)."""
    a64 = torch.as_tensor(np.asarray(a)).to(dtype).clone().requires_grad_()
    b64 = torch.as_tensor(np.asarray(b)).to(dtype)
    m = ssim_map64(a64, b64)
    H, W = a64.shape[-2:]
    d = (a64 - b64).reshape(-1, H, W)
    sums = torch.stack([m.reshape(-1, H, W).sum((1, 2)), d.abs().sum((1, 2)), (d * d).sum((1, 2))], 1)
    out = {"map": m.detach().numpy(), "sums": sums.detach().numpy(), "mean": float(m.detach().mean())}
    out["grad_mean"] = torch.autograd.grad(m.mean(), a64, retain_graph=True)[0].numpy()
    if dL_dmap is not None or plane_weights is not None:
        L = 0
        if dL_dmap is not None:
            L = L + (torch.as_tensor(np.asarray(dL_dmap)).to(dtype) * m).sum()
        if plane_weights is not None:
            L = L + (torch.as_tensor(np.asarray(plane_weights)).to(dtype) * sums).sum()
        out["grad"] = torch.autograd.grad(L, a64)[0].numpy()
    return out


def load(name):
    """One golden case as a dict of numpy arrays (read-only use)."""
    with np.load(os.path.join(GOLDEN, name + ".npz")) as z:
        return {k: z[k] for k in z.files}


def bound(ref32, ref64, scale):
    """The tolerance rule of the GPU tests: the reference's own float32 error against the same truth on the same case (max abs),
    with a floor of 4 float32 ulps of the quantity's scale. The margin is 1 x: the kernel may not be less accurate than the reference."""
    return max(float(np.abs(np.asarray(ref32, dtype=np.float64) - np.asarray(ref64, dtype=np.float64)).max()), 4 * ULP * scale)


def max_err(got, ref64):
    if isinstance(got, torch.Tensor):
        got = got.detach().cpu().numpy()
    return float(np.abs(np.asarray(got, dtype=np.float64) - np.asarray(ref64, dtype=np.float64)).max())
