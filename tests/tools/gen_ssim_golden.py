"""Generates tests/golden/ssim/*.npz by running the REFERENCE's own loss functions (src/gaussian-splatting/utils/loss_utils.py and
utils/image_utils.py; they import on CPU torch as they are) -- build container only, the reference does not travel; the fixtures are
data only: arrays the reference's program read or wrote.

Per case (shape (N, C, H, W) x content, tests/ssim_truth.py: SHAPES, CONTENTS; plus the padding case a = 1, b = 0.5 on 13 rows x 12
columns), seeded:
    img1, img2          float32 inputs
    window              the reference's 1-D window (gaussian(11, 1.5)), float32 [11]
    map64, mean64, grad64   its _ssim on .double() inputs with the window .double(): the map, its mean, d mean / d img1 -- float64
    map32, mean32, grad32   its own float32 results (ssim(img1, img2))
    plane_mean32, plane_mean64  its ssim / _ssim of every plane on its own (a [1, 1, H, W] call each): float64 [N * C]
    dL_dmap             a seeded float32 cotangent for the map, and the reference's gradient for it (autograd from the map tensor inside
    grad_dl_err32, grad_dl_max64    its _ssim) as two recorded figures: max|g32 - g64| and max|g64|. The arrays would take the 64 x 64
                        files past 1 MiB; tests/ssim_truth.py's own float64 gradient is checked here to be within 1e-10 of g64.
    ssim_n32            ssim(..., size_average=False), float32 [N]
    l1_32, l2_32, psnr32    l1_loss, l2_loss (scalars) and psnr ([N, 1]) in float32
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import ref_import  # noqa: E402
import ssim_truth as T  # noqa: E402

sys.path.insert(0, os.path.join(ref_import.REF, "src", "gaussian-splatting"))
from utils import image_utils, loss_utils  # noqa: E402


def make_inputs(shape, content, seed):
    rng = np.random.default_rng(seed)
    N, C, H, W = shape
    if content == "random":
        a, b = rng.random(shape), rng.random(shape)
    elif content == "near":
        a = rng.random(shape)
        b = np.clip(a + 0.05 * rng.standard_normal(shape), 0.0, 1.0)
    elif content == "smooth":
        y, x = np.mgrid[0:H, 0:W]
        base = 0.5 + 0.4 * np.sin(2 * np.pi * (x / max(W, 8) + 0.5 * y / max(H, 8)))
        phase = rng.random((N, C, 1, 1))
        a = base[None, None] * (0.6 + 0.4 * phase) + 0.01 * rng.standard_normal(shape)
        b = base[None, None] * (0.6 + 0.4 * phase) + 0.01 * rng.standard_normal(shape)
    elif content == "flat":
        a = np.full(shape, 0.7)
        b = 0.7 + 0.001 * rng.standard_normal(shape)
    else:
        raise ValueError(content)
    return a.astype(np.float32), b.astype(np.float32)


def main():
    os.makedirs(T.GOLDEN, exist_ok=True)
    total = 0
    jobs = [(shape, content, 1000 + 10 * si + ci) for si, shape in enumerate(T.SHAPES) for ci, content in enumerate(T.CONTENTS)]
    jobs.append((T.PADDING_SHAPE, "padding", 0))
    for shape, content, seed in jobs:
        if content == "padding":
            a, b = np.ones(shape, np.float32), np.full(shape, 0.5, np.float32)
        else:
            a, b = make_inputs(shape, content, seed)
        C = shape[1]
        dl = np.random.default_rng(seed + 500).standard_normal(shape).astype(np.float32)
        out = {"img1": a, "img2": b, "window": loss_utils.gaussian(11, 1.5).numpy(), "dL_dmap": dl}
        g_dl = {}
        for tag, dt in (("64", torch.float64), ("32", torch.float32)):
            x = torch.from_numpy(a).to(dt).requires_grad_()
            y = torch.from_numpy(b).to(dt)
            if dt == torch.float64:
                window = loss_utils.create_window(11, C).double()
                m = loss_utils._ssim(x, y, window, 11, C, True)
            else:
                window = loss_utils.create_window(11, C)
                m = loss_utils.ssim(x, y)
            g, = torch.autograd.grad(m, x)
            out["mean" + tag] = np.asarray(m.detach().numpy())
            out["grad" + tag] = g.numpy()
            full = _map_through_reference(loss_utils, x, y, window, C)
            out["map" + tag] = full.detach().numpy()
            g_dl[tag] = torch.autograd.grad((full * torch.from_numpy(dl).to(dt)).sum(), x)[0].numpy()
            w1 = loss_utils.create_window(11, 1).to(dt)
            out["plane_mean" + tag] = np.array([float(loss_utils._ssim(xp[None, None], yp[None, None], w1, 11, 1, True))
                                                 for xp, yp in zip(x.detach().flatten(0, 1), y.flatten(0, 1))], dtype=np.float64)
        out["grad_dl_err32"] = np.float64(np.abs(g_dl["32"].astype(np.float64) - g_dl["64"]).max())
        out["grad_dl_max64"] = np.float64(np.abs(g_dl["64"]).max())
        dev = np.abs(T.truth(a, b, dL_dmap=dl)["grad"] - g_dl["64"]).max()
        assert dev <= 1e-10, dev
        with torch.no_grad():
            ta, tb = torch.from_numpy(a), torch.from_numpy(b)
            out["ssim_n32"] = loss_utils.ssim(ta, tb, size_average=False).numpy()
            out["l1_32"] = np.asarray(loss_utils.l1_loss(ta, tb).numpy())
            out["l2_32"] = np.asarray(loss_utils.l2_loss(ta, tb).numpy())
            out["psnr32"] = image_utils.psnr(ta, tb).numpy()
        path = os.path.join(T.GOLDEN, T.case_name(shape, content) + ".npz")
        np.savez_compressed(path, **out)
        total += os.path.getsize(path)
        print(path, os.path.getsize(path))
    print("total bytes", total)


def _map_through_reference(loss_utils, x, y, window, C):
    """The reference's _ssim returns only means of its map. The map is the tensor whose ``.mean()`` it returns -- the only reduction
    in the function -- so it is captured (with its autograd graph) by wrapping ``torch.Tensor.mean`` for the duration of one call of the
    reference's own code."""
    captured = {}
    orig = torch.Tensor.mean

    def capture(self, *a, **k):
        captured.setdefault("map", self)
        return orig(self, *a, **k)
    torch.Tensor.mean = capture
    try:
        loss_utils._ssim(x, y, window.to(x.dtype), 11, C, True)
    finally:
        torch.Tensor.mean = orig
    return captured["map"]


if __name__ == "__main__":
    main()
