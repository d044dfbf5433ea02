"""Fused differentiable image losses on the HIP device: SSIM, L1, L2 / PSNR and the trainer's photometric objective.

``ssim`` / ``l1_loss`` / ``l2_loss`` have the signatures and results of the reference's ``utils/loss_utils.py`` (:17-21, :33-63),
``psnr`` those of ``utils/image_utils.py:17-19``; ``photometric_loss`` is ``(1 - lambda_dssim) * l1_loss + lambda_dssim * (1 - ssim)``
(``train.py:92``, ``arguments/__init__.py:83``: lambda_dssim = 0.2). Where the reference runs five depthwise 11 x 11 ``conv2d`` calls and
about twenty elementwise kernels per evaluation and keeps their autograd graph, everything here is ONE forward kernel over all
frames (``f3dg_ssim_forward``: the map when asked for, the three derivative planes the backward needs, and per-plane sums of the map,
of |a - b| and of (a - b)^2, added up by a tiny fixed-order second stage) and ONE backward kernel (``f3dg_ssim_backward``). The
reductions that follow -- a mean over planes, the blend of the two terms -- are torch operations on an [n_planes, 3] tensor; autograd
hands their gradient back as the kernel's per-plane weights, so a mean never materialises a gradient plane.

Inputs are float32 ``[..., C, H, W]`` on one HIP device (no CPU fallback); only ``img1`` (the prediction) receives a gradient -- SSIM is
symmetric, swap the arguments for the other side. The outputs of ``render_views(..., differentiable=True)["render"]`` go in as they are.
No double backward. Everything is enqueued on the current stream."""
import torch

from . import _lib
from .diff_gof_rasterization import _stream

__all__ = ["ssim", "ssim_map", "l1_loss", "l2_loss", "psnr", "image_metrics", "photometric_loss"]


def _forward_call(img1, img2, n_planes, H, W, want_map, want_planes):
    """The raw forward on contiguous float32 device tensors: (map | None, three planes | None, plane_sums [n_planes, 3])."""
    L = _lib.lib()
    dev = img1.device
    new = lambda: torch.empty((n_planes, H, W), dtype=torch.float32, device=dev)
    m = new() if want_map else None
    planes = (new(), new(), new()) if want_planes else (None, None, None)
    nbytes = L.f3dg_ssim_partials_bytes(n_planes, W, H)
    if nbytes == 0:
        raise ValueError(f"image loss: bad plane count / size ({n_planes} planes of {H} x {W})")
    partials = torch.empty(nbytes // 4, dtype=torch.float32, device=dev)
    sums = torch.empty((n_planes, 3), dtype=torch.float32, device=dev)
    rc = L.f3dg_ssim_forward(_stream(), n_planes, W, H, _lib.ptr(img1), _lib.ptr(img2), _lib.ptr(m), *[_lib.ptr(p) for p in planes],
                             _lib.ptr(partials), nbytes, _lib.ptr(sums))
    _lib.check(rc, "f3dg_ssim_forward")
    return m, (planes if want_planes else None), sums


class _ImageLoss(torch.autograd.Function):
    """``f3dg_ssim_forward`` with ``f3dg_ssim_backward`` behind it: (map or None, plane_sums [n_planes, 3]) of contiguous float32
    [n_planes, H, W] inputs. Saves the two inputs and the three derivative planes; the cotangent of ``plane_sums`` goes to the backward
    kernel as its per-plane weights, that of the map (if it was used) as the gradient plane set."""

    @staticmethod
    def forward(ctx, img1, img2, want_map):
        n_planes, H, W = img1.shape
        ctx.set_materialize_grads(False)
        need_grad = ctx.needs_input_grad[0]
        m, planes, sums = _forward_call(img1, img2, n_planes, H, W, want_map, need_grad)
        if need_grad:
            ctx.save_for_backward(img1, img2, *planes)
        return m, sums          # (m is None when the map was not asked for)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_map, g_sums):
        if g_map is None and g_sums is None:
            return None, None, None
        img1, img2, p1, p2, p3 = ctx.saved_tensors
        n_planes, H, W = img1.shape
        dense = lambda g: None if g is None else g.to(device=img1.device, dtype=torch.float32).contiguous()
        g_map, g_sums = dense(g_map), dense(g_sums)
        d_img1 = torch.empty_like(img1)
        rc = _lib.lib().f3dg_ssim_backward(_stream(), n_planes, W, H, _lib.ptr(img1), _lib.ptr(img2), _lib.ptr(g_map), _lib.ptr(g_sums),
                                           _lib.ptr(p1), _lib.ptr(p2), _lib.ptr(p3), _lib.ptr(d_img1))
        _lib.check(rc, "f3dg_ssim_backward")
        return d_img1, None, None


def _prepare(img1, img2, who):
    """Boundary checks in this package's manner, then contiguous [n_planes, H, W] views of both images."""
    if img1.shape != img2.shape:
        raise ValueError(f"{who}: img1 and img2 differ in shape: {tuple(img1.shape)} vs {tuple(img2.shape)}")
    if img1.dim() < 3:
        raise ValueError(f"{who}: images are [..., C, H, W]; got {tuple(img1.shape)}")
    if img1.numel() == 0:
        raise ValueError(f"{who}: empty images {tuple(img1.shape)}")
    if img1.dtype != torch.float32 or img2.dtype != torch.float32:
        raise TypeError(f"{who}: images must be float32 (got {img1.dtype} and {img2.dtype})")
    if torch.is_grad_enabled() and img2.requires_grad:
        raise NotImplementedError(f"{who} produces no gradient for `img2` (the target): detach it, or swap the arguments -- SSIM, L1 and "
                                  "L2 are symmetric")
    if img1.device.type != "cuda" or img2.device != img1.device:
        raise RuntimeError(f"f3dgaus_amd.losses.{who} needs both images on one HIP device (no CPU fallback)")
    H, W = img1.shape[-2:]
    return img1.contiguous().reshape(-1, H, W), img2.detach().contiguous().reshape(-1, H, W)


def _sums(img1, img2, who, want_map=False):
    """(map [like img1] or None, plane_sums [n_planes, 3] float32: sum of the map, of |a - b|, of (a - b)^2 per plane)."""
    a, b = _prepare(img1, img2, who)
    m, sums = _ImageLoss.apply(a, b, bool(want_map))
    return (m.reshape(img1.shape) if want_map else None), sums


def _per_leading(sums_col, shape):
    """Mean over the last three dims per leading index from one column of plane_sums."""
    C, H, W = shape[-3:]
    return sums_col.reshape(tuple(shape[:-3]) + (C,)).sum(-1) / float(C * H * W)


def ssim_map(img1, img2):
    """The full SSIM map, shaped like the inputs; differentiable in ``img1`` with any upstream gradient."""
    return _sums(img1, img2, "ssim_map", want_map=True)[0]


def ssim(img1, img2, window_size=11, size_average=True):
    """The reference's ``ssim`` (utils/loss_utils.py:33-63): the mean of the map -- over everything, or with ``size_average=False``
    over the last three dims for each leading index ([N] for [N, C, H, W] inputs). Only the reference's window of 11 exists here."""
    if window_size != 11:
        raise ValueError(f"ssim: the kernel implements the reference's window_size=11 only (got {window_size})")
    _, sums = _sums(img1, img2, "ssim")
    if size_average:
        return sums[:, 0].sum() / float(img1.numel())
    return _per_leading(sums[:, 0], img1.shape)


def l1_loss(network_output, gt):
    """``torch.abs(network_output - gt).mean()`` (utils/loss_utils.py:17-18)."""
    _, sums = _sums(network_output, gt, "l1_loss")
    return sums[:, 1].sum() / float(network_output.numel())


def l2_loss(network_output, gt):
    """``((network_output - gt) ** 2).mean()`` (utils/loss_utils.py:20-21)."""
    _, sums = _sums(network_output, gt, "l2_loss")
    return sums[:, 2].sum() / float(network_output.numel())


def psnr(img1, img2):
    """The reference's ``psnr`` (utils/image_utils.py:17-19): ``20 log10(1 / sqrt(mse))`` with the mean squared error over everything but
    the FIRST dim, shape ``[img1.shape[0], 1]``."""
    _, sums = _sums(img1, img2, "psnr")
    n0 = img1.shape[0]
    mse = sums[:, 2].reshape(n0, -1).sum(1, keepdim=True) / float(img1.numel() // n0)
    return 20 * torch.log10(1.0 / torch.sqrt(mse))


def image_metrics(img1, img2):
    """The per-frame metrics of the reference's ``metrics.py`` from ONE forward kernel over all frames: a dict with ``ssim``
    (``ssim(..., size_average=False)``: one value per leading index), ``psnr`` (``psnr``: [img1.shape[0], 1]) and ``l1`` (per leading
    index)."""
    _, sums = _sums(img1, img2, "image_metrics")
    n0 = img1.shape[0]
    mse = sums[:, 2].reshape(n0, -1).sum(1, keepdim=True) / float(img1.numel() // n0)
    return {"ssim": _per_leading(sums[:, 0], img1.shape), "psnr": 20 * torch.log10(1.0 / torch.sqrt(mse)),
            "l1": _per_leading(sums[:, 1], img1.shape)}


def photometric_loss(render, target, lambda_dssim=0.2, reduction="mean"):
    """``(1 - lambda_dssim) * l1_loss(render, target) + lambda_dssim * (1 - ssim(render, target))``, the reference trainer's objective
    (train.py:92), from ONE forward kernel; its backward is ONE kernel whose per-plane weights carry the upstream gradient.
    ``reduction="mean"``: a scalar over everything; ``"none"``: the loss of every leading index (every frame of [..., C, H, W])."""
    if reduction not in ("mean", "none"):
        raise ValueError(f"photometric_loss: reduction must be 'mean' or 'none' (got {reduction!r})")
    _, sums = _sums(render, target, "photometric_loss")
    lam = float(lambda_dssim)
    if reduction == "mean":
        n = float(render.numel())
        return (1.0 - lam) * (sums[:, 1].sum() / n) + lam * (1.0 - sums[:, 0].sum() / n)
    return (1.0 - lam) * _per_leading(sums[:, 1], render.shape) + lam * (1.0 - _per_leading(sums[:, 0], render.shape))
