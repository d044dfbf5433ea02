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
No double backward. Everything is enqueued on the current stream.

The geometry terms the reference's settings file weighs besides RGB (config/imagenetgs_256x256_v1.yaml:50-66: ``w_depth_normal``,
``w_distortion``, ``w_depth``, ``w_normal``, ``w_alpha``) read the nine raster planes themselves: ``geometry_sums`` is ONE forward kernel
(``f3dg_geometry_loss_forward``: the five per-frame sums, the world normal and the depth normal of a pixel formed in registers with the
epilogue's own arithmetic and never written) and ONE backward kernel (``f3dg_geometry_loss_backward``: dL/draster directly, the cotangent
of the sums as its per-frame weights). ``geometry_loss`` blends them; ``normal_consistency``, ``distortion_loss`` and ``depth_loss`` are
single-term wrappers. ``out["raster"]`` of ``render_views(..., differentiable=True)`` goes in as it is.

The settings' ``w_warping`` term compares a novel render with the forward-warped input view (``warp.forward_warp``) under the warp's
mask: ``warping_sums`` is ONE forward kernel plus the same fixed-order second stage (``f3dg_masked_l1_forward``) and ONE backward kernel
(``f3dg_masked_l1_backward``); ``warping_loss`` is its mean. Only the render receives a gradient: the warp is data."""
import math

import torch

from . import _lib
from .diff_gof_rasterization import _stream

__all__ = ["ssim", "ssim_map", "l1_loss", "l2_loss", "psnr", "image_metrics", "photometric_loss",
           "geometry_sums", "geometry_loss", "normal_consistency", "distortion_loss", "depth_loss", "warping_sums", "warping_loss"]


def _sum_buffers(partials_bytes, shape, terms, dev, who, unit, size):
    """(tile slots, their bytes, sums [n, terms]) of a two-stage sum over ``shape = (n, ...)``; 0 bytes is a shape the library refuses."""
    nbytes = partials_bytes(*shape)
    if nbytes == 0:
        raise ValueError(f"{who}: bad {unit} count / size ({shape[0]} {unit}s of {size})")
    return torch.empty(nbytes // 4, dtype=torch.float32, device=dev), nbytes, torch.empty((shape[0], terms), dtype=torch.float32, device=dev)


def _dense(g, dev):
    """A cotangent as the backward kernels read it: dense float32 on ``dev`` (None stays None)."""
    return None if g is None else g.to(device=dev, dtype=torch.float32).contiguous()


def _forward_call(img1, img2, n_planes, H, W, want_map, want_planes):
    """The raw forward on contiguous float32 device tensors: (map | None, three planes | None, plane_sums [n_planes, 3])."""
    L = _lib.lib()
    dev = img1.device
    new = lambda: torch.empty((n_planes, H, W), dtype=torch.float32, device=dev)
    m = new() if want_map else None
    planes = (new(), new(), new()) if want_planes else (None, None, None)
    partials, nbytes, sums = _sum_buffers(L.f3dg_ssim_partials_bytes, (n_planes, W, H), 3, dev, "image loss", "plane", f"{H} x {W}")
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
        g_map, g_sums = _dense(g_map, img1.device), _dense(g_sums, img1.device)
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


# ------------------------------------------------------------------------------------------------ geometry terms
class _GeometryLoss(torch.autograd.Function):
    """``f3dg_geometry_loss_forward`` with ``f3dg_geometry_loss_backward`` behind it: frame_sums [F, 5] of a contiguous float32
    [F, 9, H, W] raster. Saves its inputs only; the cotangent of the sums goes to the backward kernel as its per-frame weights."""

    @staticmethod
    def forward(ctx, raster, world_view, depth_target, normal_target, alpha_target, mask, fx, fy, flags):
        F, _, H, W = raster.shape
        L = _lib.lib()
        partials, nbytes, sums = _sum_buffers(L.f3dg_geometry_loss_partials_bytes, (F, W, H), 5, raster.device, "geometry loss", "frame", f"{H} x {W}")
        rc = L.f3dg_geometry_loss_forward(_stream(), F, H, W, _lib.ptr(raster), _lib.ptr(world_view), fx, fy, flags, _lib.ptr(depth_target),
                                          _lib.ptr(normal_target), _lib.ptr(alpha_target), _lib.ptr(mask), _lib.ptr(partials), nbytes,
                                          _lib.ptr(sums))
        _lib.check(rc, "f3dg_geometry_loss_forward")
        ctx.set_materialize_grads(False)
        if ctx.needs_input_grad[0]:
            ctx.save_for_backward(raster, world_view, depth_target, normal_target, alpha_target, mask)
            ctx.scalars = (fx, fy, flags)
        return sums

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_sums):
        if g_sums is None:
            return (None,) * 9
        raster, world_view, depth_target, normal_target, alpha_target, mask = ctx.saved_tensors
        fx, fy, flags = ctx.scalars
        F, _, H, W = raster.shape
        g_sums = _dense(g_sums, raster.device)
        d_raster = torch.empty_like(raster)
        rc = _lib.lib().f3dg_geometry_loss_backward(_stream(), F, H, W, _lib.ptr(raster), _lib.ptr(world_view), fx, fy, flags,
                                                    _lib.ptr(depth_target), _lib.ptr(normal_target), _lib.ptr(alpha_target), _lib.ptr(mask),
                                                    _lib.ptr(g_sums), _lib.ptr(d_raster))
        _lib.check(rc, "f3dg_geometry_loss_backward")
        return (d_raster,) + (None,) * 8


def _geometry_data(t, name, who, lead, planes, H, W, dev, allow_bool=False):
    """A target or the mask as a contiguous float32 [F, planes, H, W] device tensor (None stays None). ``planes`` = 1 also takes
    [..., H, W] without the plane axis."""
    if t is None:
        return None
    if torch.is_grad_enabled() and t.requires_grad:
        raise NotImplementedError(f"{who} produces no gradient for `{name}`: detach it (only `raster` receives a gradient)")
    if allow_bool and t.dtype == torch.bool:
        t = t.to(torch.float32)
    if t.dtype != torch.float32:
        raise TypeError(f"{who}: `{name}` must be float32 (got {t.dtype})")
    want = tuple(lead) + (planes, H, W)
    if tuple(t.shape) != want and not (planes == 1 and tuple(t.shape) == tuple(lead) + (H, W)):
        raise ValueError(f"{who}: `{name}` is {tuple(t.shape)}; the raster {tuple(lead) + (9, H, W)} needs {want}")
    if t.device != dev:
        raise RuntimeError(f"f3dgaus_amd.losses.{who} needs `{name}` on the raster's HIP device (no CPU fallback)")
    return t.detach().contiguous().reshape(-1, planes, H, W)


def _geometry_sums(raster, world_views, cfg, who, alpha_weight=False, depth_target=None, normal_target=None, alpha_target=None, mask=None):
    """Boundary checks in this package's manner, then the autograd function: ([F, 5] sums, the raster's leading shape, H, W)."""
    if raster.dim() < 3 or raster.shape[-3] != 9:
        raise ValueError(f"{who}: the raster is [..., 9, H, W]; got {tuple(raster.shape)}")
    if raster.numel() == 0:
        raise ValueError(f"{who}: empty raster {tuple(raster.shape)}")
    if raster.dtype != torch.float32:
        raise TypeError(f"{who}: the raster must be float32 (got {raster.dtype})")
    lead, (H, W) = tuple(raster.shape[:-3]), raster.shape[-2:]
    F = raster.numel() // (9 * H * W)
    if world_views is None:                    # no term that reads a camera was asked for
        wv = torch.eye(4, dtype=torch.float32, device=raster.device).reshape(1, 16)
        fx = fy = 1.0
    else:
        if torch.is_grad_enabled() and world_views.requires_grad:
            raise NotImplementedError(f"{who} produces no gradient for the cameras (`world_views`): detach them")
        if world_views.dtype != torch.float32:
            raise TypeError(f"{who}: `world_views` must be float32 (got {world_views.dtype})")
        if world_views.numel() == 0 or world_views.numel() % 16:
            raise ValueError(f"{who}: `world_views` is [F, 4, 4] or [F, 16]; got {tuple(world_views.shape)}")
        wv = world_views.detach().reshape(-1, 16)
        FoV = cfg['model']['fov'] * math.pi / 180
        fx, fy = W / (2 * math.tan(FoV / 2.)), H / (2 * math.tan(FoV / 2.))          # as render_views forms them for its epilogue
    V = wv.shape[0]
    if F % V:
        raise ValueError(f"{who}: {V} cameras for {F} frames: one per frame, or V with F = n * V (frame b * V + v, as render_views(bs=None))")
    dev = raster.device
    data = [_geometry_data(depth_target, "depth_target", who, lead, 1, H, W, dev), _geometry_data(normal_target, "normal_target", who, lead, 3, H, W, dev),
            _geometry_data(alpha_target, "alpha_target", who, lead, 1, H, W, dev), _geometry_data(mask, "mask", who, lead, 1, H, W, dev, allow_bool=True)]
    if dev.type != "cuda" or wv.device != dev:
        raise RuntimeError(f"f3dgaus_amd.losses.{who} needs the raster and `world_views` on one HIP device (no CPU fallback)")
    if V != F:
        wv = wv.repeat(F // V, 1)              # image-major
    sums = _GeometryLoss.apply(raster.contiguous().reshape(F, 9, H, W), wv.contiguous(), *data, float(fx), float(fy),
                               _lib.GEOM_ALPHA_WEIGHT if alpha_weight else 0)
    return sums, lead, H, W


def geometry_sums(raster, world_views, cfg, *, alpha_weight=False, depth_target=None, normal_target=None, alpha_target=None, mask=None):
    """The per-frame sums [F, 5] of the five geometry terms over a raster [..., 9, H, W] (F = the product of the leading dims), from ONE
    forward kernel; differentiable in ``raster`` through ONE backward kernel. With N = ``rendered_normal`` and D = ``depth_normal`` exactly
    as ``render_views`` returns them, n^ = normalize(raster[3:6]), d = raster[6], alpha = raster[7] and m = ``mask`` (1 without one):

        [:, 0]  depth-normal consistency  w (1 - <N, D>),   w = 1, or alpha with ``alpha_weight`` (as data: no gradient through w)
        [:, 1]  distortion                raster[8]
        [:, 2]  depth                     m |d - depth_target|
        [:, 3]  normal                    m (1 - <n^, normal_target>)   (camera frame; the target is used as given)
        [:, 4]  alpha                     |alpha - alpha_target|

    A term whose target is None is 0 and contributes no gradient. ``world_views`` is [F, 4, 4] or [F, 16], one per frame, or [V, ...] with
    F = n * V (frame b * V + v, as ``render_views(bs=None)`` lays frames out); the focal lengths come from ``cfg['model']['fov']`` and the
    raster's own W, H. Targets are float32 [..., H, W] or [..., 1, H, W] ([..., 3, H, W] for the normals) with the raster's leading dims;
    the mask may also be bool. Only ``raster`` receives a gradient."""
    return _geometry_sums(raster, world_views, cfg, "geometry_sums", alpha_weight, depth_target, normal_target, alpha_target, mask)[0]


_BLEND = {}


def _blend_weights(weights, device):
    """(columns of the non-zero weights or None for all five, their float32 values) as device tensors, built once per (device, weights):
    the blend of a training step then costs no host-to-device copy."""
    key = (device, tuple(weights))
    hit = _BLEND.get(key)
    if hit is None:
        cols = [k for k, w in enumerate(weights) if w != 0.0]
        hit = (None if len(cols) == len(weights) else torch.tensor(cols, dtype=torch.long, device=device),
               torch.tensor([weights[k] for k in cols], dtype=torch.float32, device=device))
        if len(_BLEND) >= 64:           # (weights on a schedule: keep the table small)
            _BLEND.clear()
        _BLEND[key] = hit
    return hit


def _geometry_loss(who, raster, world_views, cfg, weights, alpha_weight=False, depth_target=None, normal_target=None, alpha_target=None,
                   mask=None, reduction="mean"):
    """``geometry_loss`` with the weights in the order of the sums' columns; a term with weight 0 is not handed to the kernel."""
    if reduction not in ("mean", "none"):
        raise ValueError(f"{who}: reduction must be 'mean' or 'none' (got {reduction!r})")
    weights = [float(w) for w in weights]
    targets = [depth_target, normal_target, alpha_target]
    for w, t, name in zip(weights[2:], targets, ("depth", "normal", "alpha")):
        if w != 0.0 and t is None:
            raise ValueError(f"{who}: w_{name} = {w} needs `{name}_target`")
    depth_target, normal_target, alpha_target = (t if w != 0.0 else None for w, t in zip(weights[2:], targets))
    sums, lead, H, W = _geometry_sums(raster, world_views, cfg, who, alpha_weight, depth_target, normal_target, alpha_target,
                                      mask if (weights[2] != 0.0 or weights[3] != 0.0) else None)
    cols, w = _blend_weights(weights, sums.device)
    if w.numel() == 0:
        per_frame = torch.zeros(sums.shape[0], dtype=torch.float32, device=sums.device)
    else:           # (a column with weight 0 is left out, not multiplied by 0: whatever it holds cannot reach the loss)
        per_frame = ((sums if cols is None else sums.index_select(1, cols)) * w).sum(1)
    if reduction == "mean":
        return per_frame.sum() / float(sums.shape[0] * H * W)
    return per_frame.reshape(lead) / float(H * W)


def geometry_loss(raster, world_views, cfg, *, w_depth_normal=0., w_distortion=0., w_depth=0., w_normal=0., w_alpha=0., alpha_weight=False,
                  depth_target=None, normal_target=None, alpha_target=None, mask=None, reduction="mean"):
    """The weighted sum of the geometry terms of ``geometry_sums``, the weights named as the reference's settings file names them
    (config/imagenetgs_256x256_v1.yaml:50-66). Every term is its mean over ALL pixels (masked terms too: their sum over F * H * W).
    ``reduction="mean"``: a scalar; ``"none"``: the loss of every frame (the raster's leading shape), each term divided by H * W.
    A term with weight 0 is not evaluated; a non-zero weight whose target is missing raises ``ValueError``."""
    return _geometry_loss("geometry_loss", raster, world_views, cfg, (w_depth_normal, w_distortion, w_depth, w_normal, w_alpha), alpha_weight,
                          depth_target, normal_target, alpha_target, mask, reduction)


def normal_consistency(raster, world_views, cfg, alpha_weight=False):
    """mean(w (1 - <rendered_normal, depth_normal>)) over all pixels of all frames, w = 1 or the rendered alpha (``alpha_weight``)."""
    return _geometry_loss("normal_consistency", raster, world_views, cfg, (1.0, 0.0, 0.0, 0.0, 0.0), alpha_weight)


def distortion_loss(raster):
    """The mean of the distortion map (raster[..., 8, :, :])."""
    return _geometry_loss("distortion_loss", raster, None, None, (0.0, 1.0, 0.0, 0.0, 0.0))


def depth_loss(raster, depth_target, mask=None):
    """mean(mask |rendered_depth - depth_target|) over all pixels of all frames."""
    return _geometry_loss("depth_loss", raster, None, None, (0.0, 0.0, 1.0, 0.0, 0.0), depth_target=depth_target, mask=mask)


# ------------------------------------------------------------------------------------------------ warping term
class _MaskedL1(torch.autograd.Function):
    """``f3dg_masked_l1_forward`` with ``f3dg_masked_l1_backward`` behind it: frame_sums [F, 2] of contiguous float32 a, b [F, C, H, W]
    and m [F, 1, H, W]. Saves its inputs only; the cotangent of the sums goes to the backward kernel as its per-frame weights."""

    @staticmethod
    def forward(ctx, a, b, m):
        F, C, H, W = a.shape
        L = _lib.lib()
        partials, nbytes, sums = _sum_buffers(L.f3dg_masked_l1_partials_bytes, (F, C, W, H), 2, a.device, "warping loss", "frame", f"{C} x {H} x {W}")
        rc = L.f3dg_masked_l1_forward(_stream(), F, C, H, W, _lib.ptr(a), _lib.ptr(b), _lib.ptr(m), _lib.ptr(partials), nbytes, _lib.ptr(sums))
        _lib.check(rc, "f3dg_masked_l1_forward")
        ctx.set_materialize_grads(False)
        if ctx.needs_input_grad[0]:
            ctx.save_for_backward(a, b, m)
        return sums

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_sums):
        if g_sums is None:
            return None, None, None
        a, b, m = ctx.saved_tensors
        F, C, H, W = a.shape
        g_sums = _dense(g_sums, a.device)
        d_a = torch.empty_like(a)
        rc = _lib.lib().f3dg_masked_l1_backward(_stream(), F, C, H, W, _lib.ptr(a), _lib.ptr(b), _lib.ptr(m), _lib.ptr(g_sums), _lib.ptr(d_a))
        _lib.check(rc, "f3dg_masked_l1_backward")
        return d_a, None, None


def _warping_sums(render, warped, mask, who):
    """Boundary checks in this package's manner, then the autograd function: ([F, 2] sums, (C, H, W))."""
    if render.dim() < 3:
        raise ValueError(f"{who}: the render is [..., C, H, W]; got {tuple(render.shape)}")
    if render.numel() == 0:
        raise ValueError(f"{who}: empty render {tuple(render.shape)}")
    if warped.dim() < 3 or warped.shape[-3:] != render.shape[-3:] or warped.numel() != render.numel():
        raise ValueError(f"{who}: `render` and `warped` differ in shape: {tuple(render.shape)} vs {tuple(warped.shape)} (the same [C, H, W] and "
                         "the same number of frames: [B * V, ...] against [B, V, ...] is fine)")
    if render.dtype != torch.float32 or warped.dtype != torch.float32:
        raise TypeError(f"{who}: `render` and `warped` must be float32 (got {render.dtype} and {warped.dtype})")
    if torch.is_grad_enabled() and warped.requires_grad:
        raise NotImplementedError(f"{who} produces no gradient for `warped` (the warp is data): detach it")
    lead, (C, H, W) = tuple(render.shape[:-3]), render.shape[-3:]
    dev = render.device
    if torch.is_grad_enabled() and mask.requires_grad:
        raise NotImplementedError(f"{who} produces no gradient for `mask`: detach it (only `render` receives a gradient)")
    if mask.dtype == torch.bool:
        mask = mask.to(torch.float32)
    if mask.dtype != torch.float32:
        raise TypeError(f"{who}: `mask` must be float32 or bool (got {mask.dtype})")
    if mask.dim() < 2 or tuple(mask.shape[-2:]) != (H, W) or mask.numel() * C != render.numel():
        raise ValueError(f"{who}: `mask` is {tuple(mask.shape)}; the render {tuple(render.shape)} needs {lead + (1, H, W)} (or its frames "
                         "under other leading dims)")
    if dev.type != "cuda" or warped.device != dev or mask.device != dev:
        raise RuntimeError(f"f3dgaus_amd.losses.{who} needs `render`, `warped` and `mask` on one HIP device (no CPU fallback)")
    sums = _MaskedL1.apply(render.contiguous().reshape(-1, C, H, W), warped.detach().contiguous().reshape(-1, C, H, W),
                           mask.detach().contiguous().reshape(-1, 1, H, W))
    return sums, (C, H, W)


def warping_sums(render, warped, mask):
    """The per-frame sums [F, 2] of the warping term over ``render`` and ``warped`` [..., C, H, W] and ``mask`` [..., 1, H, W] (or
    [..., H, W]; float32 or bool), F the product of the leading dims, which may be split differently -- ``render_views(...,
    differentiable=True)["render"]`` [B * V, 3, H, W] (image-major) and ``warp.forward_warp``'s [B, V, 3, H, W] go in as they are:

        [:, 0]  sum over channels and pixels of  m |render - warped|
        [:, 1]  sum over pixels of  m

    ONE forward kernel and a fixed-order second stage (bit-reproducible); differentiable in ``render`` only, through ONE backward kernel:
    ``m sign(render - warped)`` times the cotangent of column 0."""
    return _warping_sums(render, warped, mask, "warping_sums")[0]


def warping_loss(render, warped, mask, reduction="mean"):
    """``sum(m |render - warped|) / (F C H W)``: the masked L1 against the warped frame as a mean over ALL pixels, the convention
    ``geometry_loss`` uses for its masked terms. ``reduction="none"``: the loss of every frame (the leading shape), each divided by
    C H W. To normalise by the covered pixels instead::

        s = warping_sums(render, warped, mask)
        loss = s[:, 0].sum() / (C * s[:, 1].sum()).clamp_min(1.0)"""
    if reduction not in ("mean", "none"):
        raise ValueError(f"warping_loss: reduction must be 'mean' or 'none' (got {reduction!r})")
    sums, (C, H, W) = _warping_sums(render, warped, mask, "warping_loss")
    if reduction == "mean":
        return sums[:, 0].sum() / float(sums.shape[0] * C * H * W)
    return sums[:, 0].reshape(tuple(render.shape[:-3])) / float(C * H * W)
