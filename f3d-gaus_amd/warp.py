"""Depth-based forward warp of frames into new cameras on the HIP device: the masked pseudo-target behind the settings' ``w_warping`` /
``w_prop`` (config/imagenetgs_256x256_v1.yaml:50-66: ``threshold``, ``erode_warped_mask``, ``erode_kernel_size``, ``erode_pad_size``).

The reference's release holds the settings, no trainer and no warp: the semantics are THIS project's (include/f3dg.h has the definition,
DESIGN.md the reasons, tests/warp_truth.py a float64 restatement). A source pixel with z-depth d is lifted through the rasterizer's own
pixel centre, moved into the target camera and splatted bilinearly into its four neighbours; a z-buffer pass keeps what the nearest
surface hides from contributing (a footprint claims a z-buffer pixel only with a bilinear weight of at least ``occlusion_min_weight``),
and the sums are resolved into ``warped``, ``warped_depth``, the total ``weight`` and ``mask = weight >= threshold``, optionally eroded.
``f3dg_forward_warp`` runs all source frames x target cameras of a call as ONE sequence of five launches; its accumulators are 64-bit
fixed point (step 2^-24, exact for |image| and depth up to 32768), so the outputs are bit-identical from run to run.

The warp is data: no gradient flows to the image, the depth or the cameras, and inputs that require grad are refused.
``losses.warping_loss`` compares a differentiable render with the result. Inputs are float32 on one HIP device (no CPU fallback);
everything is enqueued on the current stream."""
import math

import torch

from . import _lib
from .diff_gof_rasterization import _stream

__all__ = ["forward_warp", "relative_transforms"]


def relative_transforms(src_world_view, dst_world_views):
    """``rel[b, v] = inverse(src_world_view[b]) @ dst_world_views[b, v]`` (row-vector convention: a point of source camera b, as a row,
    times ``rel[b, v]`` is the point in target camera (b, v)). ``src_world_view`` [B, 4, 4]; ``dst_world_views`` [B, V, 4, 4], or
    [V, 4, 4] shared by all sources. The product runs in float64 where the inputs live, with no host synchronisation (a singular
    source camera yields non-finite entries, which warp nothing), and is rounded to float32: [B, V, 4, 4]."""
    if src_world_view.dim() != 3 or tuple(src_world_view.shape[1:]) != (4, 4):
        raise ValueError(f"relative_transforms: `src_world_view` is [B, 4, 4]; got {tuple(src_world_view.shape)}")
    B = src_world_view.shape[0]
    shape = tuple(dst_world_views.shape)
    if len(shape) == 3 and shape[1:] == (4, 4):
        dst = dst_world_views.unsqueeze(0)
    elif len(shape) == 4 and shape[0] == B and shape[2:] == (4, 4):
        dst = dst_world_views
    else:
        raise ValueError(f"relative_transforms: `dst_world_views` is [V, 4, 4] or [{B}, V, 4, 4]; got {shape}")
    if dst.shape[1] == 0 or B == 0:
        raise ValueError(f"relative_transforms: no cameras ({tuple(src_world_view.shape)}, {shape})")
    inv, _ = torch.linalg.inv_ex(src_world_view.detach().double(), check_errors=False)
    return (inv.unsqueeze(1) @ dst.detach().double()).to(torch.float32).expand(B, dst.shape[1], 4, 4).contiguous()


def _plane(t, name, B, H, W, dev, allow_bool=False):
    """``depth`` / ``valid`` as a contiguous float32 [B, H, W] device tensor."""
    if torch.is_grad_enabled() and t.requires_grad:
        raise NotImplementedError(f"forward_warp produces no gradient for `{name}`: detach it (the warp is data)")
    if allow_bool and t.dtype == torch.bool:
        t = t.to(torch.float32)
    if t.dtype != torch.float32:
        raise TypeError(f"forward_warp: `{name}` must be float32 (got {t.dtype})")
    if tuple(t.shape) not in ((B, H, W), (B, 1, H, W)):
        raise ValueError(f"forward_warp: `{name}` is {tuple(t.shape)}; the image needs {(B, H, W)} or {(B, 1, H, W)}")
    if t.device != dev:
        raise RuntimeError(f"f3dgaus_amd.warp.forward_warp needs `{name}` on the image's HIP device (no CPU fallback)")
    return t.detach().contiguous().reshape(B, H, W)


def forward_warp(image, depth, src_world_view, dst_world_views, cfg, *, valid=None, z_near=0.01, depth_tolerance=0.05,
                 occlusion_min_weight=1 / 16, threshold=None, erode=0, want_depth=True, want_weight=False, workspace=None):
    """Warp ``image`` [B, C, H, W] (1 <= C <= 16) with z-depth ``depth`` [B, H, W] or [B, 1, H, W], seen by cameras ``src_world_view``
    [B, 4, 4], into the cameras ``dst_world_views`` [B, V, 4, 4] (or [V, 4, 4], shared). One field of view for both sides, from
    ``cfg['model']['fov']``, as ``render_views`` forms fx and fy. Returns a dict:

        warped        [B, V, C, H, W]  the weighted mean colour of what lands on a pixel and survives the depth test; 0 where nothing does
        mask          [B, V, 1, H, W]  1.0 where the total bilinear weight reaches ``threshold`` (default ``cfg['model']['threshold']``,
                                       0.9 without one), else 0.0; with ``erode = k`` (odd, 3..15; 0 / 1 = off) its k x k minimum
                                       (``erode_kernel_size`` with ``erode_pad_size = k // 2``)
        warped_depth  [B, V, 1, H, W]  the weighted mean target-camera z (None with ``want_depth=False``)
        weight        [B, V, 1, H, W]  the total weight (None unless ``want_weight``)
        workspace     the scratch tensor of the call: hand it to the next call of the same shape to skip the allocation

    ``valid`` [B, H, W] / [B, 1, H, W] (float32 or bool): a source pixel takes part iff ``valid > 0``, its depth is finite and positive
    and its point lies beyond ``z_near`` in the target camera; the colour and depth of any other pixel are never read into arithmetic.
    A contribution must lie within ``depth_tolerance`` (depth units; the default 0.05 is a choice for the settings' 6.667..8.667 depth
    range, not a measurement) of the nearest surface on its pixel. No gradient reaches any input: tensors that require grad raise."""
    who = "forward_warp"
    if image.dim() != 4:
        raise ValueError(f"{who}: the image is [B, C, H, W]; got {tuple(image.shape)}")
    if image.numel() == 0:
        raise ValueError(f"{who}: empty image {tuple(image.shape)}")
    if image.dtype != torch.float32:
        raise TypeError(f"{who}: the image must be float32 (got {image.dtype})")
    B, C, H, W = image.shape
    if C > 16:
        raise ValueError(f"{who}: at most 16 channels (got {C})")
    for t, name in ((image, "image"), (src_world_view, "src_world_view"), (dst_world_views, "dst_world_views")):
        if torch.is_grad_enabled() and t.requires_grad:
            raise NotImplementedError(f"{who} produces no gradient for `{name}`: detach it (the warp is data)")
    dev = image.device
    depth = _plane(depth, "depth", B, H, W, dev)
    if valid is not None:
        valid = _plane(valid, "valid", B, H, W, dev, allow_bool=True)
    for t, name in ((src_world_view, "src_world_view"), (dst_world_views, "dst_world_views")):
        if t.dtype != torch.float32:
            raise TypeError(f"{who}: `{name}` must be float32 (got {t.dtype})")
    if tuple(src_world_view.shape) != (B, 4, 4):
        raise ValueError(f"{who}: `src_world_view` is {tuple(src_world_view.shape)}; the image needs {(B, 4, 4)}")
    if dev.type != "cuda" or src_world_view.device != dev or dst_world_views.device != dev:
        raise RuntimeError(f"f3dgaus_amd.warp.{who} needs the image and the cameras on one HIP device (no CPU fallback)")
    erode = int(erode)
    if erode < 0 or erode > 15 or (erode > 0 and erode % 2 == 0):
        raise ValueError(f"{who}: erode is an odd window of at most 15 (0 or 1: off); got {erode}")
    rel = relative_transforms(src_world_view, dst_world_views)
    V = rel.shape[1]
    if threshold is None:
        threshold = cfg['model'].get('threshold', 0.9)
    FoV = cfg['model']['fov'] * math.pi / 180
    fx, fy = W / (2 * math.tan(FoV / 2.)), H / (2 * math.tan(FoV / 2.))          # as render_views forms them for its epilogue
    L = _lib.lib()
    nbytes = L.f3dg_forward_warp_workspace_bytes(B, V, C, W, H)
    if nbytes == 0:
        raise ValueError(f"{who}: unsupported size ({B} x {V} pairs of {C} x {H} x {W}; H * W is at most 2^23)")
    if (workspace is None or workspace.device != dev or workspace.dtype != torch.int64 or not workspace.is_contiguous()
            or workspace.numel() * 8 < nbytes):
        workspace = torch.empty((nbytes + 7) // 8, dtype=torch.int64, device=dev)
    new = lambda planes: torch.empty((B, V, planes, H, W), dtype=torch.float32, device=dev)
    warped, mask = new(C), new(1)
    warped_depth = new(1) if want_depth else None
    weight = new(1) if want_weight else None
    rc = L.f3dg_forward_warp(_stream(), B, V, C, H, W, _lib.ptr(image.detach().contiguous()), _lib.ptr(depth), _lib.ptr(valid), _lib.ptr(rel),
                             float(fx), float(fy), float(z_near), float(depth_tolerance), float(occlusion_min_weight), float(threshold), erode,
                             _lib.ptr(workspace), workspace.numel() * 8, _lib.ptr(warped), _lib.ptr(mask), _lib.ptr(warped_depth),
                             _lib.ptr(weight))
    _lib.check(rc, "f3dg_forward_warp")
    return {"warped": warped, "mask": mask, "warped_depth": warped_depth, "weight": weight, "workspace": workspace}
