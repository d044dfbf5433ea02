"""Which Gaussians matter: per-Gaussian contribution statistics of rendered views, and the pruning of a set by them
(csrc/f3dg_contribution.hip, include/f3dg.h).

    stats = gaussian_contribution(pc, bs, world_views, full_projs, centers, bg, cfg)        # over all the views that will be rendered
    pruned, kept_ids = prune_gaussians(pc, bs, stats)                                       # touched >= 1: exact renders stay bit-identical
    out = render_views(pruned, 0, world_views, full_projs, centers, bg, cfg)

For a pair (pixel, entry of its tile list), walked front to back from T = 1 in the reference's arithmetic: a pair that is not skipped
(t <= 0.2, alpha < 1/255, pixel done) either STOPS the pixel (T (1 - alpha) < 1e-4: counted in ``stops``) or is BLENDED with weight
w = alpha T (counted in ``blended``, ``max_weight``, ``sum_weight``). ``touched = blended + stops``: a Gaussian that is never blended may
still be the one that ends a pixel's walk, so pruning goes by ``touched``. Integer sums and a maximum only: every statistic is
bit-reproducible whatever the lists, the path, the chunking of the views or the arithmetic of the forward.
"""
import ctypes as C
import math

import numpy as np
import torch

from . import _lib
from .diff_gof_rasterization import _stream, rasterize_views

RECORD_WORDS = 8                 # 32 bytes per Gaussian: u64 sum_fixed, u64 blended | stops << 32, u32 max_bits, u32 pad[3]
MAX_PIXELS = 1 << 31             # views x W x H that one array may accumulate (each counter then fits 32 bits, the sum 63)
MAX_ARRAYS = 8


def _require_hip(*tensors):
    for t in tensors:
        if t is not None and t.device.type != "cuda":
            raise RuntimeError("f3dgaus_amd contribution statistics need tensors on a HIP device (no CPU fallback)")


class GaussianContribution:
    """The statistics of P Gaussians: ``raw`` [P,8] int32 (the library's 32-byte records, added into by every call), the views and
    pixels accumulated so far, and the readable columns."""

    def __init__(self, P, device):
        self.raw = torch.zeros((int(P), RECORD_WORDS), dtype=torch.int32, device=device)
        self.views = 0
        self.pixels = 0

    @property
    def P(self):
        return self.raw.shape[0]

    def _i64(self):
        return self.raw.view(torch.int64)                 # [P,4]: sum_fixed, counts, max_bits | pad, pad

    @property
    def sum_fixed(self):
        return self._i64()[:, 0]

    @property
    def sum_weight(self):
        """float64: the fixed-point sum over 2^32 (exact below 2^21; beyond, the nearest float64)."""
        return self._i64()[:, 0].to(torch.float64) / 4294967296.0

    @property
    def blended(self):
        return self._i64()[:, 1] & 0xFFFFFFFF

    @property
    def stops(self):
        return (self._i64()[:, 1] >> 32) & 0xFFFFFFFF

    @property
    def touched(self):
        return self.blended + self.stops

    @property
    def max_weight(self):
        return self.raw[:, 4].contiguous().view(torch.float32)


def _check_stats(stats, P, device):
    if not isinstance(stats, GaussianContribution):
        raise RuntimeError("stats must be a GaussianContribution")
    r = stats.raw
    if r.dtype != torch.int32 or tuple(r.shape) != (int(P), RECORD_WORDS) or not r.is_contiguous() or (r.numel() and r.data_ptr() % 32):
        raise RuntimeError(f"stats.raw must be a contiguous, 32-byte aligned int32 tensor of shape ({int(P)}, {RECORD_WORDS}), got {tuple(r.shape)}")
    if r.device != device:
        raise RuntimeError(f"stats live on {r.device}, the Gaussians on {device}")


def contribution_raw(workspace, P, W, H, n_views, tanfovx, tanfovy, stats=None, final_T=None):
    """f3dg_contribution on the workspace a ``rasterize_views`` call of (n_views, P, W, H) left (inference or save_aux, any arithmetic,
    culled lists or not, either path; one Gaussian set). Adds into ``stats`` (a fresh GaussianContribution when None) and returns it;
    ``final_T`` [n_views,H,W] float32, when given, receives every pixel's transmittance at the end of its walk."""
    P, W, H, n_views = int(P), int(W), int(H), int(n_views)
    device = workspace.buffer.device
    _require_hip(workspace.buffer)
    if getattr(workspace, "n_sets", 1) != 1:
        raise RuntimeError("contribution statistics of a several-sets call are not served")
    if (workspace.P, workspace.W, workspace.H, workspace.n_views) != (P, W, H, n_views):
        raise RuntimeError(f"the workspace's last call was (P, W, H, n_views) = {(workspace.P, workspace.W, workspace.H, workspace.n_views)}, "
                           f"not {(P, W, H, n_views)}")
    if stats is None:
        stats = GaussianContribution(P, device)
    _check_stats(stats, P, device)
    if stats.pixels + n_views * W * H >= MAX_PIXELS:
        raise RuntimeError(f"one statistics array accumulates fewer than 2^31 pixels (views x W x H); this call would make it {stats.pixels + n_views * W * H}")
    if final_T is not None and (final_T.dtype != torch.float32 or final_T.device != device or not final_T.is_contiguous() or
                                final_T.numel() != n_views * H * W):
        raise RuntimeError(f"final_T must be a contiguous float32 tensor of shape ({n_views}, {H}, {W}) on {device}")
    rc = _lib.lib().f3dg_contribution(_stream(), C.c_void_p(workspace.buffer.data_ptr()), workspace.nbytes, workspace.max_rendered, n_views, P, W, H,
                                      float(tanfovx), float(tanfovy), _lib.ptr(stats.raw), _lib.ptr(final_T))
    _lib.check(rc, "f3dg_contribution")
    stats.views += n_views
    stats.pixels += n_views * W * H
    return stats


def _set_of(pc, bs):
    get = (lambda k: pc[k][bs]) if isinstance(pc, dict) else (lambda k: pc[bs][k])
    keys = list(pc.keys()) if isinstance(pc, dict) else list(pc[bs].keys())
    return get, keys


def gaussian_contribution(pc, bs, world_views, full_projs, centers, bg, cfg, views_per_call=32, stats=None, kernel_size=0.0,
                          scaling_modifier=1.0, override_color=None):
    """The statistics of image ``bs`` of the Gaussian dict ``pc`` over all the given cameras: the views are rendered ``views_per_call`` at
    a time (inference calls, default lists, as ``render_views`` renders them) and every call's workspace goes through
    ``contribution_raw``. Adds into ``stats`` when given. The result does not depend on ``views_per_call``."""
    get, _ = _set_of(pc, bs)
    xyz = get("xyz")
    _require_hip(xyz)
    if int(views_per_call) < 1:
        raise RuntimeError("views_per_call must be at least 1")
    P = xyz.shape[0]
    if stats is not None:
        _check_stats(stats, P, xyz.device)
    tanfov = math.tan(cfg['model']['fov'] * np.pi / 360)
    res = int(cfg['model']['training_resolution'])
    wv, fp, cc = world_views.reshape(-1, 4, 4), full_projs.reshape(-1, 4, 4), centers.reshape(-1, 3)
    V = wv.shape[0]
    if fp.shape[0] != V or cc.shape[0] != V:
        raise RuntimeError("world_views, full_projs and centers must agree on the number of views")
    if stats is None:
        stats = GaussianContribution(P, xyz.device)
    if override_color is None:
        shs, colors = torch.cat([get("features_dc"), get("features_rest")], dim=1).contiguous(), None
    else:
        shs, colors = None, get("rgbs")
    step = int(views_per_call)
    ws = None
    with torch.no_grad():
        for v0 in range(0, V, step):
            n = min(step, V - v0)
            if ws is not None and ws.n_views != n:
                ws = None
            _, _, ws = rasterize_views(xyz, get("opacity"), wv[v0:v0 + n], fp[v0:v0 + n], cc[v0:v0 + n], bg, image_height=res, image_width=res,
                                       tanfovx=tanfov, tanfovy=tanfov, sh=shs, colors_precomp=colors, scales=get("scaling"),
                                       rotations=get("rotation"), sh_degree=cfg['model']['max_sh_degree'], scale_modifier=scaling_modifier,
                                       kernel_size=kernel_size, workspace=ws, channels="rgb_depth_alpha")
            contribution_raw(ws, P, res, res, n, tanfov, tanfov, stats=stats)
    return stats


def prune_gaussians(pc, bs, stats=None, *, keep=None, min_touched=1, min_max_weight=None, min_sum_weight=None):
    """The Gaussians of image ``bs`` of ``pc`` that pass every given test, in their input order:
    ``touched >= min_touched``, ``max_weight >= min_max_weight``, ``sum_weight >= min_sum_weight`` (of ``stats``; inclusive; None: no
    such test) and ``keep[i] != 0`` (``keep``: [P] bool / uint8). Returns ``(pruned, kept_ids)``: ``pruned`` has the keys of ``pc`` with
    values [1,K,...] -- every renderer takes it with ``bs=0`` --, ``kept_ids`` [K] int32 ascending. With ``min_touched=1`` alone an exact
    render of the views the statistics cover is bit-identical to the full set's. K = 0 is legal."""
    if stats is None and keep is None:
        raise RuntimeError("prune_gaussians needs statistics (stats=) or an explicit mask (keep=)")
    get, keys = _set_of(pc, bs)
    xyz = get("xyz")
    _require_hip(xyz, keep)
    device = xyz.device
    P = xyz.shape[0]
    arrays = []
    for k in keys:
        t = get(k)
        if t.shape[0] != P:
            raise RuntimeError(f"pc[{k!r}] holds {t.shape[0]} Gaussians, pc['xyz'] {P}")
        if t.dtype != torch.float32 or t.device != device:
            raise RuntimeError(f"pc[{k!r}] must be a float32 tensor on {device}")
        arrays.append((k, t.contiguous()))
    if len(arrays) > MAX_ARRAYS:
        raise RuntimeError(f"at most {MAX_ARRAYS} arrays are gathered in one call, pc has {len(arrays)}")
    if stats is not None:
        _check_stats(stats, P, device)
    if keep is not None:
        if keep.numel() != P or keep.dtype not in (torch.bool, torch.uint8):
            raise RuntimeError(f"keep must be a bool or uint8 tensor of {P} elements, got {keep.dtype} {tuple(keep.shape)}")
        keep = keep.reshape(-1).to(torch.uint8).contiguous()
    min_touched = int(min_touched) if (stats is not None and min_touched is not None) else 0
    if min_touched < 0:
        raise RuntimeError("min_touched must not be negative")
    mmw = 0.0 if min_max_weight is None else float(min_max_weight)
    msw = 0.0 if min_sum_weight is None else float(min_sum_weight)
    if math.isnan(mmw) or math.isnan(msw):
        raise RuntimeError("a threshold is NaN")

    L = _lib.lib()
    K = 0
    ws = None
    if P > 0:
        ws = torch.empty(int(L.f3dg_gaussian_compact_workspace_bytes(P)), dtype=torch.uint8, device=device)
        n = C.c_longlong(0)
        rc = L.f3dg_gaussian_compact_count(_stream(), C.c_void_p(ws.data_ptr()), ws.numel(), P, _lib.ptr(stats.raw) if stats is not None else None,
                                           _lib.ptr(keep), min_touched, mmw, msw, C.byref(n))
        _lib.check(rc, "f3dg_gaussian_compact_count")
        K = int(n.value)
    kept_ids = torch.empty((K,), dtype=torch.int32, device=device)
    outs = [(k, torch.empty((1, K) + tuple(t.shape[1:]), dtype=torch.float32, device=device)) for k, t in arrays]
    if K > 0:
        widths = [int(t[0].numel()) for _, t in arrays]
        gather = [i for i, w in enumerate(widths) if w > 0]
        na = len(gather)
        srcs = (C.c_void_p * max(na, 1))(*[arrays[i][1].data_ptr() for i in gather])
        dsts = (C.c_void_p * max(na, 1))(*[outs[i][1].data_ptr() for i in gather])
        rows = (C.c_int * max(na, 1))(*[widths[i] for i in gather])
        rc = L.f3dg_gaussian_compact_emit(_stream(), C.c_void_p(ws.data_ptr()), ws.numel(), P, K, na, srcs, dsts, rows, C.c_void_p(kept_ids.data_ptr()))
        _lib.check(rc, "f3dg_gaussian_compact_emit")
    return dict(outs), kept_ids
