"""The frames of the reference's orbit video, composed on the device (visualize.py:403-416).

Per orbit view the reference builds, on the host, one row of five panels per image -- input image, colour-mapped input depth, render,
colour-mapped rendered depth, (depth_normal + 1) / 2 --, lays the images out with torchvision's ``make_grid(nrow=int(sqrt(B)))`` and
truncates to 8 bits. Here ``compose_orbit_frames`` does that in ONE kernel (``f3dg_compose_frames``) that reads ``render_orbit``'s
float32 tensors where they lie and writes finished uint8 HWC frames, into HBM or straight into pinned host memory; the colour range
(``colorize_first``'s numpy percentiles over the whole input-depth batch) is ``depth_range``: torch ops on the device, no host read.
No matplotlib and no torchvision at run time: the reference's only colour map, ``magma_r``, travels with the package as a text table of 256 RGB triples.
"""
import ctypes as C
import math
import os

import numpy as np
import torch

from . import _lib
from .diff_gof_rasterization import _stream

_HERE = os.path.dirname(os.path.abspath(__file__))
_KINDS = {"rgb": _lib.PANEL_RGB, "signed": _lib.PANEL_SIGNED, "colormap": _lib.PANEL_COLORMAP}
_LUT_HOST = {}
_LUT_DEVICE = {}


def colormap_lut(name='magma_r'):
    """uint8 [256, 3] host tensor: the RGB bytes of matplotlib's colour map ``name``, entry i = ``cmap(i, bytes=True)[:3]``.
    ``magma_r`` (what visualize.py:408-410 uses) is read from the package's own table; any other name needs matplotlib."""
    if name not in _LUT_HOST:
        if name == 'magma_r':
            table = np.loadtxt(os.path.join(_HERE, "magma_r_lut.txt"), dtype=np.uint8, comments="#", ndmin=2)
            if table.shape != (256, 3):
                raise RuntimeError("magma_r_lut.txt must hold 256 lines of three byte values")
        else:
            try:
                import matplotlib
            except ImportError as e:
                raise RuntimeError(f"colour map {name!r} needs matplotlib (only 'magma_r' travels with the package)") from e
            cmap = matplotlib.colormaps[name]
            if cmap.N != 256:
                raise RuntimeError(f"colour map {name!r} has {cmap.N} entries; the composer indexes 256")
            table = np.ascontiguousarray(cmap(np.arange(256), bytes=True)[:, :3])
        _LUT_HOST[name] = torch.from_numpy(table.copy())
    return _LUT_HOST[name]


def _device_lut(name, device):
    key = (name, str(device))
    if key not in _LUT_DEVICE:
        _LUT_DEVICE[key] = colormap_lut(name).to(device)
    return _LUT_DEVICE[key]


def _percentile(s, n, q):
    """numpy's linear-interpolated percentile of float32 data, bit for bit: s sorted float32 (valid entries first), n their count (0-d
    int64 tensor), q in percent. numpy divides q by a float32 100 for float32 input, so the virtual index and the lerp are float32."""
    q32 = float(np.float32(q) / np.float32(100))        # a host constant: multiplying by it is a float32 multiply by float32(q32)
    last = torch.clamp(n - 1, min=0)
    vi = last.to(torch.float32) * q32
    lo = torch.floor(vi)
    g = vi - lo
    lo_i = torch.clamp(lo.to(torch.int64), max=last)
    hi_i = torch.clamp(lo_i + 1, max=last)
    # (index_select with a 1-d index: `s[lo_i]` with a 0-d index tensor reads the index back to the host)
    a, b = s.index_select(0, torch.stack([lo_i, hi_i])).unbind(0)
    diff = b - a
    return torch.where(g >= 0.5, b - diff * (1 - g), a + diff * g)


@torch.no_grad()
def depth_range(depth, lo=2, hi=85, invalid_val=-99):
    """float32 [2] = (vmin, vmax) on ``depth``'s device: what ``colorize_first`` (src/utils.py:176-181) takes from
    ``np.percentile(value[value != invalid_val], lo / hi)`` over the whole batch, bit for bit, with no host read: the valid count stays
    on the device and the invalid entries are sorted to the end. NaN when a valid entry is NaN (numpy's answer) or none is valid."""
    d = depth.reshape(-1)
    if d.dtype != torch.float32:
        raise RuntimeError("depth_range needs a float32 tensor")
    valid = d != invalid_val
    n = valid.sum()
    s = torch.sort(torch.where(valid, d, torch.full_like(d, float("inf")))).values
    r = torch.stack([_percentile(s, n, lo), _percentile(s, n, hi)])
    bad = torch.isnan(d).any() | (n == 0)
    return torch.where(bad, torch.full_like(r, float("nan")), r)


def _describe(t, kind, range_index, n_ranges, keep):
    """(Panel, B, V or None, H, W) of one panel tensor, [B, V, C, H, W] or [B, C, H, W] (static: the same on every frame), read in place
    through its strides when its rows are contiguous."""
    if not torch.is_tensor(t) or t.dtype != torch.float32:
        raise RuntimeError("compose_frames needs float32 panels")
    if t.device.type != "cuda":
        raise RuntimeError("compose_frames needs tensors on a HIP device (no CPU fallback)")
    if t.dim() not in (4, 5):
        raise RuntimeError("a panel is [B, V, C, H, W], or [B, C, H, W] for one that is the same on every frame")
    if kind not in _KINDS:
        raise RuntimeError(f"panel kind must be one of {sorted(_KINDS)}")
    H, W = t.shape[-2:]
    if t.stride(-1) != 1 or t.stride(-2) != W or any(s < 0 for s in t.stride()):
        t = t.contiguous()
    keep.append(t)
    planes = t.shape[-3]
    if (kind == "rgb" and planes != 3) or (kind == "signed" and planes not in (1, 3)) or (kind == "colormap" and planes != 1):
        raise RuntimeError(f"a {kind!r} panel cannot have {planes} planes")
    if kind == "colormap" and n_ranges == 0:
        raise RuntimeError("a colormap panel needs `ranges` (float32 [n, 2] on the panels' device)")
    if kind == "colormap" and not 0 <= int(range_index) < n_ranges:
        raise RuntimeError(f"range_index {range_index} outside the {n_ranges} rows of `ranges`")
    V = t.shape[1] if t.dim() == 5 else None
    frame_stride = t.stride(1) if t.dim() == 5 and V > 1 else 0
    p = _lib.Panel(t.data_ptr(), t.stride(0) if t.shape[0] > 1 else 0, frame_stride, t.stride(-3) if planes > 1 else 0,
                   _KINDS[kind], planes, int(range_index) if kind == "colormap" else 0)
    return p, t.shape[0], (None if frame_stride == 0 and (V is None or V == 1) else V), H, W


@torch.no_grad()
def compose_frames(panels, nrow=None, padding=2, lut=None, ranges=None, out=None, max_workgroups=0, invalid_val=-99):
    """``panels``: list of ``(tensor, kind, range_index)`` (at most 8), left to right. tensor: float32 on the HIP device,
    [B, V, C, H, W], or [B, C, H, W] / V == 1 for a panel that is the same on every frame; views and slices are read in place (rows
    contiguous). kind: ``"rgb"`` (3 planes, ``(255 * clip(v, 0, 1))`` truncated), ``"signed"`` (3 planes, or 1 repeated:
    ``(v + 1) / 2`` first), ``"colormap"`` (1 plane through ``lut`` over ``ranges[range_index]`` = (vmin, vmax), the reference's
    ``colorize``; entries equal to ``invalid_val`` are grey). ``lut``: uint8 [256, 3] on the device (None: ``magma_r``); ``ranges``:
    float32 [n, 2] on the device. The B strips are laid out as ``make_grid(nrow, padding)`` does (``nrow=None``: ``int(sqrt(B))``).
    Returns uint8 [V, Hg, Wg, 3]. ``out``: such a tensor to fill, on the device or PINNED on the host (the kernel then writes host
    memory itself, with at most ``max_workgroups`` workgroups, as ``pack_frames`` does)."""
    panels = list(panels)
    if not 1 <= len(panels) <= _lib.MAX_PANELS:
        raise RuntimeError(f"compose_frames takes 1 to {_lib.MAX_PANELS} panels")
    n_ranges = 0
    if ranges is not None:
        if ranges.device.type != "cuda" or ranges.dtype != torch.float32:
            raise RuntimeError("`ranges` must be a float32 tensor on the HIP device")
        ranges = ranges.reshape(-1, 2).contiguous()
        n_ranges = ranges.shape[0]
    keep, desc = [], []
    for item in panels:
        t, kind = item[0], item[1]
        desc.append(_describe(t, kind, item[2] if len(item) > 2 and item[2] is not None else 0, n_ranges, keep))
    device = keep[0].device
    B, H, W = desc[0][1], desc[0][3], desc[0][4]
    Vs = {d[2] for d in desc if d[2] is not None}
    if len(Vs) > 1 or any((d[1], d[3], d[4]) != (B, H, W) for d in desc) or any(t.device != device for t in keep):
        raise RuntimeError("all panels must agree in B, V, H, W and device")
    V = Vs.pop() if Vs else 1
    if any(d[0].kind == _lib.PANEL_COLORMAP for d in desc):
        if ranges is None or ranges.device != device:
            raise RuntimeError("a colormap panel needs `ranges` on the panels' device")
        if lut is None:
            lut = _device_lut('magma_r', device)
        elif lut.device != device or lut.dtype != torch.uint8 or tuple(lut.shape) != (256, 3):
            raise RuntimeError("`lut` must be a uint8 [256, 3] tensor on the panels' device")
        lut = lut.contiguous()
    else:
        lut = ranges = None
    nrow = int(math.sqrt(B)) if nrow is None else int(nrow)
    L = _lib.lib()
    hg, wg, nb = C.c_int(), C.c_int(), C.c_size_t()
    _lib.check(L.f3dg_compose_frames_size(V, B, H, W, nrow, int(padding), len(desc), C.byref(hg), C.byref(wg), C.byref(nb)),
               "f3dg_compose_frames_size")
    Hg, Wg = hg.value, wg.value
    host = 0
    if out is None:
        out = torch.empty((V, Hg, Wg, 3), dtype=torch.uint8, device=device)
    elif out.dtype != torch.uint8 or not out.is_contiguous() or out.numel() != nb.value:
        raise RuntimeError(f"out must be a contiguous uint8 tensor of shape ({V}, {Hg}, {Wg}, 3)")
    elif out.device.type == "cpu":
        if not out.is_pinned():
            raise RuntimeError("a host `out` must be pinned (tensor.pin_memory()): the kernel writes into it")
        host = 1
    elif out.device != device:
        raise RuntimeError(f"out must be on {device} or in pinned host memory")
    table = (_lib.Panel * len(desc))(*[d[0] for d in desc])
    rc = L.f3dg_compose_frames(_stream(), V, B, H, W, nrow, int(padding), len(desc), C.cast(table, C.c_void_p), _lib.ptr(lut),
                               _lib.ptr(ranges), float(invalid_val), _lib.ptr(out), host, int(max_workgroups))
    _lib.check(rc, "f3dg_compose_frames")
    return out.view(V, Hg, Wg, 3)


@torch.no_grad()
def compose_orbit_frames(images, input_depth, orbit, out=None, nrow=None, padding=2, lut=None, invalid_val=-99, max_workgroups=0):
    """The reference's video frames (visualize.py:403-416) from ``render_orbit``'s dict: per image the input image [B, 3, H, W], the
    colour-mapped input depth [B, 1, H, W], ``orbit["render"]``, the colour-mapped ``orbit["rendered_depth"]`` and
    ``(orbit["depth_normal"] + 1) / 2``; both depth panels share ``depth_range(input_depth)`` as at :408-410. uint8
    [num_views, Hg, Wg, 3]; ``out`` / ``max_workgroups`` as in ``compose_frames``."""
    if "depth_normal" not in orbit:
        raise RuntimeError("compose_orbit_frames needs orbit['depth_normal'] (render_orbit(epilogue=True))")
    for t in (images, input_depth):
        if not torch.is_tensor(t) or t.device.type != "cuda":
            raise RuntimeError("compose_orbit_frames needs tensors on a HIP device (no CPU fallback)")
    B, _, H, W = images.shape
    ranges = depth_range(input_depth, invalid_val=invalid_val).reshape(1, 2)
    panels = [(images, "rgb", None), (input_depth.reshape(B, 1, H, W), "colormap", 0), (orbit["render"], "rgb", None),
              (orbit["rendered_depth"], "colormap", 0), (orbit["depth_normal"], "signed", None)]
    return compose_frames(panels, nrow=nrow, padding=padding, lut=lut, ranges=ranges, out=out, max_workgroups=max_workgroups,
                          invalid_val=invalid_val)
