"""Plain numpy statement of the frame composer's contract (include/f3dg.h, f3dg_compose_frames): colour map, panel rules, grid,
final truncation. Exact: float32 IEEE operations and integer arithmetic only, so a comparison with it is an equality."""
import math

import numpy as np

GREY = np.array([128, 128, 128], dtype=np.uint8)


def to_bytes(v):
    """(uint8)(255 * clip(v, 0, 1)) in float32 with truncation; NaN -> 0 (fmaxf(NaN, 0) = 0)."""
    v = np.asarray(v, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        c = np.where(np.isnan(v), np.float32(0), np.minimum(np.maximum(v, np.float32(0)), np.float32(1))).astype(np.float32)
        return (np.float32(255) * c).astype(np.uint8)


def lut_index(t):
    """(index, kind) of the colour-map rule on float32 t: kind 0 = table entry `index`, 1 = bad (NaN). Under -> 0, over -> 255."""
    t = np.asarray(t, dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        idx = np.where(t < 0, 0, np.where(t >= 1, 255, (np.where(np.isfinite(t), t, np.float32(0)) * np.float32(256)).astype(np.int64)))
    return np.clip(idx, 0, 255), np.isnan(t)


def colorize(d, vmin, vmax, lut, invalid_val=-99.0):
    """float32 depth of any shape -> uint8 [..., 3]."""
    d = np.asarray(d, dtype=np.float32)
    vmin, vmax = np.float32(vmin), np.float32(vmax)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        t = ((d - vmin) / (vmax - vmin)).astype(np.float32) if vmin != vmax else (d * np.float32(0)).astype(np.float32)
    idx, bad = lut_index(t)
    rgb = np.asarray(lut, dtype=np.uint8)[idx]
    rgb[bad] = 0
    rgb[d == np.float32(invalid_val)] = GREY
    return rgb


def panel_bytes(x, kind, vmin=None, vmax=None, lut=None, invalid_val=-99.0):
    """x [B, V, C, H, W] float32 -> uint8 [B, V, H, W, 3]."""
    x = np.asarray(x, dtype=np.float32)
    if kind == "colormap":
        assert x.shape[2] == 1
        return colorize(x[:, :, 0], vmin, vmax, lut, invalid_val)
    if x.shape[2] == 1:
        x = np.repeat(x, 3, axis=2)
    assert x.shape[2] == 3
    if kind == "signed":
        x = ((x + np.float32(1)) / np.float32(2)).astype(np.float32)
    else:
        assert kind == "rgb"
    return np.moveaxis(to_bytes(x), 2, -1)


def grid_shape(B, H, PW, nrow, padding):
    if B == 1:
        return H, PW, 1, 0
    xmaps = min(nrow, B)
    ymaps = -(-B // xmaps)
    return ymaps * (H + padding) + padding, xmaps * (PW + padding) + padding, xmaps, padding


def compose(panels, nrow=None, padding=2, lut=None, ranges=None, invalid_val=-99.0):
    """panels: list of (array [B, V, C, H, W] or static [B, C, H, W], kind, range_index) -> uint8 [V, Hg, Wg, 3]."""
    arrs = [np.asarray(p[0], dtype=np.float32) for p in panels]
    V = max([a.shape[1] for a in arrs if a.ndim == 5] + [1])
    strips = []
    for a, p in zip(arrs, panels):
        if a.ndim == 4:
            a = a[:, None]
        if a.shape[1] == 1 and V > 1:
            a = np.repeat(a, V, axis=1)
        vmin = vmax = None
        if p[1] == "colormap":
            vmin, vmax = np.asarray(ranges, dtype=np.float32).reshape(-1, 2)[p[2]]
        strips.append(panel_bytes(a, p[1], vmin, vmax, lut, invalid_val))
    strip = np.concatenate(strips, axis=3)                     # [B, V, H, P*W, 3]
    B, _, H, PW, _ = strip.shape
    nrow = int(math.sqrt(B)) if nrow is None else nrow
    Hg, Wg, xmaps, pad = grid_shape(B, H, PW, nrow, padding)
    out = np.zeros((V, Hg, Wg, 3), dtype=np.uint8)
    for k in range(B):
        y0, x0 = (k // xmaps) * (H + pad) + pad, (k % xmaps) * (PW + pad) + pad
        out[:, y0:y0 + H, x0:x0 + PW] = strip[k]
    return out


def percentile_f32(values, q):
    """The recipe of frames.depth_range in numpy scalars (float32 throughout)."""
    s = np.sort(np.asarray(values, dtype=np.float32))
    n = s.size
    vi = np.float32(n - 1) * (np.float32(q) / np.float32(100))
    lo = np.floor(vi)
    g = np.float32(vi - lo)
    lo = int(lo)
    hi = min(lo + 1, n - 1)
    a, b = s[lo], s[hi]
    diff = np.float32(b - a)
    return np.float32(b - diff * (np.float32(1) - g)) if g >= 0.5 else np.float32(a + diff * g)
