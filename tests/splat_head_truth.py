"""Differentiable torch restatement of the cycle-aggregative projection ("splat head") -- TEST INFRASTRUCTURE ONLY.

The reference's lines, op for op (src/gaussian_predictor.py: get_pos_from_network_output :857-881, forward :961-1002, transform_rotations
:839-855 with quaternion_raw_multiply :45-64, transform_SHs :821-837 with the matrices of :649-655, flatten_vector :788-791), in the dtype
of ``net_out`` (float32 or float64) and on its device. Its float32 forward is pinned to the reference's fixtures and its float32 gradients
to the reference's own autograd (tests/test_splat_head_backward.py); its float64 autograd is the gradient truth of the backward kernel.
"""
import os

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
KEYS = ("xyz", "opacity", "scaling", "rotation", "features_dc", "features_rest", "unet_depth")
# gradient channel groups of the tolerance rule: six slices of d_net_out [B,23,H,W] and d_depth
GROUPS = {"offset": slice(0, 3), "opacity": slice(3, 4), "scaling": slice(4, 7), "rotation": slice(7, 11), "dc": slice(11, 14),
          "rest": slice(14, 23)}
V_TO_SH = ((0.0, 0.0, -1.0), (-1.0, 0.0, 0.0), (0.0, 1.0, 0.0))


def _flatten(x):
    return x.reshape(x.shape[0], x.shape[1], -1).permute(0, 2, 1)


def splat_head_torch(net_out, depth, ray_dirs, v2w, quat, squre_clip=10000.0):
    dt, dev = net_out.dtype, net_out.device
    B, _, H, W = net_out.shape
    ray_dirs, v2w, quat = ray_dirs.to(dev, dt).reshape(1, 3, H, W), v2w.to(dev, dt).reshape(B, 4, 4), quat.to(dev, dt).reshape(B, 4)
    depth = depth.to(dt)
    offset, opacity, scaling, rotation, fdc, frest = net_out.split([3, 1, 3, 4, 3, 9], dim=1)
    pos = ray_dirs.expand(B, 3, H, W).clone() * depth + offset
    pos = _flatten(pos)
    pos = torch.cat([pos, torch.ones((B, pos.shape[1], 1), device=dev, dtype=dt)], dim=2)
    pos = torch.bmm(pos, v2w)
    pos = pos[:, :, :3] / (pos[:, :, 3:] + 1e-10)
    if squre_clip < 10.0:
        pos[:, :, 0].clamp_(-squre_clip, squre_clip)
        pos[:, :, 1].clamp_(-squre_clip, squre_clip)
    out = {"xyz": pos, "opacity": _flatten(torch.sigmoid(opacity)), "scaling": _flatten(torch.exp(scaling)),
           "features_dc": _flatten(fdc).unsqueeze(2), "unet_depth": _flatten(depth)}
    b = _flatten(F.normalize(rotation))
    a = quat.unsqueeze(1).expand(*b.shape)
    aw, ax, ay, az = torch.unbind(a, -1)
    bw, bx, by, bz = torch.unbind(b, -1)
    out["rotation"] = torch.stack((aw * bw - ax * bx - ay * by - az * bz, aw * bx + ax * bw + ay * bz - az * by,
                                   aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw), -1)
    rest = _flatten(frest)
    rest = rest.reshape(B, rest.shape[1], -1, 3)                                    # b n sh rgb
    v_to_sh = torch.tensor(V_TO_SH, dtype=dt, device=dev).unsqueeze(0).expand(B, 3, 3)
    T = torch.bmm(torch.bmm(v_to_sh.transpose(1, 2), v2w[:, :3, :3]), v_to_sh)
    shs = rest.permute(0, 1, 3, 2).reshape(B, -1, 3)                                # b (n rgb) sh
    out["features_rest"] = torch.bmm(shs, T).reshape(B, -1, 3, 3).permute(0, 1, 3, 2)
    return {k: out[k].contiguous() for k in KEYS}


def restatement_grads(inputs, cots, squre_clip, dtype, device="cpu"):
    """(d_net_out, d_depth) of sum_k <out_k, cots[k]> by the restatement's autograd in ``dtype``; ``cots[k]`` None = output unused."""
    net = inputs["net_out"].detach().to(device, dtype).requires_grad_()
    dep = inputs["depth"].detach().to(device, dtype).requires_grad_()
    out = splat_head_torch(net, dep, inputs["ray_dirs"], inputs["v2w"], inputs["quat"], squre_clip)
    used = [k for k in KEYS if cots.get(k) is not None]
    gn, gd = torch.autograd.grad([out[k] for k in used], [net, dep], [cots[k].to(device, dtype) for k in used], allow_unused=True)
    gn = torch.zeros_like(net) if gn is None else gn
    gd = torch.zeros_like(dep) if gd is None else gd
    return gn.detach(), gd.detach()


def by_group(d_net, d_depth):
    g = {name: d_net[:, sl] for name, sl in GROUPS.items()}
    g["depth"] = d_depth
    return g


def group_bounds(g32, g64):
    """Per group: (E_ref, max|g64|) with E_ref = max|g32 - g64| / max|g64| -- the float32 error of the reference's own autograd."""
    res = {}
    for name, t64 in by_group(*g64).items():
        t32 = by_group(*g32)[name]
        m = float(t64.abs().max())
        res[name] = (float((t32.double().cpu() - t64.cpu()).abs().max()) / m if m > 0 else 0.0, m)
    return res


def check_groups(got, g32, g64, factor=4.0, label="", mask=None):
    """The tolerance rule: per group max|got - g64| <= factor * E_ref * max|g64|. ``mask`` [B,1,H,W] bool: pixels that take part.
    Prints every figure before asserting; returns {group: (E_ref, kernel error relative to max|g64|)}."""
    if mask is not None:
        sel = lambda pair: tuple(torch.where(mask.to(t.device), t, torch.zeros_like(t)) for t in pair)
        got, g32, g64 = sel(got), sel(g32), sel(g64)
    bounds = group_bounds(g32, g64)
    figures, bad = {}, []
    for name, t in by_group(*got).items():
        e_ref, m = bounds[name]
        err = float((t.double().cpu() - by_group(*g64)[name].cpu()).abs().max())
        figures[name] = (e_ref, err / m if m > 0 else err)
        print(f"{label} {name:8s} E_ref {e_ref:.3e}  kernel {figures[name][1]:.3e}  max|g64| {m:.3e}")
        if not (np.isfinite(err) and err <= factor * e_ref * m):
            bad.append((name, figures[name]))
    assert not bad, (label, bad)
    return figures


def load_inputs():
    g = np.load(os.path.join(GOLD, "splat_head.npz"))
    return {k: torch.from_numpy(g[k]) for k in ("net_out", "depth", "ray_dirs", "v2w", "quat")}, g


def load_cotangents():
    g = np.load(os.path.join(GOLD, "splat_head_grad.npz"))
    return {k: torch.from_numpy(g["cot_" + k]) for k in KEYS}, g
