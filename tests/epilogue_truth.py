"""Truth for the render epilogue's backward (f3dg_render_epilogue_backward): a dtype-generic torch restatement of the reference's
post-processing of a rendered frame (src/gaussian_renderer/__init__.py:881-909 depths_to_points / depth_to_normal, :1043-1053 world
normals) -- the same lines ``gaussian_renderer._epilogue_autograd`` restates in float32 -- and the fixtures, the float32 / float64
autograd of that restatement and the tolerance rule the GPU tests share.

Tolerance rule, per channel group (normal = channels 3..5, depth = channel 6) of dL/draster:
    E_ref = max|g32 - g64| / max|g64|     g32 / g64: the restatement's own autograd in float32 / float64 on the CPU
    the kernel passes when max|g_kernel - g64| <= 4 * E_ref * max|g64|
(4: the project's margin for a kernel that orders float32 sums differently from torch)"""
import math

import torch

GROUPS = {"normal": slice(3, 6), "depth": slice(6, 7)}
FOV_DEG = 50.0


def epilogue_torch(raster, world_view, W, H, FoVx, FoVy):
    """raster [9,H,W], world_view [4,4] (row-vector convention), any floating dtype (taken from ``raster``).
    Returns (normal_world [3,H,W], depth_normal [3,H,W])."""
    dtype = raster.dtype
    wv = world_view.reshape(4, 4).to(dtype)
    render_normal = torch.nn.functional.normalize(raster[3:6], p=2, dim=0)
    c2w = (wv.T).inverse()
    normal_world = (c2w[:3, :3] @ render_normal.reshape(3, -1)).reshape(3, *render_normal.shape[1:])
    depth = raster[6:7]
    # depths_to_points (:881-896); the intrinsics are float32 DATA in the reference (``.float()``), whatever the arithmetic's dtype
    fx = W / (2 * math.tan(FoVx / 2.))
    fy = H / (2 * math.tan(FoVy / 2.))
    intrins = torch.tensor([[fx, 0., W / 2.], [0., fy, H / 2.], [0., 0., 1.0]]).float().to(dtype)
    grid_x, grid_y = torch.meshgrid(torch.arange(W).float(), torch.arange(H).float(), indexing='xy')
    points = torch.stack([grid_x, grid_y, torch.ones_like(grid_x)], dim=-1).reshape(-1, 3).to(dtype)
    rays_d = points @ intrins.inverse().T @ c2w[:3, :3].T
    rays_o = c2w[:3, 3]
    points = (depth.reshape(-1, 1) * rays_d + rays_o).reshape(*depth.shape[1:], 3)
    # depth_to_normal (:898-909)
    output = torch.zeros_like(points)
    dx = points[2:, 1:-1] - points[:-2, 1:-1]
    dy = points[1:-1, 2:] - points[1:-1, :-2]
    output[1:-1, 1:-1, :] = torch.nn.functional.normalize(torch.cross(dx, dy, dim=-1), dim=-1)
    return normal_world, output.permute(2, 0, 1)


def rigid_world_view(seed):
    """world_view (row-vector convention: the transpose of the world-to-camera matrix) of a rigid camera: a rotation of about
    0.4 rad about a seeded axis and a seeded translation."""
    gen = torch.Generator().manual_seed(1000 + seed)
    axis = torch.randn(3, generator=gen, dtype=torch.float64)
    axis = axis / axis.norm()
    ang = 0.4 + 0.1 * seed
    K = torch.tensor([[0., -axis[2], axis[1]], [axis[2], 0., -axis[0]], [-axis[1], axis[0], 0.]], dtype=torch.float64)
    R = torch.eye(3, dtype=torch.float64) + math.sin(ang) * K + (1 - math.cos(ang)) * (K @ K)
    M = torch.eye(4, dtype=torch.float64)
    M[:3, :3] = R
    M[:3, 3] = torch.randn(3, generator=gen, dtype=torch.float64) * 0.5 + torch.tensor([0., 0., 2.], dtype=torch.float64)
    return M.T.contiguous().float()


def make_fixture(V, H, W, seed=0):
    """A well-conditioned frame per view: depth 2 + 0.3 sin(0.4 x) cos(0.3 y) + 0.02 noise, accumulated normals 0.5 noise + (0,0,1),
    the other six channels noise; a rigid camera per view; seeded cotangents on both derived maps. float32, on the CPU."""
    gen = torch.Generator().manual_seed(7 + seed)
    raster = torch.randn(V, 9, H, W, generator=gen)
    x = torch.arange(W).float().reshape(1, 1, W)
    y = torch.arange(H).float().reshape(1, H, 1)
    raster[:, 6] = 2.0 + 0.3 * torch.sin(0.4 * x) * torch.cos(0.3 * y) + 0.02 * torch.randn(V, H, W, generator=gen)
    raster[:, 3:6] = 0.5 * torch.randn(V, 3, H, W, generator=gen) + torch.tensor([0., 0., 1.]).reshape(1, 3, 1, 1)
    wv = torch.stack([rigid_world_view(seed * 10 + v) for v in range(V)])
    return {"raster": raster.contiguous(), "world_view": wv.contiguous(), "H": H, "W": W,
            "FoVx": FOV_DEG * math.pi / 180, "FoVy": FOV_DEG * math.pi / 180,
            "g_normal": torch.randn(V, 3, H, W, generator=gen), "g_depth_normal": torch.randn(V, 3, H, W, generator=gen)}


def focal(fx_or_fixture):
    f = fx_or_fixture
    return f["W"] / (2 * math.tan(f["FoVx"] / 2.)), f["H"] / (2 * math.tan(f["FoVy"] / 2.))


def restatement_grads(f, dtype, use_normal=True, use_depth_normal=True):
    """dL/draster [V,9,H,W] (``dtype``) of  sum(normal_world * g_normal) + sum(depth_normal * g_depth_normal)  through the restatement."""
    out = []
    for v in range(f["raster"].shape[0]):
        r = f["raster"][v].to(dtype).requires_grad_()
        nw, dn = epilogue_torch(r, f["world_view"][v], f["W"], f["H"], f["FoVx"], f["FoVy"])
        loss = r.sum() * 0
        if use_normal:
            loss = loss + (nw * f["g_normal"][v].to(dtype)).sum()
        if use_depth_normal:
            loss = loss + (dn * f["g_depth_normal"][v].to(dtype)).sum()
        out.append(torch.autograd.grad(loss, r)[0])
    return torch.stack(out)


def check_groups(got, g32, g64, label=""):
    """Prints E_ref and the kernel's error per channel group, then asserts the tolerance rule. A group whose float64 gradient is
    identically zero must be exactly zero. Returns {group: (E_ref, kernel error relative to max|g64|)}."""
    got = got.detach().double().cpu()
    fig, bad = {}, []
    for name, sl in GROUPS.items():
        m = float(g64[:, sl].abs().max())
        if m == 0.0:
            k = float(got[:, sl].abs().max())
            print(f"{label} {name:6s} max|g64| 0  kernel max {k:.3e}")
            fig[name] = (0.0, k)
            if k != 0.0:
                bad.append((name, k, 0.0))
            continue
        e_ref = float((g32[:, sl].double() - g64[:, sl]).abs().max()) / m
        err = float((got[:, sl] - g64[:, sl]).abs().max()) / m
        print(f"{label} {name:6s} max|g64| {m:.3e}  E_ref {e_ref:.3e}  kernel {err:.3e}  bound {4 * e_ref:.3e}")
        fig[name] = (e_ref, err)
        if not err <= 4 * e_ref:
            bad.append((name, err, e_ref))
    assert not bad, (label, bad)
    return fig
