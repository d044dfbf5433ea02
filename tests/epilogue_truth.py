"""Truth for the render epilogue's backward (f3dg_render_epilogue_backward): a dtype-generic torch restatement of the reference's
post-processing of a rendered frame (src/gaussian_renderer/__init__.py:881-909 depths_to_points / depth_to_normal, :1043-1053 world
normals) -- the same lines ``gaussian_renderer._epilogue_autograd`` restates in float32 -- and the fixtures, the float32 / float64
autograd of that restatement and the tolerance rule the GPU tests share.

Tolerance rule, per channel group (normal = channels 3..5, depth = channel 6) of dL/draster:
    E_ref = max|g32 - g64| / max|g64|     g32 / g64: the restatement's own autograd in float32 / float64 on the CPU
    the kernel passes when max|g_kernel - g64| <= 4 * E_ref * max|g64|
(4: the project's margin for a kernel that orders float32 sums differently from torch)

The second half is the truth of the FORWARD kernels (f3dg_render_epilogue_view, f3dg_render_epilogue): the float64 forward on the call's own
inputs, the error scale of every element, the condition number of every depth normal and the cases both forward test files share."""
import math
import os

import numpy as np
import torch

GROUPS = {"normal": slice(3, 6), "depth": slice(6, 7)}
FOV_DEG = 50.0


def epilogue_torch(raster, world_view, W, H, FoVx, FoVy, c2w=None):
    """raster [9,H,W], world_view [4,4] (row-vector convention), any floating dtype (taken from ``raster``).
    Returns (normal_world [3,H,W], depth_normal [3,H,W]). ``c2w`` [4,4]: the camera-to-world matrix handed in as data, in place of the
    inverse of ``world_view``'s transpose (the form of f3dg_render_epilogue; ``world_view`` is then not read)."""
    dtype = raster.dtype
    render_normal = torch.nn.functional.normalize(raster[3:6], p=2, dim=0)
    c2w = (world_view.reshape(4, 4).to(dtype).T).inverse() if c2w is None else c2w.reshape(4, 4).to(dtype)
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


# ------------------------------------------------------------------------------------------------ the forward against float64
# ("the epilogue's forward against float64"; figure and bars: tests/forward_bars.py)
K_GROUPS = ("normal_world", "depth_normal")
COND_MIN = 64.0                 # a pixel whose cross product is conditioned worse is fragile: float32 cannot determine the direction
# float32 roundings on the longest chain to an element, each at most 2^-24 of the scale -- the a-priori bound of K for a correct float32
# evaluation whose camera-to-world matrix is one rounding from the float64 one (what the kernels form), to first order:
#   normal_world  |n|^2: 1 + 2, halved by the root, root 1, division 1 -> 3.5 on n^; C's rounding 1, product 1, two additions
#   depth_normal  pixel coordinate 2, C 1, products 1, two additions: 6 on the ray; x depth 1, + origin 1: 8 on a point, 9 on a
#                 difference, 9 + 9 + 1 + 1 on a component of the cross product -- in units of A_c, which holds every one of these
#                 terms, so in units of the scale |A_c|/|c| + 1 the sum is at most 20, + the normalisation's 4
OP_COUNT = {"normal_world": 7.5, "depth_normal": 24.0}
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def c2w_truth(world_view):
    """float64 inverse of world_view^T, [V,4,4]: the camera-to-world matrix of f3dg_render_epilogue_view's truth."""
    return torch.linalg.inv(world_view.double().reshape(-1, 4, 4).transpose(1, 2))


def focal32(W, H, FoVx, FoVy):
    """(fx, fy) as the float32 values the C call receives, as Python floats."""
    return float(np.float32(W / (2 * math.tan(FoVx / 2.)))), float(np.float32(H / (2 * math.tan(FoVy / 2.))))


def forward_truth(raster, Cw, fx, fy):
    """float64 forward of the epilogue on the call's own inputs: raster [V,9,H,W] float32, ``Cw`` [V,4,4] float64 camera-to-world
    (``c2w_truth(world_view)``, or the float32 c2w handed to f3dg_render_epilogue, as data), ``fx`` / ``fy`` from ``focal32``.
    Returns {"out": {group: [V,3,H,W]}, "A": {"normal_world": per element, "depth_normal": per pixel [V,1,H,W]}, "cond" [V,1,H,W],
    "interior", "zero_class", "fragile": bool [V,1,H,W]}. The float32 literal 1e-12 stands at its own value."""
    import forward_bars as FB
    r = raster.detach().cpu().double()
    V, _, H, W = r.shape
    eps = float(np.float32(1e-12))
    a = r[:, 3:6]
    nh = a / a.norm(dim=1, keepdim=True).clamp_min(eps)
    R = Cw[:, :3, :3]
    out = {"normal_world": torch.einsum("vij,vjhw->vihw", R, nh)}
    A = {"normal_world": torch.einsum("vij,vjhw->vihw", R.abs(), nh.abs())}
    ax, bx, ay, by = 1.0 / fx, -(W / 2.0) / fx, 1.0 / fy, -(H / 2.0) / fy
    xs, ys = torch.arange(W, dtype=torch.float64).reshape(1, 1, 1, W), torch.arange(H, dtype=torch.float64).reshape(1, 1, H, 1)
    col = lambda j: R[:, :, j].reshape(V, 3, 1, 1)
    ray = (xs * ax + bx) * col(0) + (ys * ay + by) * col(1) + col(2)
    A_ray = ((xs * ax).abs() + abs(bx)) * col(0).abs() + ((ys * ay).abs() + abs(by)) * col(1).abs() + col(2).abs()
    d, o = r[:, 6:7], Cw[:, :3, 3].reshape(V, 3, 1, 1)
    p, A_p = d * ray + o, d.abs() * A_ray + o.abs()
    zeros = lambda *s: torch.zeros(*s, dtype=torch.float64)
    dn, scale, cond = zeros(V, 3, H, W), torch.ones(V, 1, H, W, dtype=torch.float64), torch.full((V, 1, H, W), float("inf"), dtype=torch.float64)
    interior = torch.zeros(V, 1, H, W, dtype=torch.bool)
    zero_class = torch.zeros(V, 1, H, W, dtype=torch.bool)
    if H >= 3 and W >= 3:
        interior[:, :, 1:-1, 1:-1] = True
        e, A_e = p[:, :, 2:, 1:-1] - p[:, :, :-2, 1:-1], A_p[:, :, 2:, 1:-1] + A_p[:, :, :-2, 1:-1]
        g, A_g = p[:, :, 1:-1, 2:] - p[:, :, 1:-1, :-2], A_p[:, :, 1:-1, 2:] + A_p[:, :, 1:-1, :-2]
        c = torch.cross(e, g, dim=1)
        i1, i2 = [1, 2, 0], [2, 0, 1]             # c_i = e_i1 g_i2 - e_i2 g_i1: the product rule, term by term
        A_c = A_e[:, i1] * g[:, i2].abs() + e[:, i1].abs() * A_g[:, i2] + A_e[:, i2] * g[:, i1].abs() + e[:, i2].abs() * A_g[:, i1]
        cn, Acn = c.norm(dim=1, keepdim=True), A_c.norm(dim=1, keepdim=True)
        dn[:, :, 1:-1, 1:-1] = c / cn.clamp_min(eps)
        zc = (d[:, :, 2:, 1:-1] == 0) & (d[:, :, :-2, 1:-1] == 0) & (d[:, :, 1:-1, 2:] == 0) & (d[:, :, 1:-1, :-2] == 0)
        zero_class[:, :, 1:-1, 1:-1] = zc
        scale[:, :, 1:-1, 1:-1] = torch.where(cn > 0, Acn / cn, torch.full_like(cn, float("inf"))) + 1.0
        cond[:, :, 1:-1, 1:-1] = cn / (FB.U24 * Acn)
    out["depth_normal"], A["depth_normal"] = dn, scale
    return {"out": out, "A": A, "cond": cond, "interior": interior, "zero_class": zero_class,
            "fragile": interior & ~zero_class & (cond < COND_MIN)}


def forward_K(nw, dn, tr, label=""):
    """K of an implementation's (normal_world, depth_normal) [V,3,H,W] (either may be None) against ``forward_truth``'s result.
    Returns ({group: 1-D K over the ordinary elements / pixels}, [messages of broken exactness and special-value rules])."""
    import forward_bars as FB
    ks, bad = {}, []
    if nw is not None:
        x, t, A = nw.detach().cpu(), tr["out"]["normal_world"], tr["A"]["normal_world"]
        sel = torch.ones_like(t, dtype=torch.bool)
        bad += FB.special_failures(x, t, A, sel, f"{label} normal_world")      # a zero accumulated normal: scale 0, exactly 0
        ks["normal_world"] = FB.k_of(x, t, A, sel)
    if dn is not None:
        x, t = dn.detach().cpu().double(), tr["out"]["depth_normal"]
        exact0 = (~tr["interior"] | tr["zero_class"]).expand_as(x)
        if not bool((x[exact0] == 0).all()):
            bad.append(f"{label} depth_normal: a border pixel or a pixel whose four neighbour depths are 0 is not exactly 0")
        held = (tr["interior"] & ~tr["zero_class"] & ~tr["fragile"])[:, 0]
        err = (x - t).abs().amax(dim=1)                                          # the max-norm of the 3-vector's error
        k = err[held] / (FB.U24 * tr["A"]["depth_normal"][:, 0][held])
        ks["depth_normal"] = torch.where(torch.isfinite(k), k, torch.full_like(k, float("inf")))
    return ks, bad


def restatement32(case, given_c2w=False):
    """The float32 restatement on a case, view by view: (normal_world, depth_normal) [V,3,H,W]. ``given_c2w``: the case's float32
    ``c2w`` handed in as data (f3dg_render_epilogue's form) instead of the float32 inverse of ``world_view``."""
    outs = [epilogue_torch(case["raster"][v], case["world_view"][v], case["W"], case["H"], case["FoVx"], case["FoVy"],
                           c2w=case["c2w"][v] if given_c2w else None) for v in range(case["raster"].shape[0])]
    return torch.stack([o[0] for o in outs]), torch.stack([o[1] for o in outs])


def _diamond(H, W, cy, cx, radius):
    y, x = torch.arange(H).reshape(H, 1), torch.arange(W).reshape(1, W)
    return ((y - cy).abs() + (x - cx).abs()) <= radius


_CASES = None


def forward_cases():
    """{name: case}: ``make_fixture``'s keys plus "c2w" (float32: the float64 inverse of world_view^T rounded once -- the data of the
    f3dg_render_epilogue calls) and "pooled" (an ordinary case: its K enters the pooled bars). Built once, never modified."""
    global _CASES
    if _CASES is not None:
        return _CASES
    deg = math.pi / 180
    cases = {"20x35": make_fixture(3, 20, 35), "3x3": make_fixture(1, 3, 3), "2x5": make_fixture(1, 2, 5)}
    f = make_fixture(2, 17, 33, seed=1)                     # FoVx != FoVy with W != H
    f["FoVx"], f["FoVy"] = 60 * deg, 35 * deg
    cases["17x33_fov"] = f
    g = np.load(os.path.join(GOLD, "renderer_post.npz"))
    cases["golden64"] = {"raster": torch.from_numpy(g["raster"]).unsqueeze(0).contiguous(), "world_view": torch.from_numpy(g["wv"]).reshape(1, 4, 4),
                         "H": 64, "W": 64, "FoVx": 13.164 * deg, "FoVy": 13.164 * deg}
    f = make_fixture(2, 17, 33, seed=2)                     # a far camera: translation about 1e3, the scene ten times deeper
    f["world_view"] = f["world_view"].clone()
    f["world_view"][:, 3, :3] = torch.tensor([[700., -400., 900.], [-1000., 300., 500.]])
    f["raster"][:, 6] *= 10.0
    cases["far"] = f
    f = make_fixture(1, 17, 33, seed=6)                     # a small scene seen from the origin: cross products of about 1e-10, far under
    f["world_view"] = f["world_view"].clone()               # 1e-6 and far above the normalisation's 1e-12 (as well conditioned as the others)
    f["world_view"][:, 3, :3] = 0.0
    f["raster"][:, 6] *= 1e-4
    cases["small_scene"] = f
    f = make_fixture(3, 20, 35, seed=3)                     # background: depth exactly 0 on a diamond per view (its inside: the exact-zero
    for v, (cy, cx, rad) in enumerate(((6, 9, 2), (12, 25, 3), (9, 17, 1))):      # class; its rim: ordinary pixels with one or two zero neighbours)
        f["raster"][v, 6][_diamond(20, 35, cy, cx, rad)] = 0.0
    cases["background"] = f
    f = make_fixture(3, 20, 35, seed=4)                     # degenerate accumulated normals: exactly 0, and of length about 1e-20
    n = torch.arange(20 * 35).reshape(20, 35)
    f["raster"][:, 3:6] = torch.where((n % 13 == 0).reshape(1, 1, 20, 35), torch.zeros(()), f["raster"][:, 3:6])
    f["raster"][:, 3:6] = torch.where((n % 13 == 5).reshape(1, 1, 20, 35), f["raster"][:, 3:6] * 1e-20, f["raster"][:, 3:6])
    cases["degenerate"] = f
    for name, c in cases.items():
        c["c2w"] = c2w_truth(c["world_view"]).float().contiguous()
        c["pooled"] = name != "degenerate"
    _CASES = cases
    return cases


_TRUTHS = {}


def case_truth(name, given_c2w=False):
    """(forward_truth, the float32 restatement's K, its broken rules, its outputs) of a case and entry-point form: computed once."""
    key = (name, given_c2w)
    if key not in _TRUTHS:
        c = forward_cases()[name]
        Cw = c["c2w"].double() if given_c2w else c2w_truth(c["world_view"])
        tr = forward_truth(c["raster"], Cw, *focal32(c["W"], c["H"], c["FoVx"], c["FoVy"]))
        with torch.no_grad():
            r32 = restatement32(c, given_c2w)
        ks, bad = forward_K(r32[0], r32[1], tr, f"restatement {name}")
        _TRUTHS[key] = (tr, ks, bad, r32)
    return _TRUTHS[key]
