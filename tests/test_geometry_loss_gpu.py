"""GPU tests of the fused geometry losses: f3dg_geometry_loss_forward / f3dg_geometry_loss_backward through ctypes and through
f3dgaus_amd.losses. Truth and the tolerance rules are tests/geometry_loss_truth.py: sums against the float64 restatement within its own
float32 error (x 4) plus the worst case of a float32 summation order; gradients by ``epilogue_truth.check_groups`` (kernel <= 4 E_ref)
on channels 3..5 and 6, every other channel exact. Every figure is printed before it is asserted (``pytest -s``).

Shapes (F, H, W): (2, 19, 37) ragged in both axes; (3, 17, 33) one pixel past a 32 x 16 tile each way; (1, 3, 5) a single interior row;
(1, 2, 7) no interior pixel (D = 0 everywhere). Every frame has at most 1024 pixels."""
import ctypes as C

import pytest
import torch

import f3dgaus_amd as f3d
from f3dgaus_amd import _lib, losses
import epilogue_truth as E
import geometry_loss_truth as T

pytestmark = pytest.mark.gpu
SHAPES = [(2, 19, 37), (3, 17, 33), (1, 3, 5), (1, 2, 7)]
CFG = {"model": {"fov": E.FOV_DEG}}
TARGETS = ("depth_target", "normal_target", "alpha_target")
_CACHE = {}


def _truth(f, aw, skip=(), frame_weights=None):
    return dict(t32=T.per_pixel(f, torch.float32, aw, skip), t64=T.per_pixel(f, torch.float64, aw, skip),
                g32=T.grads(f, torch.float32, aw, skip, frame_weights), g64=T.grads(f, torch.float64, aw, skip, frame_weights))


def _case(shape, aw):
    """(fixture, truth) of a shape: computed once, shared, never modified."""
    key = (shape, bool(aw))
    if key not in _CACHE:
        f = T.make_fixture(*shape)
        _CACHE[key] = (f, _truth(f, aw))
    return _CACHE[key]


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _dev(f, dev, skip=()):
    pick = lambda name: None if (name in skip or f.get(name) is None) else f[name].to(dev).contiguous()
    return dict(raster=f["raster"].to(dev).contiguous(), wv=f["world_view"].to(dev).contiguous(), depth_target=pick("depth_target"),
                normal_target=pick("normal_target"), alpha_target=pick("alpha_target"), mask=pick("mask"))


def _raw_forward(f, dev, aw, skip=()):
    """f3dg_geometry_loss_forward; the sums start as NaN, so an element the kernels skip shows."""
    F, _, H, W = f["raster"].shape
    fx, fy = E.focal(f)
    d = _dev(f, dev, skip)
    L = _lib.lib()
    nbytes = L.f3dg_geometry_loss_partials_bytes(F, W, H)
    partials = torch.full((nbytes // 4,), float("nan"), device=dev)
    sums = torch.full((F, 5), float("nan"), device=dev)
    rc = L.f3dg_geometry_loss_forward(_stream(), F, H, W, _lib.ptr(d["raster"]), _lib.ptr(d["wv"]), float(fx), float(fy), 1 if aw else 0,
                                      _lib.ptr(d["depth_target"]), _lib.ptr(d["normal_target"]), _lib.ptr(d["alpha_target"]), _lib.ptr(d["mask"]),
                                      _lib.ptr(partials), nbytes, _lib.ptr(sums))
    assert rc == _lib.OK, rc
    torch.cuda.synchronize()
    return sums


def _raw_backward(f, dev, aw, skip=(), frame_weights=None):
    """f3dg_geometry_loss_backward; dL_draster starts as NaN: the kernel ASSIGNS every element."""
    F, _, H, W = f["raster"].shape
    fx, fy = E.focal(f)
    d = _dev(f, dev, skip)
    fw = (f["frame_weights"] if frame_weights is None else frame_weights).to(dev).contiguous()
    out = torch.full((F, 9, H, W), float("nan"), device=dev)
    rc = _lib.lib().f3dg_geometry_loss_backward(_stream(), F, H, W, _lib.ptr(d["raster"]), _lib.ptr(d["wv"]), float(fx), float(fy), 1 if aw else 0,
                                                _lib.ptr(d["depth_target"]), _lib.ptr(d["normal_target"]), _lib.ptr(d["alpha_target"]),
                                                _lib.ptr(d["mask"]), _lib.ptr(fw), _lib.ptr(out))
    assert rc == _lib.OK, rc
    torch.cuda.synchronize()
    return out


def _api(f, dev, aw, skip=(), frame_weights=None, grad=True):
    """(sums, raster.grad) through losses.geometry_sums with L = sum(frame_weights * sums)."""
    d = _dev(f, dev, skip)
    r = d["raster"].clone().requires_grad_(grad)
    sums = losses.geometry_sums(r, d["wv"].reshape(-1, 4, 4), CFG, alpha_weight=aw, depth_target=d["depth_target"], normal_target=d["normal_target"],
                                alpha_target=d["alpha_target"], mask=d["mask"])
    if not grad:
        return sums, None
    fw = (f["frame_weights"] if frame_weights is None else frame_weights).to(dev)
    (sums * fw).sum().backward()
    torch.cuda.synchronize()
    return sums.detach(), r.grad


def _exact_channels(got, f, shape, skip=()):
    """Channels 0..2, 7 and 8 (and 6 where no pixel is interior) against their closed forms, to the bit."""
    got = got.cpu()
    fw = f["frame_weights"]
    assert float(got[:, :3].abs().max()) == 0.0
    assert torch.equal(got[:, 8], fw[:, 1].reshape(-1, 1, 1).expand_as(got[:, 8]))
    ch7 = fw[:, 4].reshape(-1, 1, 1) * torch.sign(f["raster"][:, 7] - f["alpha_target"]) if "alpha_target" not in skip else torch.zeros_like(got[:, 7])
    assert torch.equal(got[:, 7], ch7)
    if shape[1] < 3:
        m = f["mask"] if "mask" not in skip else torch.ones_like(f["mask"])
        assert torch.equal(got[:, 6], (fw[:, 2].reshape(-1, 1, 1) * m) * torch.sign(f["raster"][:, 6] - f["depth_target"]))


@pytest.mark.parametrize("aw", [False, True])
@pytest.mark.parametrize("shape", SHAPES)
def test_sums_against_the_float64_restatement(gpu_device, shape, aw):
    f, t = _case(shape, aw)
    got = _raw_forward(f, gpu_device, aw)
    T.check_sums(got, t["t32"], t["t64"], label=f"sums {shape} aw={aw}")
    if shape[1] < 3:        # D = 0 everywhere: term 0 is the sum of the weights
        w = f["raster"][:, 7].double() if aw else torch.ones_like(f["raster"][:, 7]).double()
        _, bound = T.sum_bounds(t["t32"], t["t64"])
        assert abs(float(got[0, 0]) - float(w.sum())) <= float(bound[0, 0])
    api, _ = _api(f, gpu_device, aw, grad=False)
    assert torch.equal(api, got)


@pytest.mark.parametrize("aw", [False, True])
@pytest.mark.parametrize("shape", SHAPES)
def test_gradients_against_the_float64_restatement(gpu_device, shape, aw):
    f, t = _case(shape, aw)
    got = _raw_backward(f, gpu_device, aw)
    assert bool(torch.isfinite(got).all())
    E.check_groups(got, t["g32"], t["g64"], label=f"C ABI {shape} aw={aw}")
    _exact_channels(got, f, shape)
    _, api = _api(f, gpu_device, aw)
    E.check_groups(api, t["g32"], t["g64"], label=f"losses.geometry_sums {shape} aw={aw}")
    _exact_channels(api, f, shape)
    assert torch.equal(api, got)
    if shape[1] >= 3:       # the gather reaches border pixels, never a corner (no interior axial neighbour): there the sign term alone
        corner = got[:, 6, 0, 0].cpu()
        assert torch.equal(corner, (f["frame_weights"][:, 2] * f["mask"][:, 0, 0]) * torch.sign(f["raster"][:, 6, 0, 0] - f["depth_target"][:, 0, 0]))


@pytest.mark.parametrize("name", TARGETS)
def test_a_skipped_term_is_zero_and_its_weight_is_zero(gpu_device, name):
    shape, aw = SHAPES[0], True
    f, _ = _case(shape, aw)
    k = 2 + TARGETS.index(name)
    sums = _raw_forward(f, gpu_device, aw, skip=(name,))
    full = _raw_forward(f, gpu_device, aw)
    assert float(sums[:, k].abs().max()) == 0.0 and float(full[:, k].abs().min()) > 0.0
    others = [c for c in range(5) if c != k]
    assert torch.equal(sums[:, others], full[:, others])
    fw0 = f["frame_weights"].clone()
    fw0[:, k] = 0.0
    skipped = _raw_backward(f, gpu_device, aw, skip=(name,))
    zeroed = _raw_backward(f, gpu_device, aw, frame_weights=fw0)
    assert bool(torch.isfinite(skipped).all()) and torch.equal(skipped, zeroed)
    assert not torch.equal(skipped, _raw_backward(f, gpu_device, aw))
    _, api = _api(f, gpu_device, aw, skip=(name,))
    assert torch.equal(api, skipped)


def test_no_mask_is_a_mask_of_ones(gpu_device):
    f0, _ = _case(SHAPES[0], False)
    f = dict(f0)
    f["mask"] = torch.ones_like(f0["mask"])
    assert torch.equal(_raw_forward(f, gpu_device, False), _raw_forward(f0, gpu_device, False, skip=("mask",)))
    assert torch.equal(_raw_backward(f, gpu_device, False), _raw_backward(f0, gpu_device, False, skip=("mask",)))


def test_clamp_and_ties(gpu_device):
    """A pixel whose accumulated normal is exactly 0 (F.normalize's clamp active: n^ = 0, terms 0 and 3 are w and m, the gradient is
    g / 1e-12); depth and alpha targets that equal the rendered values at chosen pixels (sign(0) = 0)."""
    shape, aw = SHAPES[0], True
    f0, _ = _case(shape, aw)
    f = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in f0.items()}
    zv, zy, zx = 1, 7, 12
    f["raster"][zv, 3:6, zy, zx] = 0.0
    f["mask"][zv, zy, zx] = 1.0
    ties = [(0, 5, 9), (1, 0, 0), (1, 18, 36), (0, 9, 20)]
    for v, y, x in ties:
        f["depth_target"][v, y, x] = f["raster"][v, 6, y, x]
        f["alpha_target"][v, y, x] = f["raster"][v, 7, y, x]
    t = _truth(f, aw)
    for t_ in (t["t32"], t["t64"]):
        assert float(t_[zv, 0, zy, zx]) == float(f["raster"][zv, 7, zy, zx]) and float(t_[zv, 3, zy, zx]) == 1.0
        for v, y, x in ties:
            assert float(t_[v, 2, y, x]) == 0.0 and float(t_[v, 4, y, x]) == 0.0
    T.check_sums(_raw_forward(f, gpu_device, aw), t["t32"], t["t64"], label="clamp/ties sums")
    got = _raw_backward(f, gpu_device, aw)
    assert bool(torch.isfinite(got).all())
    keep = torch.ones_like(t["g64"], dtype=torch.bool)
    keep[zv, 3:6, zy, zx] = False
    others = lambda x: torch.where(keep, x.double().cpu(), torch.zeros((), dtype=torch.float64))
    E.check_groups(others(got), others(t["g32"]), others(t["g64"]), label="clamp/others")       # the ordinary pixels, the 1e12-scaled values taken out
    p64, p32, pk = t["g64"][zv, 3:6, zy, zx], t["g32"][zv, 3:6, zy, zx].double(), got[zv, 3:6, zy, zx].double().cpu()
    m = float(p64.abs().max())
    e_ref, err = float((p32 - p64).abs().max()) / m, float((pk - p64).abs().max()) / m
    print(f"clamp pixel: max|g64| {m:.3e}  E_ref {e_ref:.3e}  kernel {err:.3e}  bound {4 * e_ref:.3e}")
    assert m > 1e10 and err <= 4 * e_ref, (m, err, e_ref)
    _exact_channels(got, f, shape)
    no_depth = _raw_backward(f, gpu_device, aw, skip=("depth_target",))
    for v, y, x in ties:    # a zero sign contribution: the alpha gradient vanishes, the depth gradient is the gather alone
        assert float(got[v, 7, y, x]) == 0.0
        assert float(got[v, 6, y, x]) == float(no_depth[v, 6, y, x])
    assert float(got[1, 6, 0, 0]) == 0.0 and float(got[1, 6, 18, 36]) == 0.0            # tied corners: nothing at all


def test_isolation_and_determinism(gpu_device):
    shape, aw = SHAPES[1], True
    f, _ = _case(shape, aw)
    s, g = _raw_forward(f, gpu_device, aw), _raw_backward(f, gpu_device, aw)
    assert torch.equal(s, _raw_forward(f, gpu_device, aw)) and torch.equal(g, _raw_backward(f, gpu_device, aw))
    bad = dict(f)
    bad["raster"] = f["raster"].clone()
    bad["raster"][1, 6, 8, 16] = float("nan")
    sb, gb = _raw_forward(bad, gpu_device, aw), _raw_backward(bad, gpu_device, aw)
    assert bool(torch.isnan(sb[1, 0])) and bool(torch.isnan(gb[1]).any())
    for fr in (0, 2):
        assert torch.equal(sb[fr], s[fr]) and torch.equal(gb[fr], g[fr])
    alone = {k: (v[1:2].contiguous() if torch.is_tensor(v) else v) for k, v in f.items()}
    assert torch.equal(_raw_forward(alone, gpu_device, aw)[0], s[1]) and torch.equal(_raw_backward(alone, gpu_device, aw)[0], g[1])


def test_plumbing(gpu_device):
    dev = gpu_device
    F, H, W = 4, 5, 7
    f = T.make_fixture(F, H, W, seed=2)
    d = _dev(f, dev)
    fw = f["frame_weights"].to(dev)
    kw = dict(alpha_weight=True, depth_target=d["depth_target"], normal_target=d["normal_target"], alpha_target=d["alpha_target"], mask=d["mask"])
    ref_s, ref_g = _api(f, dev, True)
    # a non-contiguous raster view against its contiguous copy
    big = torch.randn(F, 11, H, W + 3, generator=torch.Generator().manual_seed(1)).to(dev)
    big[:, 1:10, :, 2:2 + W] = d["raster"]
    big.requires_grad_()
    view = big[:, 1:10, :, 2:2 + W]
    assert not view.is_contiguous()
    s = losses.geometry_sums(view, d["wv"], CFG, **kw)
    (s * fw).sum().backward()
    assert torch.equal(s.detach(), ref_s) and torch.equal(big.grad[:, 1:10, :, 2:2 + W], ref_g)
    assert float(big.grad[:, 0].abs().max()) == 0.0 and float(big.grad[:, 10].abs().max()) == 0.0
    # [B, V, 9, H, W]: per-frame losses, and the [V] cameras repeated image-major
    B, V = 2, 2
    f2 = dict(f)
    f2["world_view"] = f["world_view"][:V].repeat(B, 1, 1)
    d2 = _dev(f2, dev)
    r5 = d2["raster"].reshape(B, V, 9, H, W)
    kw5 = {k: (v.reshape((B, V) + tuple(v.shape[1:])) if torch.is_tensor(v) else v) for k, v in kw.items()}
    s_full = losses.geometry_sums(r5, d2["wv"].reshape(B * V, 4, 4), CFG, **kw5)
    s_bcast = losses.geometry_sums(r5, d2["wv"][:V], CFG, **kw5)
    assert s_full.shape == (B * V, 5) and torch.equal(s_full, s_bcast) and not torch.equal(s_full, ref_s)
    ws = dict(w_depth_normal=0.7, w_distortion=0.1, w_depth=0.5, w_normal=0.2, w_alpha=1.0)
    none = losses.geometry_loss(r5, d2["wv"][:V], CFG, reduction="none", **ws, **kw5)
    mean = losses.geometry_loss(r5, d2["wv"][:V], CFG, **ws, **kw5)
    assert none.shape == (B, V) and mean.dim() == 0
    wvec = torch.tensor(list(ws.values()), dtype=torch.float64, device=dev)
    want = (s_full.double() @ wvec) / (H * W)
    mag = (s_full.double().abs() @ wvec) / (H * W)          # the blend is ~10 float32 roundings per frame on terms of this size; twice that
    assert bool(((none.reshape(-1).double() - want).abs() <= 16 * 2.0 ** -24 * mag).all())          # for the mean over the frames
    assert abs(float(mean) - float(want.mean())) <= 32 * 2.0 ** -24 * float(mag.mean())
    # the single-term wrappers are columns of the same sums (F adds and a divide in float32)
    n = B * V * H * W
    close = lambda a, col: abs(float(a) - float(col.double().sum()) / n) <= 8 * 2.0 ** -24 * float(col.double().abs().sum()) / n
    assert close(losses.normal_consistency(r5, d2["wv"][:V], CFG, alpha_weight=True), s_full[:, 0])
    assert close(losses.distortion_loss(r5), s_full[:, 1])
    assert close(losses.depth_loss(r5, kw5["depth_target"], mask=kw5["mask"]), s_full[:, 2])
    # no_grad: the same value, no graph, the forward's two launches only
    L = _lib.lib()
    leaf = d["raster"].clone().requires_grad_()
    with torch.no_grad():
        L.f3dg_debug_launch_count(1)
        s_ng = losses.geometry_sums(leaf, d["wv"], CFG, **kw)
        assert int(L.f3dg_debug_launch_count(1)) == 2
    assert s_ng.grad_fn is None and not s_ng.requires_grad and torch.equal(s_ng, ref_s)
    L.f3dg_debug_launch_count(1)
    (losses.geometry_sums(leaf, d["wv"], CFG, **kw) * fw).sum().backward()
    assert int(L.f3dg_debug_launch_count(1)) == 3 and torch.equal(leaf.grad, ref_g)
    # a side stream
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        leaf2 = d["raster"].clone().requires_grad_()
        s_side = losses.geometry_sums(leaf2, d["wv"], CFG, **kw)
        (s_side * fw).sum().backward()
    side.synchronize()
    torch.cuda.current_stream().wait_stream(side)
    assert torch.equal(s_side.detach(), ref_s) and torch.equal(leaf2.grad, ref_g)


def test_render_views_into_the_loss(gpu_device):
    """predictor-shaped Gaussians -> render_views(differentiable=True) -> geometry_loss on out["raster"] -> backward: 1 set x 2 views at
    64 x 64, all five weights, the alpha weight, and a mask that keeps empty pixels out of the 1e-12 clamp regime."""
    from f3dgaus_amd import synthetic
    dev = gpu_device
    cam = synthetic.orbit_cameras(8, 64, device=dev)
    g = synthetic.make_gaussians(400, s0=0.05, seed=5, device=dev)
    leaves = {k: v.unsqueeze(0).clone().requires_grad_() for k, v in g.items()}                # one set: [1, P, ...]
    cams = tuple(cam[k][[1, 5]].contiguous() for k in ("viewmatrix", "projmatrix", "campos"))
    cfg = cam["cfg"]
    out = f3d.render_views(leaves, None, *cams, torch.tensor([0.2, 0.5, 0.3], device=dev), cfg, differentiable=True)
    raster = out["raster"]
    raster.retain_grad()
    F, _, H, W = raster.shape
    gen = torch.Generator().manual_seed(8)
    mask = (out["rendered_alpha"] > 0.5).detach()
    depth_t = (out["rendered_depth"].detach().cpu() + 0.1 * torch.randn(F, 1, H, W, generator=gen)).to(dev)
    normal_t = torch.nn.functional.normalize(torch.randn(F, 3, H, W, generator=gen), dim=1).to(dev)
    alpha_t = (torch.rand(F, 1, H, W, generator=gen) < 0.5).float().to(dev)
    ws = dict(w_depth_normal=0.7, w_distortion=0.1, w_depth=0.5, w_normal=0.2, w_alpha=1.0)
    loss = losses.geometry_loss(raster, cams[0], cfg, alpha_weight=True, depth_target=depth_t, normal_target=normal_t, alpha_target=alpha_t,
                                mask=mask, **ws)
    loss.backward()
    for k, t in leaves.items():          # the terms read no colour plane (dL/draster is 0 on channels 0..2): the colour leaves get exactly nothing
        assert t.grad is not None and bool(torch.isfinite(t.grad).all()), k
        assert (float(t.grad.abs().max()) == 0.0) if k.startswith("features") else (float(t.grad.abs().max()) > 0), k
    fov = cfg["model"]["fov"] * torch.pi / 180
    f = {"raster": raster.detach().cpu(), "world_view": cams[0].reshape(F, 4, 4).cpu(), "H": H, "W": W, "FoVx": fov, "FoVy": fov,
         "depth_target": depth_t[:, 0].cpu(), "normal_target": normal_t.cpu(), "alpha_target": alpha_t[:, 0].cpu(), "mask": mask[:, 0].float().cpu(),
         "frame_weights": (torch.tensor(list(ws.values())) / (F * H * W)).float().repeat(F, 1)}
    t = _truth(f, True)
    with torch.no_grad():
        sums = losses.geometry_sums(raster, cams[0], cfg, alpha_weight=True, depth_target=depth_t, normal_target=normal_t, alpha_target=alpha_t,
                                    mask=mask)
    T.check_sums(sums, t["t32"], t["t64"], label="render_views -> geometry_sums")
    got = raster.grad
    assert bool(torch.isfinite(got).all())
    E.check_groups(got, t["g32"], t["g64"], label="render_views -> geometry_loss")
    _exact_channels(got, f, (F, H, W))
