"""GPU tests of the forward warp and the masked L1: f3dg_forward_warp / f3dg_masked_l1_forward / _backward through ctypes, and
f3dgaus_amd.warp.forward_warp / losses.warping_sums / warping_loss. Truth, fixture, fragile-pixel rule and tolerances are
tests/warp_truth.py: weight, warped * weight and warped_depth * weight within 4 E_ref + n_max q of the float64 restatement on non-fragile
pixels, the mask exact outside the threshold margin and the fragile set. Outputs start as NaN, so an element a kernel skips shows.
Every figure is printed before it is asserted (``pytest -s``).

Shapes (B, V, H, W): (2, 4, 19, 37) ragged in both axes; (2, 4, 33, 17) one past a 32 x 16 tile; (1, 2, 16, 16); (1, 1, 3, 5)."""
import ctypes as C

import pytest
import torch

from f3dgaus_amd import _lib, losses, warp
import warp_truth as T

pytestmark = pytest.mark.gpu
L1_SHAPES = [(2, 19, 37), (3, 17, 33), (1, 3, 5)]


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _nan(dev, *shape):
    return torch.full(shape, float("nan"), device=dev)


def _raw_warp(c, dev, erode=0, want_depth=True, want_weight=True, rel=None, **params):
    """f3dg_forward_warp on a case's fixture and rel; outputs and workspace start as NaN / garbage."""
    f = c["f"]
    B, Cn, H, W = f["image"].shape
    rel = (c["rel"] if rel is None else rel).to(dev).contiguous()
    V = rel.shape[1]
    fx, fy = T.focal(H, W)
    p = {**T.DEFAULTS, **params}
    L = _lib.lib()
    nbytes = L.f3dg_forward_warp_workspace_bytes(B, V, Cn, W, H)
    assert nbytes > 0
    ws = torch.full(((nbytes + 7) // 8,), -0x0123456789ABCDEF, dtype=torch.int64, device=dev)
    image, depth = f["image"].to(dev), f["depth"].to(dev)
    valid = f["valid"].to(dev) if c["use_valid"] else None
    out = {"warped": _nan(dev, B, V, Cn, H, W), "mask": _nan(dev, B, V, 1, H, W), "warped_depth": _nan(dev, B, V, 1, H, W) if want_depth else None,
           "weight": _nan(dev, B, V, 1, H, W) if want_weight else None}
    rc = L.f3dg_forward_warp(_stream(), B, V, Cn, H, W, _lib.ptr(image), _lib.ptr(depth), _lib.ptr(valid), _lib.ptr(rel), fx, fy, p["z_near"],
                             p["depth_tolerance"], p["occlusion_min_weight"], p["threshold"], erode, _lib.ptr(ws), ws.numel() * 8,
                             _lib.ptr(out["warped"]), _lib.ptr(out["mask"]), _lib.ptr(out["warped_depth"]), _lib.ptr(out["weight"]))
    assert rc == _lib.OK, rc
    torch.cuda.synchronize()
    return out


def _api_warp(c, dev, **kw):
    f = c["f"]
    valid = f["valid"].to(dev) if c["use_valid"] else None
    out = warp.forward_warp(f["image"].to(dev), f["depth"].to(dev), f["src_world_view"].to(dev), c["dst"].to(dev), T.CFG, valid=valid, **kw)
    torch.cuda.synchronize()
    return out


def _same(a, b, keys=("warped", "mask", "warped_depth", "weight")):
    return all(torch.equal(a[k], b[k]) for k in keys if a.get(k) is not None and b.get(k) is not None)


@pytest.mark.parametrize("use_valid", [True, False])
@pytest.mark.parametrize("shape", T.GPU_SHAPES)
def test_c_abi_against_the_float64_restatement(gpu_device, shape, use_valid):
    c = T.case(shape, use_valid=use_valid)
    assert c["fragile_share"] <= T.FRAGILE_CAP
    plain = _raw_warp(c, gpu_device)
    T.check_outputs(plain, c, label=f"C ABI {shape} valid={use_valid}")
    for k in (3, 5):            # erosion changes the mask and nothing else
        got = _raw_warp(c, gpu_device, erode=k)
        T.check_outputs(got, c, erode=k, label=f"C ABI {shape} valid={use_valid} erode {k}")
        assert _same(got, plain, keys=("warped", "warped_depth", "weight"))
        assert bool((got["mask"] <= plain["mask"]).all())
    assert _same(_raw_warp(c, gpu_device, erode=1), plain)


@pytest.mark.parametrize("shared", [False, True])
@pytest.mark.parametrize("shape", T.GPU_SHAPES)
def test_forward_warp_against_the_float64_restatement(gpu_device, shape, shared):
    """Per-image [B,V,4,4] and shared [V,4,4] target cameras through warp.forward_warp (rel formed on the device in float64)."""
    c = T.case(shape, shared=shared)
    assert c["fragile_share"] <= T.FRAGILE_CAP
    f = c["f"]
    rel = warp.relative_transforms(f["src_world_view"].to(gpu_device), c["dst"].to(gpu_device))
    d = float((rel.cpu() - c["rel"]).abs().max())
    print(f"{shape} shared={shared}: |rel(device) - rel(truth)| {d:.3e}")
    assert d <= 2.0 ** -22           # two float32 ulps of entries below 8: both are float64 products rounded once
    got = _api_warp(c, gpu_device, want_weight=True, erode=5)
    assert got["warped"].shape == (shape[0], shape[1], 3, shape[2], shape[3]) and got["mask"].shape == (shape[0], shape[1], 1, shape[2], shape[3])
    T.check_outputs(got, c, erode=5, label=f"forward_warp {shape} shared={shared}")
    if d == 0.0:
        assert _same(got, _raw_warp(c, gpu_device, erode=5))


def test_one_channel(gpu_device):
    c = T.case(T.GPU_SHAPES[0], C=1)
    got = _raw_warp(c, gpu_device, erode=3)
    T.check_outputs(got, c, erode=3, label="C = 1")
    api = _api_warp(c, gpu_device, want_weight=True, erode=3)
    assert api["warped"].shape[2] == 1
    T.check_outputs(api, c, erode=3, label="C = 1, forward_warp")


def test_identity_view_returns_the_frame(gpu_device):
    """Target 0 is the source camera. Without special pixels the mask is all ones and warped = image: with |Csum - image| <= b_C,
    |Wsum - 1| <= b_W and |image| <= 1, |Csum / Wsum - image| <= (b_C + b_W) / (1 - b_W)."""
    c = T.case((1, 2, 16, 16), special=False)
    f, b = c["f"], T.bounds(c)
    for got in (_raw_warp(c, gpu_device), _api_warp(c, gpu_device, want_weight=True)):
        assert bool((got["mask"][:, 0] == 1).all())
        err = float((got["warped"][:, 0].cpu().double() - f["image"].double()).abs().max())
        errz = float((got["warped_depth"][:, 0, 0].cpu().double() - f["depth"].double()).abs().max())
        lim, limz = (b["Csum"] + b["Wsum"]) / (1 - b["Wsum"]), (b["Zsum"] + b["Wsum"] * float(f["depth"].max())) / (1 - b["Wsum"])
        print(f"identity: |warped - image| {err:.3e} (bound {lim:.3e})  |warped_depth - depth| {errz:.3e} (bound {limz:.3e})")
        assert err <= lim and errz <= limz
    # with dead source pixels: the identity mask is the live map
    for shape in T.GPU_SHAPES:
        cs = T.case(shape)
        got = _raw_warp(cs, gpu_device)
        live = T.live_map(cs["f"]).double()
        ok = ~cs["fragile"][:, 0]
        assert torch.equal(got["mask"][:, 0, 0].cpu().double()[ok], live[ok])


def test_bitwise_reproducible_and_optional_outputs(gpu_device):
    c = T.case(T.GPU_SHAPES[0])
    a, b = _raw_warp(c, gpu_device, erode=5), _raw_warp(c, gpu_device, erode=5)
    assert _same(a, b) and all(a[k] is not None for k in ("warped", "mask", "warped_depth", "weight"))
    lean = _raw_warp(c, gpu_device, erode=5, want_depth=False, want_weight=False)
    assert lean["warped_depth"] is None and lean["weight"] is None and _same(lean, a, keys=("warped", "mask"))
    x, y = _api_warp(c, gpu_device, erode=5, want_weight=True), _api_warp(c, gpu_device, erode=5, want_weight=True)
    assert _same(x, y)
    z = _api_warp(c, gpu_device, erode=5, want_depth=False)
    assert z["warped_depth"] is None and z["weight"] is None and _same(z, x, keys=("warped", "mask"))
    # the workspace of one call serves the next (whatever it holds), also after a call of another shape wrote over its start
    again = _api_warp(c, gpu_device, erode=5, want_weight=True, workspace=x["workspace"])
    assert again["workspace"] is x["workspace"] and _same(again, x)
    small = T.case(T.GPU_SHAPES[2])
    s1 = _api_warp(small, gpu_device, want_weight=True)
    s2 = _api_warp(small, gpu_device, want_weight=True, workspace=x["workspace"])
    assert s2["workspace"] is x["workspace"] and _same(s1, s2)
    assert _api_warp(c, gpu_device, workspace=s1["workspace"])["workspace"] is not s1["workspace"]          # too small: a new one
    # a side stream
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        on_side = _api_warp(c, gpu_device, erode=5, want_weight=True)
    side.synchronize()
    torch.cuda.current_stream().wait_stream(side)
    assert _same(on_side, x)
    # no_grad inputs that require grad elsewhere are data here
    with torch.no_grad():
        leaf = c["f"]["image"].to(gpu_device).requires_grad_()
        out = warp.forward_warp(leaf, c["f"]["depth"].to(gpu_device), c["f"]["src_world_view"].to(gpu_device), c["dst"].to(gpu_device), T.CFG,
                                valid=c["f"]["valid"].to(gpu_device), erode=5, want_weight=True)
    assert not out["warped"].requires_grad and _same(out, x)


def test_launch_counts(gpu_device):
    c = T.case(T.GPU_SHAPES[2])
    L = _lib.lib()
    L.f3dg_debug_launch_count(1)
    _raw_warp(c, gpu_device)
    assert int(L.f3dg_debug_launch_count(1)) == 4           # fill, z-buffer, accumulate, resolve: all pairs at once
    _raw_warp(c, gpu_device, erode=5)
    assert int(L.f3dg_debug_launch_count(1)) == 5


def test_unprojectable_targets_touch_nothing(gpu_device):
    """Target coordinates are range-checked as floating-point numbers before any conversion to int: pairs whose transform sends every point
    to +-huge, +-Inf or NaN coordinates, behind the camera or far off the image leave weight 0, mask 0 and zeros; the other pairs of the
    same call are untouched by them."""
    c = T.case(T.GPU_SHAPES[0])
    good = _raw_warp(c, gpu_device)
    rel = c["rel"].clone()
    eye = torch.eye(4)
    huge, nanm, behind, off = eye.clone(), eye.clone(), eye.clone(), eye.clone()
    huge[3, 0], huge[3, 1] = 3e38, -3e38                    # u, v = +-1e39 / z: beyond int
    nanm[0, 0], nanm[3, 2] = float("nan"), float("inf")
    behind[3, 2] = -1e4                                     # z < z_near everywhere
    off[3, 0] = 1e3                                         # finite, far right of the image
    rel[0, 0], rel[0, 1], rel[1, 2], rel[1, 3] = huge, nanm, behind, off
    got = _raw_warp(c, gpu_device, rel=rel)
    for k, v in got.items():
        assert bool(torch.isfinite(v).all()), k
    for (b, v) in ((0, 0), (0, 1), (1, 2), (1, 3)):
        for k in ("warped", "mask", "warped_depth", "weight"):
            assert float(got[k][b, v].abs().max()) == 0.0, (b, v, k)
    for (b, v) in ((0, 2), (0, 3), (1, 0), (1, 1)):
        for k in ("warped", "mask", "warped_depth", "weight"):
            assert torch.equal(got[k][b, v], good[k][b, v]), (b, v, k)


def test_threshold_and_cfg(gpu_device):
    """``threshold`` defaults to cfg['model']['threshold'] (0.9 without one); the mask is weight >= threshold."""
    c = T.case(T.GPU_SHAPES[1])
    f = c["f"]
    args = (f["image"].to(gpu_device), f["depth"].to(gpu_device), f["src_world_view"].to(gpu_device), c["dst"].to(gpu_device))
    base = warp.forward_warp(*args, T.CFG, valid=f["valid"].to(gpu_device), want_weight=True)
    bare = warp.forward_warp(*args, {"model": {"fov": T.FOV_DEG}}, valid=f["valid"].to(gpu_device), want_weight=True)
    low = warp.forward_warp(*args, {"model": {"fov": T.FOV_DEG, "threshold": 0.5}}, valid=f["valid"].to(gpu_device), want_weight=True)
    arg = warp.forward_warp(*args, T.CFG, valid=f["valid"].to(gpu_device), want_weight=True, threshold=0.5)
    assert _same(base, bare) and _same(low, arg) and torch.equal(low["weight"], base["weight"])
    assert torch.equal(low["mask"], (low["weight"].double() >= float(torch.tensor(0.5))).float())
    assert float(low["mask"].sum()) > float(base["mask"].sum())
    boolean = warp.forward_warp(*args, T.CFG, valid=f["valid"].to(gpu_device) > 0, want_weight=True)
    assert _same(boolean, base)


# ------------------------------------------------------------------------------------------------ masked L1
_L1 = {}


def _l1_case(shape, Cn=3):
    """(a, b, m, t32, t64): seeded inputs with a ~70 % mask and a few exact ties; the per-element terms m |a - b| in both precisions."""
    if shape not in _L1:
        F, H, W = shape
        gen = torch.Generator().manual_seed(77 + H)
        a, b = torch.rand(F, Cn, H, W, generator=gen), torch.rand(F, Cn, H, W, generator=gen)
        m = (torch.rand(F, 1, H, W, generator=gen) < 0.7).float()
        b[:, :, 1, 2] = a[:, :, 1, 2]
        m[:, :, 1, 2] = 1.0
        t32 = m * (a - b).abs()
        t64 = m.double() * (a.double() - b.double()).abs()
        _L1[shape] = (a, b, m, t32, t64)
    return _L1[shape]


def _raw_l1_forward(a, b, m, dev):
    F, Cn, H, W = a.shape
    L = _lib.lib()
    nbytes = L.f3dg_masked_l1_partials_bytes(F, Cn, W, H)
    partials, sums = _nan(dev, nbytes // 4), _nan(dev, F, 2)
    a, b, m = a.to(dev), b.to(dev), m.to(dev)           # (named: a temporary's memory would be handed to the next one)
    rc = L.f3dg_masked_l1_forward(_stream(), F, Cn, H, W, _lib.ptr(a), _lib.ptr(b), _lib.ptr(m), _lib.ptr(partials), nbytes, _lib.ptr(sums))
    assert rc == _lib.OK, rc
    torch.cuda.synchronize()
    return sums


def _raw_l1_backward(a, b, m, fw, dev):
    F, Cn, H, W = a.shape
    out = _nan(dev, F, Cn, H, W)
    a, b, m, fw = a.to(dev), b.to(dev), m.to(dev), fw.to(dev).contiguous()
    rc = _lib.lib().f3dg_masked_l1_backward(_stream(), F, Cn, H, W, _lib.ptr(a), _lib.ptr(b), _lib.ptr(m), _lib.ptr(fw), _lib.ptr(out))
    assert rc == _lib.OK, rc
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("shape", L1_SHAPES)
def test_masked_l1_sums(gpu_device, shape):
    """The rule of tests/geometry_loss_truth.py: |s - s64| <= 4 sum |t32 - t64| + N 2^-24 sum |t64|, N the number of summed elements."""
    a, b, m, t32, t64 = _l1_case(shape)
    F, H, W = shape
    got = _raw_l1_forward(a, b, m, gpu_device).double().cpu()
    s64 = torch.stack([t64.sum((1, 2, 3)), m.double().sum((1, 2, 3))], 1)
    n0, n1 = 3 * H * W, H * W
    bound = torch.stack([4 * (t32.double() - t64).abs().sum((1, 2, 3)) + n0 * 2.0 ** -24 * t64.sum((1, 2, 3)), n1 * 2.0 ** -24 * m.double().sum((1, 2, 3))], 1)
    for f in range(F):
        for k in range(2):
            print(f"masked L1 {shape} frame {f} col {k}: s64 {float(s64[f, k]):.6e}  kernel err {abs(float(got[f, k] - s64[f, k])):.3e}  bound {float(bound[f, k]):.3e}")
    assert bool(((got - s64).abs() <= bound).all())
    assert torch.equal(got[:, 1], s64[:, 1])                # a count below 2^24: exact in any order
    dev = gpu_device
    api = losses.warping_sums(a.to(dev), b.to(dev), m.to(dev))
    assert torch.equal(api.double().cpu(), got) and torch.equal(_raw_l1_forward(a, b, m, dev).double().cpu(), got)
    assert torch.equal(losses.warping_sums(a.to(dev), b.to(dev), m.to(dev)[:, 0] > 0).double().cpu(), got)           # [F,H,W] bool mask


@pytest.mark.parametrize("shape", L1_SHAPES)
def test_masked_l1_backward_is_exact(gpu_device, shape):
    a, b, m, _, _ = _l1_case(shape)
    F, H, W = shape
    dev = gpu_device
    gen = torch.Generator().manual_seed(5)
    fw = torch.randn(F, 2, generator=gen)
    want = (fw[:, 0].reshape(F, 1, 1, 1) * m) * torch.sign(a - b)
    got = _raw_l1_backward(a, b, m, fw, dev)
    assert bool(torch.isfinite(got).all()) and torch.equal(got.cpu(), want)
    assert float(got[:, :, 1, 2].abs().max()) == 0.0                         # ties: sign(0) = 0
    # through autograd: the cotangent of the sums is the kernel's weight
    leaf = a.to(dev).requires_grad_()
    sums = losses.warping_sums(leaf, b.to(dev), m.to(dev))
    (sums * fw.to(dev)).sum().backward()
    assert torch.equal(leaf.grad.cpu(), want)
    # warping_loss: the mean over all F C H W elements; its gradient is m sign / (F C H W)
    leaf2 = a.to(dev).requires_grad_()
    loss = losses.warping_loss(leaf2, b.to(dev), m.to(dev))
    loss.backward()
    n = F * 3 * H * W
    g = (torch.tensor(1.0) / n).reshape(1, 1).expand(F, 2)
    assert torch.equal(leaf2.grad, _raw_l1_backward(a, b, m, g, dev))
    t64 = m.double() * (a.double() - b.double()).abs()
    t32 = (m * (a - b).abs()).double()
    sum_bound = float(4 * (t32 - t64).abs().sum() + n * 2.0 ** -24 * t64.sum())            # the sums' rule, then F adds and a divide in float32
    assert abs(float(loss.detach()) - float(t64.sum()) / n) <= sum_bound / n + 8 * 2.0 ** -24 * float(t64.sum()) / n
    # a mask of zeros: a zero gradient, no NaN
    leaf3 = a.to(dev).requires_grad_()
    zero = losses.warping_loss(leaf3, b.to(dev), torch.zeros_like(m).to(dev))
    zero.backward()
    assert float(zero.detach()) == 0.0 and bool(torch.isfinite(leaf3.grad).all()) and float(leaf3.grad.abs().max()) == 0.0


def test_warping_loss_plumbing(gpu_device):
    """[B, V, C, H, W] inputs as forward_warp returns them, reduction='none', a non-contiguous render, no_grad, launch counts."""
    dev = gpu_device
    c = T.case(T.GPU_SHAPES[0])
    B, V, H, W = T.GPU_SHAPES[0]
    w = _api_warp(c, dev, erode=3)
    gen = torch.Generator().manual_seed(11)
    base = torch.rand(B, V, 5, H, W + 2, generator=gen).to(dev).requires_grad_()
    render = base[:, :, 1:4, :, 1:1 + W]
    assert not render.is_contiguous()
    flat = losses.warping_sums(render.reshape(B * V, 3, H, W), w["warped"], w["mask"])          # render_views' [B * V, ...] against [B, V, ...]
    per = losses.warping_loss(render, w["warped"], w["mask"], reduction="none")
    mean = losses.warping_loss(render, w["warped"], w["mask"])
    assert per.shape == (B, V) and mean.dim() == 0
    sums = losses.warping_sums(render, w["warped"], w["mask"])
    assert sums.shape == (B * V, 2) and torch.equal(sums[:, 1].reshape(B, V), w["mask"].sum((2, 3, 4)))
    assert torch.equal(per.reshape(-1), sums[:, 0] / float(3 * H * W)) and torch.equal(flat, sums)
    mean.backward()
    n = B * V * 3 * H * W
    want = (torch.tensor(1.0, device=dev) / n * w["mask"]) * torch.sign(render.detach() - w["warped"])
    assert torch.equal(base.grad[:, :, 1:4, :, 1:1 + W], want)
    assert float(base.grad[:, :, 0].abs().max()) == 0.0 and float(base.grad[:, :, 4].abs().max()) == 0.0
    L = _lib.lib()
    with torch.no_grad():
        L.f3dg_debug_launch_count(1)
        s_ng = losses.warping_sums(render, w["warped"], w["mask"])
        assert int(L.f3dg_debug_launch_count(1)) == 2
    assert s_ng.grad_fn is None and torch.equal(s_ng, sums)
    L.f3dg_debug_launch_count(1)
    losses.warping_loss(render, w["warped"], w["mask"]).backward()
    assert int(L.f3dg_debug_launch_count(1)) == 3
