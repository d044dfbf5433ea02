"""GPU tests of the fused image loss: f3dg_ssim_forward / f3dg_ssim_backward through ctypes and through f3dgaus_amd.losses.

Truth is tests/ssim_truth.py in float64 (pinned to the reference's float64 results by tests/test_ssim_truth.py). Tolerance rule
(``ssim_truth.bound``): a quantity is held to THE REFERENCE'S OWN float32 ERROR against the same truth on the same case, margin 1 x, with a
floor of 4 float32 ulps of the quantity's scale -- max abs error for the map, abs error for the mean (floor 4 ulps of 1 = 4.8e-7), max abs
error over max|g| for a gradient, max abs error over the planes for the per-plane means. The reference's float32 results, or for the
seeded random dL/dm its two recorded error figures, are in the fixtures (tests/golden/ssim/*.npz). Only for the end-to-end test, whose
images are rendered on the device, the reference's float32 evaluation is ``ssim_truth.truth(dtype=torch.float32)``: its restatement with
the same 121 float32 window entries (within 0.6-1.6 x of the reference's own error on the fixture cases). The formula
is ill-conditioned where images are smooth (sigma^2 = E[x^2] - mu^2 cancels against C2 = 9e-4): the reference's float32 map is ~8e-4 from
its float64 self on the smooth 64 x 64 case and ~6e-6 on the random one, which is why the bound is read per case and is no constant.
A separable float32 evaluation adds 22 terms where the reference adds 121; on the host the map came out at 0.29-0.57 x the reference's error.
Every figure is printed before it is asserted (``pytest -s``)."""
import ctypes as C

import numpy as np
import pytest
import torch

import f3dgaus_amd as f3d
from f3dgaus_amd import _lib, losses
import ssim_truth as T

pytestmark = pytest.mark.gpu
_CACHE = {}
FLOOR = 4 * T.ULP


def _case(name):
    """Fixture arrays and the float64 truth of one case (with the fixture's random cotangent): computed once, shared, never modified."""
    if name not in _CACHE:
        z = T.load(name)
        a, b = z["img1"], z["img2"]
        dl = z["dL_dmap"]
        _CACHE[name] = dict(z=z, a=a, b=b, dl=dl, t64=T.truth(a, b, dL_dmap=dl))
    return _CACHE[name]


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _raw_forward(a, b, want_map=True, want_planes=True, want_sums=True):
    """f3dg_ssim_forward on [n, H, W] device tensors; every output starts as NaN, so an element the kernel skips shows."""
    n, H, W = a.shape
    L = _lib.lib()
    nan = lambda *s: torch.full(s, float("nan"), device=a.device)
    m = nan(n, H, W) if want_map else None
    planes = [nan(n, H, W) for _ in range(3)] if want_planes else [None] * 3
    nbytes = L.f3dg_ssim_partials_bytes(n, W, H)
    partials = nan(nbytes // 4) if want_sums else None
    sums = nan(n, 3) if want_sums else None
    rc = L.f3dg_ssim_forward(_stream(), n, W, H, _lib.ptr(a), _lib.ptr(b), _lib.ptr(m), *[_lib.ptr(p) for p in planes], _lib.ptr(partials),
                             nbytes if want_sums else 0, _lib.ptr(sums))
    assert rc == _lib.OK, rc
    torch.cuda.synchronize()
    return m, planes, sums


def _raw_backward(a, b, planes, dL_dmap=None, weights=None):
    n, H, W = a.shape
    g = torch.full((n, H, W), float("nan"), device=a.device)
    rc = _lib.lib().f3dg_ssim_backward(_stream(), n, W, H, _lib.ptr(a), _lib.ptr(b), _lib.ptr(dL_dmap), _lib.ptr(weights),
                                       *[_lib.ptr(p) for p in planes], _lib.ptr(g))
    assert rc == _lib.OK, rc
    torch.cuda.synchronize()
    return g


def _planar(x, dev):
    return torch.from_numpy(np.ascontiguousarray(x)).to(dev).reshape(-1, x.shape[-2], x.shape[-1]).contiguous()


def _check(label, err, bnd):
    print(f"{label}: error {err:.3e}  bound {bnd:.3e}  ratio {err / bnd:.2f}")
    assert err <= bnd, (label, err, bnd)


@pytest.mark.parametrize("name", T.cases())
def test_fixture_case_through_the_c_abi(gpu_device, name):
    c = _case(name)
    z, t64 = c["z"], c["t64"]
    shape = c["a"].shape
    npl, hw = shape[0] * shape[1], shape[2] * shape[3]
    a, b = _planar(c["a"], gpu_device), _planar(c["b"], gpu_device)
    m, planes, sums = _raw_forward(a, b)
    assert bool(torch.isfinite(m).all()) and all(bool(torch.isfinite(p).all()) for p in planes) and bool(torch.isfinite(sums).all())
    # the map
    _check(name + " map", T.max_err(m.reshape(shape), t64["map"]), T.bound(z["map32"], z["map64"], 1.0))
    # per-plane sums: the SSIM sums as plane means against the reference's own per-plane means (every plane evaluated alone by the
    # reference, float32 against float64; max abs error over the planes, floor 4 ulps of 1); the L1 and L2 sums within n 2^-24 relative
    # of float64 (n pixels per plane)
    s = sums.double().cpu().numpy()
    assert T.max_err(t64["sums"][:, 0] / hw, z["plane_mean64"]) <= 1e-10
    _check(name + " per-plane ssim means", T.max_err(s[:, 0] / hw, z["plane_mean64"]), T.bound(z["plane_mean32"], z["plane_mean64"], 1.0))
    for q, what in ((1, "L1"), (2, "L2")):
        rel = float(np.abs(s[:, q] - t64["sums"][:, q]).max() / np.abs(t64["sums"][:, q]).max())
        _check(f"{name} {what} sums (relative)", rel, hw * 2.0 ** -24)
    # the mean
    mean = float(s[:, 0].sum() / (npl * hw))
    _check(name + " mean", abs(mean - t64["mean"]), max(abs(float(z["mean32"]) - float(z["mean64"])), FLOOR))
    # gradient of the mean: per-plane weights (1 / n, 0, 0), no gradient plane
    w = torch.zeros(npl, 3, device=gpu_device)
    w[:, 0] = 1.0 / (npl * hw)
    g = _raw_backward(a, b, planes, weights=w)
    scale = float(np.abs(z["grad64"]).max())
    _check(name + " grad(mean) / max|g|", T.max_err(g.reshape(shape), t64["grad_mean"]) / scale, T.bound(z["grad32"], z["grad64"], scale) / scale)
    # the same through a full dL/dm plane set holding 1 / n
    g_full = _raw_backward(a, b, planes, dL_dmap=torch.full_like(a, 1.0 / (npl * hw)))
    assert torch.equal(g_full, g)
    # a seeded random full dL/dm
    g = _raw_backward(a, b, planes, dL_dmap=_planar(c["dl"], gpu_device))
    scale = float(z["grad_dl_max64"])
    assert abs(float(np.abs(t64["grad"]).max()) - scale) <= 1e-10
    _check(name + " grad(random dL/dm) / max|g|", T.max_err(g.reshape(shape), t64["grad"]) / scale, max(float(z["grad_dl_err32"]) / scale, FLOOR))
    # outputs are optional one by one, and what is written does not depend on what else is
    m2, _, _ = _raw_forward(a, b, want_planes=False, want_sums=False)
    _, planes2, sums2 = _raw_forward(a, b, want_map=False)
    assert torch.equal(m2, m) and torch.equal(sums2, sums) and all(torch.equal(p, q) for p, q in zip(planes, planes2))


@pytest.mark.parametrize("name", T.cases())
def test_fixture_case_through_losses(gpu_device, name):
    c = _case(name)
    z, t64 = c["z"], c["t64"]
    a = torch.from_numpy(c["a"]).to(gpu_device).requires_grad_()
    b = torch.from_numpy(c["b"]).to(gpu_device)
    # ssim: the mean and its gradient
    v = losses.ssim(a, b)
    assert v.shape == () and v.grad_fn is not None
    _check(name + " ssim", abs(float(v) - t64["mean"]), max(abs(float(z["mean32"]) - float(z["mean64"])), FLOOR))
    g, = torch.autograd.grad(v, a)
    scale = float(np.abs(z["grad64"]).max())
    _check(name + " d ssim / max|g|", T.max_err(g, t64["grad_mean"]) / scale, T.bound(z["grad32"], z["grad64"], scale) / scale)
    # ssim_map with the random upstream gradient
    m = losses.ssim_map(a, b)
    assert m.shape == a.shape
    _check(name + " ssim_map", T.max_err(m, t64["map"]), T.bound(z["map32"], z["map64"], 1.0))
    g, = torch.autograd.grad(m, a, torch.from_numpy(c["dl"]).to(gpu_device))
    scale = float(z["grad_dl_max64"])
    _check(name + " d ssim_map / max|g|", T.max_err(g, t64["grad"]) / scale, max(float(z["grad_dl_err32"]) / scale, FLOOR))
    # the reference's other reductions and metrics: shapes from the fixture, values within the reference's float32 distance
    # from float64 (floor: 4 ulps of the value)
    with torch.no_grad():
        per = losses.ssim(a, b, size_average=False)
        assert per.shape == z["ssim_n32"].shape
        tru = t64["map"].reshape(a.shape[0], -1).mean(1)
        _check(name + " ssim per image", T.max_err(per, tru), T.bound(z["ssim_n32"], tru, 1.0))
        d = c["a"].astype(np.float64) - c["b"].astype(np.float64)
        for fn, key, tru in ((losses.l1_loss, "l1_32", np.abs(d).mean()), (losses.l2_loss, "l2_32", (d * d).mean())):
            got = fn(a, b)
            assert got.shape == z[key].shape
            _check(f"{name} {key}", abs(float(got) - tru), T.bound(z[key], tru, tru))
        ps = losses.psnr(a, b)
        assert ps.shape == z["psnr32"].shape
        tru = 20 * np.log10(1.0 / np.sqrt((d * d).reshape(a.shape[0], -1).mean(1, keepdims=True)))
        _check(name + " psnr", T.max_err(ps, tru), T.bound(z["psnr32"], tru, float(np.abs(tru).max())))
        mt = losses.image_metrics(a, b)
        assert torch.equal(mt["ssim"], per) and torch.equal(mt["psnr"], ps) and mt["l1"].shape == per.shape


def test_identical_and_zero_images(gpu_device):
    """ssim(a, a): the map within 4 ulps of 1 and the mean's gradient within the same bound of 0 (numerator and denominator are the
    same float32 numbers; the gradient's two halves cancel up to roundings of terms of size <= 2 a / (n (2 sigma^2 + C2)) with
    sigma^2 ~ 1 / 12 for uniform noise: far below the bound for n = 3 x 37 x 21). All-zero images: exactly 1 = C1 C2 / (C1 C2)."""
    a = torch.from_numpy(T.load("random_1x3x37x21")["img1"]).to(gpu_device).requires_grad_()
    m = losses.ssim_map(a, a.detach())
    err = float((m - 1).abs().max())
    print(f"ssim_map(a, a): max|m - 1| {err:.3e}")
    assert err <= FLOOR
    g, = torch.autograd.grad(losses.ssim(a, a.detach()), a)
    print(f"d ssim(a, a): max|g| {float(g.abs().max()):.3e}")
    assert float(g.abs().max()) <= FLOOR
    zero = torch.zeros(2, 3, 19, 45, device=gpu_device)
    assert bool((losses.ssim_map(zero, zero) == 1.0).all()) and float(losses.ssim(zero, zero)) == 1.0
    assert float(losses.l1_loss(zero, zero)) == 0.0 and float(losses.l2_loss(zero, zero)) == 0.0


def test_sign_of_zero_contributes_no_gradient(gpu_device):
    """L1 weights alone: the gradient is w sign(a - b), exactly, and exactly 0 where a == b."""
    gen = torch.Generator().manual_seed(3)
    a = torch.rand(2, 3, 20, 37, generator=gen)
    b = torch.rand(2, 3, 20, 37, generator=gen)
    same = torch.rand(2, 3, 20, 37, generator=gen) < 0.3
    b = torch.where(same, a, b)
    a_d = a.to(gpu_device).requires_grad_()
    g, = torch.autograd.grad(losses.l1_loss(a_d, b.to(gpu_device)), a_d)
    w = np.float32(1.0) / np.float32(a.numel())
    assert torch.equal(g.cpu(), torch.sign(a - b) * float(w))
    assert bool((g.cpu()[same] == 0).all()) and int(same.sum()) > 0
    g, = torch.autograd.grad(losses.l2_loss(a_d, b.to(gpu_device)), a_d)
    tru = 2 * (a.double() - b.double()) / a.numel()
    assert float((g.cpu().double() - tru).abs().max()) <= FLOOR * float(tru.abs().max())


def test_padding(gpu_device):
    """a = 1, b = 0.5 on 13 rows x 12 columns (fixture padding_1x1x13x12): only the 3 x 2 block in the middle sees a full window; the
    border is attenuated by the zero padding and must match the truth like any fixture case."""
    z = T.load(T.case_name(T.PADDING_SHAPE, "padding"))
    assert bool((z["img1"] == 1).all()) and bool((z["img2"] == 0.5).all())
    t64 = T.truth(z["img1"], z["img2"])
    assert T.max_err(t64["map"], z["map64"]) <= 1e-10
    a = torch.from_numpy(z["img1"]).to(gpu_device).requires_grad_()
    m = losses.ssim_map(a, torch.from_numpy(z["img2"]).to(gpu_device))
    _check("padding map", T.max_err(m, z["map64"]), T.bound(z["map32"], z["map64"], 1.0))
    g, = torch.autograd.grad(m, a, torch.from_numpy(z["dL_dmap"]).to(gpu_device))
    scale = float(z["grad_dl_max64"])
    _check("padding grad / max|g|", T.max_err(g, T.truth(z["img1"], z["img2"], dL_dmap=z["dL_dmap"])["grad"]) / scale,
           max(float(z["grad_dl_err32"]) / scale, FLOOR))
    m = m.detach().cpu().numpy()
    inner = m[0, 0, 5:8, 5:7]
    assert inner.shape == (3, 2) and bool((inner == inner[0, 0]).all())
    border = np.ones((13, 12), bool)
    border[5:8, 5:7] = False
    assert bool((m[0, 0][border] != inner[0, 0]).all())
    assert abs(float(z["map64"][0, 0, 0, 0]) - float(z["map64"][0, 0, 6, 6])) > 1e-3       # the truth does differ there


def test_planes_are_isolated_and_a_nan_stays_local(gpu_device):
    gen = torch.Generator().manual_seed(9)
    a = torch.rand(3, 33, 33, generator=gen).to(gpu_device)
    b = torch.rand(3, 33, 33, generator=gen).to(gpu_device)
    dl = torch.randn(3, 33, 33, generator=gen).to(gpu_device)
    w = torch.randn(3, 3, generator=gen).to(gpu_device)
    bad = a.clone()
    bad[0, 17, 9] = float("nan")
    res = []
    for x in (a, bad):
        m, planes, sums = _raw_forward(x, b)
        res.append((m, sums, _raw_backward(x, b, planes, dL_dmap=dl, weights=w), _raw_backward(x, b, planes, weights=w)))
    for clean, dirty in zip(res[0], res[1]):
        assert torch.equal(clean[1:], dirty[1:])           # planes 1 and 2: maps, sums and both gradients, to the bit
    nonfinite = ~torch.isfinite(res[1][0][0])
    expect = torch.zeros(33, 33, dtype=torch.bool, device=gpu_device)
    expect[12:23, 4:15] = True
    assert torch.equal(nonfinite, expect)
    assert bool(torch.isfinite(res[0][0]).all()) and not bool(torch.isfinite(res[1][1][0]).any())


@pytest.mark.parametrize("n_planes", (1, 7))
def test_deterministic_and_composed(gpu_device, n_planes):
    """Two calls give the same bits. photometric_loss equals (1 - lambda) l1_loss + lambda (1 - ssim) from the separate calls within
    2 ulps, and so does its gradient (relative to its maximum)."""
    gen = torch.Generator().manual_seed(20 + n_planes)
    a = torch.rand(n_planes, 50, 70, generator=gen).to(gpu_device)           # 3 x 4 tiles per plane, ragged in both axes
    b = (a.cpu() + 0.1 * torch.randn(n_planes, 50, 70, generator=gen)).clamp(0, 1).to(gpu_device)
    w = torch.randn(n_planes, 3, generator=gen).to(gpu_device)
    runs = []
    for _ in range(2):
        m, planes, sums = _raw_forward(a, b)
        runs.append((m, sums, _raw_backward(a, b, planes, weights=w)))
    assert all(torch.equal(x, y) for x, y in zip(*runs))
    x = a.reshape(1, n_planes, 50, 70).clone().requires_grad_()
    y = b.reshape(1, n_planes, 50, 70)
    lam = 0.2
    fused = losses.photometric_loss(x, y, lambda_dssim=lam)
    g_fused, = torch.autograd.grad(fused, x)
    composed = (1 - lam) * losses.l1_loss(x, y) + lam * (1 - losses.ssim(x, y))
    g_comp, = torch.autograd.grad(composed, x)
    assert abs(float(fused) - float(composed)) <= 2 * T.ULP * abs(float(composed))
    assert float((g_fused - g_comp).abs().max()) <= 2 * T.ULP * float(g_comp.abs().max())
    t = T.truth(a.cpu().numpy(), b.cpu().numpy())
    tru = (1 - lam) * t["sums"][:, 1].sum() / a.numel() + lam * (1 - t["mean"])
    assert abs(float(fused) - tru) <= FLOOR


def test_reductions_and_shapes(gpu_device):
    gen = torch.Generator().manual_seed(31)
    r = torch.rand(2, 3, 3, 18, 34, generator=gen).to(gpu_device)            # [B, V, 3, H, W], as render_views returns it
    t = torch.rand(2, 3, 3, 18, 34, generator=gen).to(gpu_device)
    none = losses.photometric_loss(r, t, reduction="none")
    assert none.shape == (2, 3)
    per = losses.ssim(r, t, size_average=False)
    assert per.shape == (2, 3) and losses.ssim(r[0], t[0], size_average=False).shape == (3,) and losses.ssim(r[0, 0], t[0, 0], size_average=False).shape == ()
    assert losses.psnr(r, t).shape == (2, 1) and losses.psnr(r[0], t[0]).shape == (3, 1)
    # every frame's loss is that of the frame alone (the per-plane sums are the same bits; torch adds the three of a frame in its
    # own order in the two reductions: 2 ulps); the mean is their mean
    for i in range(2):
        for j in range(3):
            assert abs(float(losses.photometric_loss(r[i, j], t[i, j])) - float(none[i, j])) <= 2 * T.ULP * float(none[i, j])
    assert abs(float(losses.photometric_loss(r, t)) - float(none.double().mean())) <= FLOOR


def test_autograd_plumbing(gpu_device):
    gen = torch.Generator().manual_seed(41)
    base = torch.rand(2, 40, 24, 4, generator=gen).to(gpu_device)
    tgt = torch.rand(2, 40, 24, 4, generator=gen).to(gpu_device)
    # non-contiguous [..., C, H, W] views (channels-last storage, and a channel slice) against their contiguous copies, to the bit
    for view in (lambda x: x.permute(0, 3, 1, 2), lambda x: x.permute(0, 3, 1, 2)[:, 1:4]):
        a_nc = view(base.clone().requires_grad_())
        b_nc = view(tgt)
        assert not a_nc.is_contiguous()
        a_c = a_nc.detach().contiguous().requires_grad_()
        for fn in (losses.ssim, losses.photometric_loss, lambda p, q: (losses.ssim_map(p, q) * b_nc).sum()):
            leaf = a_nc.detach().requires_grad_()           # (a strided leaf)
            v_nc, v_c = fn(leaf, b_nc), fn(a_c, b_nc.contiguous())
            assert torch.equal(v_nc, v_c)
            g_nc, = torch.autograd.grad(v_nc, leaf)
            g_c, = torch.autograd.grad(v_c, a_c)
            assert torch.equal(g_nc, g_c) and float(g_c.abs().max()) > 0
    a = base.permute(0, 3, 1, 2).contiguous().requires_grad_()
    b = tgt.permute(0, 3, 1, 2).contiguous()
    with pytest.raises(NotImplementedError, match="img2"):
        losses.ssim(a, b.clone().requires_grad_())
    with pytest.raises(TypeError, match="float32"):
        losses.ssim(a.double(), b.double())
    with pytest.raises(ValueError, match="shape"):
        losses.photometric_loss(a, b[..., :-1])
    with pytest.raises(RuntimeError, match="HIP device"):
        losses.ssim(a, b.cpu())
    with torch.no_grad():
        v = losses.photometric_loss(a, b)
    assert v.grad_fn is None and torch.equal(v, losses.photometric_loss(a, b).detach())
    # through a graph in front of the loss, and on a side stream
    x = a.detach().clone().requires_grad_()
    losses.photometric_loss(torch.sigmoid(x), b).backward()
    assert x.grad is not None and bool(torch.isfinite(x.grad).all()) and float(x.grad.abs().max()) > 0
    ref = losses.photometric_loss(a, b)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        on_side = losses.photometric_loss(a, b)
    side.synchronize()
    assert torch.equal(on_side, ref)


def test_render_views_into_the_loss(gpu_device):
    """predictor-shaped Gaussians -> render_views(differentiable=True) -> photometric_loss -> backward: 1 set x 2 views at 64 x 64."""
    from f3dgaus_amd import synthetic
    dev = gpu_device
    cam = synthetic.orbit_cameras(8, 64, device=dev)
    g = synthetic.make_gaussians(400, s0=0.05, seed=5, device=dev)
    leaves = {k: v.unsqueeze(0).clone().requires_grad_() for k, v in g.items()}                # one set: [1, P, ...]
    cams = tuple(cam[k][[1, 5]].contiguous() for k in ("viewmatrix", "projmatrix", "campos"))
    cfg = cam["cfg"]
    out = f3d.render_views(leaves, None, *cams, torch.tensor([0.2, 0.5, 0.3], device=dev), cfg, differentiable=True)
    render = out["render"]
    render.retain_grad()
    target = torch.rand(render.shape, generator=torch.Generator().manual_seed(6)).to(dev)
    loss = losses.photometric_loss(render, target)
    loss.backward()
    for k, t in leaves.items():
        assert t.grad is not None and bool(torch.isfinite(t.grad).all()) and float(t.grad.abs().max()) > 0, k
    r, tg = render.detach().cpu().numpy(), target.cpu().numpy()
    n = r.size
    w = np.zeros((r.size // (r.shape[-1] * r.shape[-2]), 3))
    w[:, 0], w[:, 1] = -0.2 / n, 0.8 / n
    t64, t32 = T.truth(r, tg, plane_weights=w), T.truth(r, tg, plane_weights=w, dtype=torch.float32)
    scale = float(np.abs(t64["grad"]).max())
    _check("d photometric_loss / d render / max|g|", T.max_err(render.grad, t64["grad"]) / scale, T.bound(t32["grad"], t64["grad"], scale) / scale)
