"""Training through the fused backbone on the device: the GroupNorm (+ SiLU) and residual-join backward kernels
(csrc/f3dg_groupnorm_bwd.hip) behind ``gaussian_predictor.GroupNorm`` / ``residual_join`` / ``UNetBlock`` with the ``fused_autograd`` switch,
against float64 (tests/backbone_backward_truth.py).

Bound, for every gradient g of a case: max|g - g64| <= T.bound32(E32, g64) = max(2 E32, 2e-6 max(1, max|g64|)), E32 the error of torch's
float32 autograd of the same expression ON THE DEVICE on the same case -- the suite's rule for these kernels' forward, unchanged. Every case
prints error, bound and ratio before it asserts."""
import copy
import types

import pytest
import torch

import backbone_backward_truth as G
import backbone_truth as T
from f3dgaus_amd import gaussian_predictor as gp

pytestmark = pytest.mark.gpu

SWEEP = [("nchw", s) for s in T.NCHW_SHAPES] + [("nhwc", s) for s in T.NHWC_SHAPES + (T.NHWC_LONG_RUN,)]
SWEEP_IDS = ["%s-%s" % (l, "x".join(map(str, s))) for l, s in SWEEP]
NORMAL = [c for c in T.contents() if c[2] == "normal"]
OTHER = [c for c in T.contents() if c[2] != "normal"]


def _sid(s):
    return "x".join(map(str, s))


def _layout(x, layout):
    return x.contiguous(memory_format=torch.channels_last) if layout == "nhwc" else x.contiguous()


def _module(c, dev, fused=True):
    gn = gp.GroupNorm(c["weight"].numel(), eps=T.EPS).to(dev)
    with torch.no_grad():
        gn.weight.copy_(c["weight"]); gn.bias.copy_(c["bias"])
    assert gn.num_groups == c["groups"]
    return gp.set_fused_autograd(gn, fused)


def _fused_grads(gn, x, pb, silu, gy, layout):
    """One forward + backward through the module; returns ({name: gradient}, y)."""
    xl = _layout(x, layout).detach().requires_grad_()
    p = None if pb is None else pb.detach().clone().requires_grad_()
    gn.weight.grad = gn.bias.grad = None
    y = gn(xl, silu=silu, pre_bias=p)
    assert y.shape == x.shape and y.dtype == torch.float32 and gp._is_nhwc(y) == (layout == "nhwc")      # (the layout tells which kernel ran)
    y.backward(_layout(gy, layout))
    out = {"dx": xl.grad, "dweight": gn.weight.grad, "dbias": gn.bias.grad}
    if p is not None:
        out["dpre_bias"] = p.grad
    return out, y


def _sweep(dev, layout, shape, content, assert_bound):
    label, ratio, kind = content
    c = T.make_case(shape, ratio, 11, kind)
    gn = _module(c, dev)
    x, pb, gy = c["x"].to(dev), c["pre_bias"].to(dev), G.cotangent(shape, 12).to(dev)
    for silu in (False, True):
        for p in (None, pb):
            args = (x, p, gn.weight, gn.bias, gn.num_groups, gn.eps, silu, gy)
            ref, yard = G.grad_truth(*args), G.grad_torch32(*args)
            got, _ = _fused_grads(gn, x, p, silu, gy, layout)
            assert set(got) == set(ref)
            for name, err, bnd, r in G.compare(got, ref, yard):
                print(f"{layout} {_sid(shape)} {label} silu={int(silu)} pb={int(p is not None)} {name}: error {err:.3e}  bound {bnd:.3e}  ratio {r:.2f}")
                assert bool(torch.isfinite(got[name]).all()), (label, name)
                if assert_bound:
                    assert err <= bnd, (layout, shape, label, silu, p is not None, name, err, bnd)


# ------------------------------------------------------------------------------------------------ gradient sweep
@pytest.mark.parametrize("content", NORMAL, ids=lambda c: c[0])
@pytest.mark.parametrize("layout,shape", SWEEP, ids=SWEEP_IDS)
def test_group_norm_backward_sweep(gpu_device, layout, shape, content):
    """|mean| / std from 0.5 to 100; SiLU off / on, with / without pre_bias; dx, dweight, dbias, dpre_bias within the bound."""
    _sweep(gpu_device, layout, shape, content, True)


@pytest.mark.parametrize("content", OTHER, ids=lambda c: c[0])
@pytest.mark.parametrize("layout,shape", SWEEP, ids=SWEEP_IDS)
def test_group_norm_backward_constant_slabs_are_finite(gpu_device, layout, shape, content):
    """Near-constant (8 +- 1e-3) and constant slabs: every gradient finite; the ratio is printed, not asserted -- the rounding of
    x + pre_bias at 8 +- 1e-3 dominates there and leaves the rule no margin for any float32 evaluation."""
    _sweep(gpu_device, layout, shape, content, False)


# ------------------------------------------------------------------------------------------------ dispatch
def _no_torch(*a, **k):
    raise AssertionError("the torch operators were reached")


@pytest.mark.parametrize("layout", ("nchw", "nhwc"))
def test_switch_on_runs_the_kernels_under_autograd(gpu_device, layout, monkeypatch):
    c = T.make_case((2, 64, 8, 8), 10.0, 41)
    gn = _module(c, gpu_device)
    x, pb, gy = c["x"].to(gpu_device), c["pre_bias"].to(gpu_device), G.cotangent((2, 64, 8, 8), 42).to(gpu_device)
    monkeypatch.setattr(gp, "F", types.SimpleNamespace(group_norm=_no_torch, silu=_no_torch))
    assert torch.is_grad_enabled()
    for silu in (False, True):
        got, y = _fused_grads(gn, x, pb, silu, gy, layout)
        assert y.grad_fn is not None and all(bool(torch.isfinite(g).all()) for g in got.values())
    # and the join: out of place under autograd, no in-place error, gradients for both operands and both biases
    a, b = _layout(x, layout).detach().requires_grad_(), _layout(gy, layout).detach().requires_grad_()
    ba, bb = pb.detach().clone().requires_grad_(), (2 * pb).detach().requires_grad_()
    j = gp.residual_join(a * 1.0, ba, b, bb, 0.5, fused_autograd=True)
    assert type(j.grad_fn).__name__.startswith("_ResidualJoin")
    j.backward(_layout(gy, layout))
    assert all(t.grad is not None and bool(torch.isfinite(t.grad).all()) for t in (a, b, ba, bb))


def test_switch_off_still_reaches_torch_group_norm(gpu_device, monkeypatch):
    """The default is unchanged: with grad enabled a new module takes F.group_norm (and F.silu)."""
    c = T.make_case((2, 64, 8, 8), 10.0, 43)
    gn = _module(c, gpu_device, fused=False)
    assert gp.GroupNorm(64).fused_autograd is False and gp.UNetBlock(64, 64).fused_autograd is False
    calls = []
    real = gp.F

    def counted(*a, **k):
        calls.append(1)
        return real.group_norm(*a, **k)
    monkeypatch.setattr(gp, "F", types.SimpleNamespace(group_norm=counted, silu=real.silu))
    x = c["x"].to(gpu_device).requires_grad_()
    y = gn(x, silu=True, pre_bias=c["pre_bias"].to(gpu_device))
    y.sum().backward()
    assert len(calls) == 1 and x.grad is not None
    with torch.no_grad():                        # (inference: the kernel, as before)
        gn(x, silu=True)
    assert len(calls) == 1


# ------------------------------------------------------------------------------------------------ saved state
@pytest.mark.parametrize("shape", ((2, 64, 8, 8), (1, 128, 64, 64)), ids=_sid)
def test_fused_node_saves_x_and_little_else(gpu_device, shape):
    c = T.make_case(shape, 10.0, 44)
    x = c["x"].to(gpu_device).requires_grad_()
    pb = c["pre_bias"].to(gpu_device).requires_grad_()

    def saved_bytes(gn):
        seen = {}

        def pack(t):
            seen[(t.data_ptr(), t.numel())] = t.numel() * t.element_size()
            return t
        with torch.autograd.graph.saved_tensors_hooks(pack, lambda t: t):
            y = gn(x, silu=True, pre_bias=pb)
        assert y.requires_grad
        return sum(seen.values())

    nbytes = x.numel() * 4
    fused, plain = saved_bytes(_module(c, gpu_device)), saved_bytes(_module(c, gpu_device, fused=False))
    print(f"{_sid(shape)}: saved for backward, in units of x: fused {fused / nbytes:.3f}, torch {plain / nbytes:.3f}")
    assert fused < 1.25 * nbytes
    assert plain >= 2 * nbytes


# ------------------------------------------------------------------------------------------------ determinism, isolation
@pytest.mark.parametrize("layout,shape", (("nhwc", (1, 128, 64, 64)), ("nchw", (1, 128, 48, 48))), ids=("nhwc", "nchw"))
def test_backward_is_bit_identical_run_to_run(gpu_device, layout, shape):
    c = T.make_case(shape, 10.0, 45)
    gn = _module(c, gpu_device)
    x, pb, gy = c["x"].to(gpu_device), c["pre_bias"].to(gpu_device), G.cotangent(shape, 46).to(gpu_device)
    a, _ = _fused_grads(gn, x, pb, True, gy, layout)
    a = {k: v.clone() for k, v in a.items()}
    b, _ = _fused_grads(gn, x, pb, True, gy, layout)
    for k in a:
        assert torch.equal(a[k], b[k]), k


@pytest.mark.parametrize("layout", ("nchw", "nhwc"))
def test_non_finite_cotangent_stays_in_its_slab(gpu_device, layout):
    shape, n, g = (2, 128, 20, 13), 1, 5
    c = T.make_case(shape, 10.0, 47)
    gn = _module(c, gpu_device)
    cg = shape[1] // c["groups"]
    x, pb, gy = c["x"].to(gpu_device), c["pre_bias"].to(gpu_device), G.cotangent(shape, 48).to(gpu_device)
    clean, _ = _fused_grads(gn, x, pb, True, gy, layout)
    clean = {k: v.clone() for k, v in clean.items()}
    bad = gy.clone()
    bad[n, g * cg + 1, 7, 4] = float("nan")
    got, _ = _fused_grads(gn, x, pb, True, bad, layout)
    slab = torch.zeros(shape, dtype=torch.bool, device=gpu_device)
    slab[n, g * cg:(g + 1) * cg] = True
    assert not bool(torch.isfinite(got["dx"][slab]).any())
    assert torch.equal(got["dx"][~slab], clean["dx"][~slab])
    chan = torch.zeros(shape[1], dtype=torch.bool, device=gpu_device)
    chan[g * cg:(g + 1) * cg] = True
    for k in ("dweight", "dbias", "dpre_bias"):
        assert torch.equal(got[k][~chan], clean[k][~chan]), k
        assert bool(torch.isfinite(got[k][~chan]).all()), k


# ------------------------------------------------------------------------------------------------ join backward
def _join_grads(a, ba, b, bb, scale, gy, layout):
    leaves = [_layout(a, layout).detach().requires_grad_(), None if ba is None else ba.detach().clone().requires_grad_(),
              _layout(b, layout).detach().requires_grad_(), None if bb is None else bb.detach().clone().requires_grad_()]
    y = gp.residual_join(leaves[0], leaves[1], leaves[2], leaves[3], scale, fused_autograd=True)
    assert type(y.grad_fn).__name__.startswith("_ResidualJoin") and gp._is_nhwc(y) == (layout == "nhwc")
    y.backward(_layout(gy, layout))
    return [None if t is None else t.grad for t in leaves]


JOIN_SMALL = (("nchw", (2, 6, 3, 3)),         # planes of 9 values: the scalar path
              ("nchw", (2, 8, 4, 6)),         # packets
              ("nhwc", (3, 24, 5, 7)))        # 6 packets per pixel: idle threads


@pytest.mark.parametrize("layout,shape", JOIN_SMALL, ids=["%s-%s" % (l, _sid(s)) for l, s in JOIN_SMALL])
def test_residual_join_backward_is_exact_on_integers(gpu_device, layout, shape):
    """Small even integers and scale 0.5, as the forward's integer cases: grad_y * 0.5 and its per-channel sums are exact in float32."""
    N, Cc, H, W = shape
    i = torch.arange(N * H * W * Cc, device=gpu_device, dtype=torch.int64)
    f = lambda m: ((((i * m) % 9) - 4) * 2).reshape(N, H, W, Cc).permute(0, 3, 1, 2).float()
    a, b, gy = f(5), f(7), f(11)
    ch = torch.arange(Cc, device=gpu_device, dtype=torch.float32)
    want = gy * 0.5
    for ba, bb in ((8 * ch, -3 * ch - 1), (8 * ch, None), (None, None)):
        da, dba, db, dbb = _join_grads(a, ba, b, bb, 0.5, gy, layout)
        assert torch.equal(da, want) and torch.equal(db, want)
        for t in (dba, dbb):
            assert t is None or torch.equal(t, want.sum((0, 2, 3)))
        assert (dba is None) == (ba is None) and (dbb is None) == (bb is None)


@pytest.mark.parametrize("layout,shape", (("nchw", (2, 64, 16, 16)), ("nhwc", (2, 64, 16, 16)), ("nchw", (2, 8, 72, 72)), ("nhwc", (2, 8, 72, 72))),
                         ids=lambda v: v if isinstance(v, str) else _sid(v))
def test_residual_join_backward_random_data(gpu_device, layout, shape):
    """grad_y * scale to the bit (one float32 multiplication); its per-channel sum within bound32 of float64, E32 torch's float32 sum."""
    g = torch.Generator().manual_seed(9)
    a, b, gy = (torch.randn(shape, generator=g).to(gpu_device) for _ in range(3))
    ba, bb = torch.randn(shape[1], generator=g).to(gpu_device), torch.randn(shape[1], generator=g).to(gpu_device)
    scale = 0.7071067811865476
    da, dba, db, dbb = _join_grads(a, ba, b, bb, scale, gy, layout)
    want = gy * scale
    assert torch.equal(da, want) and torch.equal(db, want) and torch.equal(dba, dbb)
    ref = want.double().sum((0, 2, 3))
    e32 = float((want.sum((0, 2, 3)).double() - ref).abs().max())
    err, bnd = float((dba.double() - ref).abs().max()), T.bound32(e32, ref)
    print(f"join backward {layout} {_sid(shape)} dbias: error {err:.3e}  bound {bnd:.3e}  ratio {err / bnd:.2f}")
    assert err <= bnd


# ------------------------------------------------------------------------------------------------ a residual block
def _randomised(blk, seed):
    """Norm weights near 1, every bias and the second convolution's tiny filter of ordinary size: all gradients are exercised."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, p in blk.named_parameters():
            if name.endswith("bias"):
                p.copy_(0.1 * torch.randn(p.shape, generator=g))
            elif p.dim() == 1:
                p.copy_(1 + 0.1 * torch.randn(p.shape, generator=g))
            elif name.startswith(("conv1", "proj")):
                p.copy_(torch.randn(p.shape, generator=g) * (1.0 / (p.shape[1] * p.shape[2] * p.shape[3])) ** 0.5)
    return blk


def _block_grads(blk, x, gy):
    xl = x.detach().requires_grad_()
    blk.zero_grad(set_to_none=True)
    y = blk(xl)
    y.backward(gy.to(device=y.device, dtype=y.dtype))
    out = {"x": xl.grad}
    out.update({n: p.grad for n, p in blk.named_parameters()})
    assert all(v is not None for v in out.values()), [k for k, v in out.items() if v is None]
    return out


BLOCKS = (("64-128", dict(in_channels=64, out_channels=128), 8),
          ("128-128-attention", dict(in_channels=128, out_channels=128, attention=True), 8),
          ("64-64-down", dict(in_channels=64, out_channels=64, down=True), 16))


@pytest.mark.parametrize("name,kw,res", BLOCKS, ids=[b[0] for b in BLOCKS])
def test_unet_block_gradients(gpu_device, name, kw, res):
    """Two samples, dropout 0: every input and parameter gradient of the fused route within bound32 of E32, E32 the torch route's error on
    the device, truth the block's float64 copy on the host. Channels-last is printed beside it (no yardstick of its own: not asserted)."""
    torch.manual_seed(3)
    blk = _randomised(gp.UNetBlock(dropout=0.0, **kw), 5).eval()
    g = torch.Generator().manual_seed(6)
    x = torch.randn(2, kw["in_channels"], res, res, generator=g)
    gy = torch.randn(2, kw["out_channels"], res // (2 if kw.get("down") else 1), res // (2 if kw.get("down") else 1), generator=g)
    ref = _block_grads(copy.deepcopy(blk).double(), x.double(), gy)
    dev_blk = copy.deepcopy(blk).to(gpu_device)
    yard = _block_grads(dev_blk, x.to(gpu_device), gy)
    gp.set_fused_autograd(dev_blk, True)
    got = _block_grads(dev_blk, x.to(gpu_device), gy)
    got_cl = _block_grads(dev_blk, x.to(gpu_device).contiguous(memory_format=torch.channels_last), gy)
    for k, r in ref.items():
        e32 = float((yard[k].double().cpu() - r).abs().max())
        bnd = T.bound32(e32, r)
        err = float((got[k].double().cpu() - r).abs().max())
        err_cl = float((got_cl[k].double().cpu() - r).abs().max())
        print(f"block {name} {k}: error {err:.3e}  bound {bnd:.3e}  ratio {err / bnd:.2f}  (channels-last: error {err_cl:.3e}  ratio {err_cl / bnd:.2f})")
        assert bool(torch.isfinite(got_cl[k]).all()), k
    for k, r in ref.items():
        e32 = float((yard[k].double().cpu() - r).abs().max())
        assert float((got[k].double().cpu() - r).abs().max()) <= T.bound32(e32, r), (name, k)


def test_unet_block_training_mode_runs_the_fused_route(gpu_device):
    """training=True, dropout 0.1, a fixed seed: the fused route (dropout between norm1 and conv1) runs and every gradient is finite."""
    blk = gp.set_fused_autograd(_randomised(gp.UNetBlock(64, 128, dropout=0.1), 7).to(gpu_device), True).train()
    g = torch.Generator().manual_seed(8)
    x, gy = torch.randn(2, 64, 8, 8, generator=g).to(gpu_device), torch.randn(2, 128, 8, 8, generator=g).to(gpu_device)
    torch.manual_seed(11)
    xl = x.requires_grad_()
    y = blk(xl)
    assert type(y.grad_fn).__name__.startswith("_ResidualJoin")
    y.backward(gy)
    for n, p in list(blk.named_parameters()) + [("x", xl)]:
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), n


# ------------------------------------------------------------------------------------------------ the whole backbone
def test_whole_backbone_gradients_both_routes(gpu_device):
    """cameras.default_cfg(32), one image, the same weights in both routes and a seeded cotangent on net_out: every parameter gets a finite
    gradient either way, and the fused route's global L2 error against a host float64 run is at most T.MARGIN x the torch route's."""
    from f3dgaus_amd import cameras
    from helpers_weights import formula_state_dict
    nets = {}
    for route in ("torch", "fused"):
        cfg = cameras.default_cfg(32)
        cfg["model"]["backbone_autograd"] = route
        pred = gp.GaussianSplatPredictor_gtunet(cfg).eval()
        assert pred.backbone_autograd == route
        sd = pred.state_dict()
        keep = {k: v for k, v in sd.items() if k in ("ray_dirs", "sh_to_v_transform", "v_to_sh_transform") or k.endswith("resample_filter")}
        pred.load_state_dict(formula_state_dict({k: tuple(v.shape) for k, v in sd.items()}, keep=keep))
        nets[route] = pred.network_with_offset
    assert all(m.fused_autograd for m in nets["fused"].modules() if isinstance(m, (gp.GroupNorm, gp.UNetBlock)))
    assert not any(m.fused_autograd for m in nets["torch"].modules() if isinstance(m, (gp.GroupNorm, gp.UNetBlock)))
    g = torch.Generator().manual_seed(13)
    x = torch.rand(1, 4, 32, 32, generator=g)
    cot = torch.randn(1, 23, 32, 32, generator=g)

    def grads(net, xx):
        net.zero_grad(set_to_none=True)
        out = net(xx, N_views_xa=1)
        out.backward(cot.to(device=out.device, dtype=out.dtype))
        return {n: p.grad.double().cpu() for n, p in net.named_parameters()}

    ref = grads(copy.deepcopy(nets["torch"]).double(), x.double())
    got = {route: grads(nets[route].to(gpu_device), x.to(gpu_device)) for route in ("torch", "fused")}
    l2, worst = {}, {}
    for route in ("torch", "fused"):
        assert set(got[route]) == set(ref)
        assert all(bool(torch.isfinite(v).all()) for v in got[route].values()), route
        l2[route] = sum(float(((got[route][k] - ref[k]) ** 2).sum()) for k in ref) ** 0.5
        rel = {k: float((got[route][k] - ref[k]).norm() / max(float(ref[k].norm()), 1e-30)) for k in ref}
        k = max(rel, key=rel.get)
        worst[route] = (k, rel[k])
    norm = sum(float((ref[k] ** 2).sum()) for k in ref) ** 0.5
    print(f"whole backbone, {len(ref)} parameter tensors, |grad|_2 {norm:.3e}: global L2 error torch {l2['torch']:.3e}, fused {l2['fused']:.3e} "
          f"(ratio {l2['fused'] / l2['torch']:.2f}); worst tensor by relative L2 error: torch {worst['torch'][0]} {worst['torch'][1]:.2e}, "
          f"fused {worst['fused'][0]} {worst['fused'][1]:.2e}")
    assert l2["fused"] <= T.MARGIN * l2["torch"]
