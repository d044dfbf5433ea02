"""GPU tests of the splat head's backward (f3dg_splat_head_backward behind f3d.splat_head's autograd Function).

Truth is the float64 autograd of the torch restatement of the reference's lines (tests/splat_head_truth.py, pinned to the reference by
tests/test_splat_head_backward.py). Tolerance rule, per gradient channel group (offset, opacity, scaling, rotation, dc, rest, depth):
E_ref = max|g32 - g64| / max|g64| with g32 the same restatement's float32 autograd on the CPU (what the reference returns), and the
kernel passes when max|g_kernel - g64| <= 4 * E_ref * max|g64|."""
import ctypes as C

import numpy as np
import pytest
import torch

import f3dgaus_amd as f3d
from f3dgaus_amd import _lib, cameras
import splat_head_truth as T

pytestmark = pytest.mark.gpu
KEYS = T.KEYS
_CACHE = {}


def _fixture():
    """Inputs and cotangents of the fixtures (read once, never modified: the tests clone what they change)."""
    if "fx" not in _CACHE:
        _CACHE["fx"] = (T.load_inputs()[0], T.load_cotangents()[0])
    return _CACHE["fx"]


def _truth(tag, inputs, cots, clip):
    """(g32, g64) of the restatement on the CPU, computed once per configuration."""
    if tag not in _CACHE:
        _CACHE[tag] = (T.restatement_grads(inputs, cots, clip, torch.float32), T.restatement_grads(inputs, cots, clip, torch.float64))
    return _CACHE[tag]


def _kernel_grads(inputs, cots, clip, dev):
    net = inputs["net_out"].to(dev).requires_grad_()
    dep = inputs["depth"].to(dev).requires_grad_()
    out = f3d.splat_head(net, dep, inputs["ray_dirs"].to(dev), inputs["v2w"].to(dev), inputs["quat"].to(dev), squre_clip=clip)
    assert all(out[k].grad_fn is not None for k in KEYS), "the splat head's outputs carry no autograd graph"
    used = [k for k in KEYS if cots.get(k) is not None]
    gn, gd = torch.autograd.grad([out[k] for k in used], [net, dep], [cots[k].to(dev) for k in used])
    return gn, gd


@pytest.mark.parametrize("which", ("all",) + KEYS)
def test_fixture_gradients(gpu_device, which):
    """B = 2, 32 x 32, the fixture's cotangents on all seven outputs, then on one output at a time with the other six unused (None
    cotangents -> NULL pointers): cross-wired channels and the NULL path."""
    inputs, cots = _fixture()
    cots = cots if which == "all" else {which: cots[which]}
    g32, g64 = _truth("fixture_" + which, inputs, cots, 10000.0)
    got = _kernel_grads(inputs, cots, 10000.0, gpu_device)
    assert got[0].shape == (2, 23, 32, 32) and got[1].shape == (2, 1, 32, 32)
    T.check_groups(got, g32, g64, label="fixture/" + which)
    if which != "all":      # the groups this output does not feed are exactly zero
        for name, t in T.by_group(*got).items():
            if float(T.by_group(*g64)[name].abs().max()) == 0.0:
                assert float(t.abs().max()) == 0.0, name


def test_expanded_and_strided_cotangents(gpu_device):
    """.sum() hands the backward an expanded scalar, a transposed weight a strided tensor: both are made dense before the kernel."""
    inputs, _ = _fixture()
    w = torch.randn(3, 2, 1024, generator=torch.Generator().manual_seed(5))
    cots = {"opacity": torch.ones(2, 1024, 1), "xyz": w.permute(1, 2, 0)}
    assert not cots["xyz"].is_contiguous()
    net = inputs["net_out"].to(gpu_device).requires_grad_()
    dep = inputs["depth"].to(gpu_device).requires_grad_()
    out = f3d.splat_head(net, dep, inputs["ray_dirs"].to(gpu_device), inputs["v2w"].to(gpu_device), inputs["quat"].to(gpu_device))
    (out["opacity"].sum() + (out["xyz"] * w.to(gpu_device).permute(1, 2, 0)).sum()).backward()
    g32, g64 = _truth("expanded", inputs, {k: v.contiguous() for k, v in cots.items()}, 10000.0)
    T.check_groups((net.grad, dep.grad), g32, g64, label="expanded")


def test_clip(gpu_device):
    """squre_clip = 0.3: clamped x / y pass no gradient, everything else is unchanged. The clamped set must be the truth's: the inputs
    keep every |X|, |Y| at least 1e-5 away from the bound (asserted), so float32 and float64 clamp the same pixels."""
    inputs, cots = _fixture()
    with torch.no_grad():
        xy = T.splat_head_torch(inputs["net_out"].double(), inputs["depth"].double(), inputs["ray_dirs"], inputs["v2w"], inputs["quat"])["xyz"][..., :2]
    assert float((xy.abs() - 0.3).abs().min()) > 1e-5
    clamped = (xy.abs() > 0.3)
    assert 0 < int(clamped.sum()) < clamped.numel()
    g32, g64 = _truth("clip", inputs, cots, 0.3)
    got = _kernel_grads(inputs, cots, 0.3, gpu_device)
    T.check_groups(got, g32, g64, label="clip")
    plain = _kernel_grads(inputs, cots, 10000.0, gpu_device)
    assert torch.equal(got[0][:, 3:], plain[0][:, 3:])                        # the other five groups do not see the clamp
    free = ~(clamped[..., 0] | clamped[..., 1]).reshape(2, 1, 32, 32).to(gpu_device)
    assert torch.equal(torch.where(free, got[0][:, :3], plain[0][:, :3]), plain[0][:, :3])      # unclamped rows: bit-identical
    assert torch.equal(torch.where(free, got[1], plain[1]), plain[1])
    assert not torch.equal(got[0][:, :3], plain[0][:, :3])


def _raw_backward(B, H, W, t, clip, n_total, n_offset, gs, d_net, d_depth):
    rc = _lib.lib().f3dg_splat_head_backward(
        C.c_void_p(torch.cuda.current_stream().cuda_stream), B, H, W, _lib.ptr(t["net_out"]), _lib.ptr(t["depth"]), _lib.ptr(t["ray_dirs"]),
        _lib.ptr(t["v2w"]), _lib.ptr(t["quat"]), float(clip), n_total, n_offset, *[_lib.ptr(g) for g in gs], _lib.ptr(d_net),
        _lib.ptr(d_depth))
    assert rc == _lib.OK, rc
    torch.cuda.synchronize()


@pytest.mark.parametrize("B,H,W", [(3, 5, 7), (1, 17, 17)])
def test_shapes_and_offset_window_through_the_c_abi(gpu_device, B, H, W):
    """HW = 35 (one partial workgroup) and 289 (a full workgroup plus a tail); n_total = 3 HW, n_offset = HW with NaN in every gradient row
    outside the window and in the outputs before the call: finite, bit-identical to the n_offset = 0 call, every element written;
    d_depth = NULL leaves d_net_out bit-identical."""
    HW = H * W
    gen = torch.Generator().manual_seed(100 + HW)
    ob = cameras.OrbitRig(cameras.default_cfg()).orbit(8)
    idx = [1, 4, 6][:B]
    net = torch.randn(B, 23, H, W, generator=gen) * 0.5
    net[:, 4:7] = net[:, 4:7] * 0.3 + np.log(0.01)
    inputs = {"net_out": net, "depth": torch.rand(B, 1, H, W, generator=gen) * 2.0 + 6.667,
              "ray_dirs": torch.cat([torch.rand(1, 2, H, W, generator=gen) * 0.2 - 0.1, torch.ones(1, 1, H, W)], 1),
              "v2w": ob.view_to_world_transforms[idx, 0].contiguous(), "quat": ob.source_cv2wT_quat[idx, 0].contiguous()}
    shapes = {k: (B, HW) + f3d.gaussian_predictor._KEY_SHAPE[k] for k in KEYS}
    cots = {k: torch.randn(shapes[k], generator=gen) for k in KEYS}
    t = {k: v.to(gpu_device).contiguous() for k, v in inputs.items()}
    nan = lambda *s: torch.full(s, float("nan"), device=gpu_device)
    # compact call
    d_net0, d_dep0 = nan(B, 23, H, W), nan(B, 1, H, W)
    _raw_backward(B, H, W, t, 10000.0, HW, 0, [cots[k].to(gpu_device) for k in KEYS], d_net0, d_dep0)
    assert bool(torch.isfinite(d_net0).all()) and bool(torch.isfinite(d_dep0).all())
    g32, g64 = T.restatement_grads(inputs, cots, 10000.0, torch.float32), T.restatement_grads(inputs, cots, 10000.0, torch.float64)
    T.check_groups((d_net0, d_dep0), g32, g64, label=f"abi {B}x{H}x{W}")
    # the window of a three times longer buffer, NaN around it
    wide = []
    for k in KEYS:
        g = nan(B, 3 * HW, *shapes[k][2:])
        g[:, HW:2 * HW] = cots[k].to(gpu_device)
        wide.append(g)
    d_net1, d_dep1 = nan(B, 23, H, W), nan(B, 1, H, W)
    _raw_backward(B, H, W, t, 10000.0, 3 * HW, HW, wide, d_net1, d_dep1)
    assert torch.equal(d_net1, d_net0) and torch.equal(d_dep1, d_dep0)
    # d_depth = NULL
    d_net2 = nan(B, 23, H, W)
    _raw_backward(B, H, W, t, 10000.0, 3 * HW, HW, wide, d_net2, None)
    assert torch.equal(d_net2, d_net0)
    # all-NULL upstream gradients: everything is written, with zeros
    d_net3, d_dep3 = nan(B, 23, H, W), nan(B, 1, H, W)
    _raw_backward(B, H, W, t, 10000.0, HW, 0, [None] * 7, d_net3, d_dep3)
    assert float(d_net3.abs().max()) == 0.0 and float(d_dep3.abs().max()) == 0.0


def test_degenerate_quaternions(gpu_device):
    """A pixel whose rotation channels are exactly 0 (F.normalize's clamp_min(1e-12) is active: the gradient is dq / 1e-12) and one with
    norm 1e-3. These two are compared on their own, relative to max|g64| at that pixel, so that their 1e12 / 1e3 scale does not swamp the
    group maximum; the relative bound is 4 * max(E_ref of that pixel, E_ref of the rotation group over the ordinary pixels) -- a single
    pixel has four values, too few for its own E_ref to be a stable worst case. All other pixels follow the group rule."""
    inputs, cots = _fixture()
    inputs = {k: v.clone() for k, v in inputs.items()}
    zero_px, small_px = (0, 3, 5), (1, 10, 20)
    inputs["net_out"][zero_px[0], 7:11, zero_px[1], zero_px[2]] = 0.0
    q = inputs["net_out"][small_px[0], 7:11, small_px[1], small_px[2]]
    inputs["net_out"][small_px[0], 7:11, small_px[1], small_px[2]] = q / q.norm() * 1e-3
    g32, g64 = T.restatement_grads(inputs, cots, 10000.0, torch.float32), T.restatement_grads(inputs, cots, 10000.0, torch.float64)
    got = _kernel_grads(inputs, cots, 10000.0, gpu_device)
    mask = torch.ones(2, 1, 32, 32, dtype=torch.bool)
    for b, y, x in (zero_px, small_px):
        mask[b, 0, y, x] = False
    fig = T.check_groups(got, g32, g64, label="degenerate/others", mask=mask)
    e_group = fig["rotation"][0]
    for name, (b, y, x) in (("zero", zero_px), ("norm 1e-3", small_px)):
        t64, t32, tk = g64[0][b, 7:11, y, x], g32[0][b, 7:11, y, x].double(), got[0][b, 7:11, y, x].double().cpu()
        m = float(t64.abs().max())
        e_pix, err = float((t32 - t64).abs().max()) / m, float((tk - t64).abs().max()) / m
        print(f"degenerate/{name}: max|g64| {m:.3e}  E_ref(pixel) {e_pix:.3e}  E_ref(group) {e_group:.3e}  kernel {err:.3e}")
        assert bool(torch.isfinite(tk).all()) and m > 0
        assert err <= 4 * max(e_pix, e_group), (name, err, e_pix, e_group)
    assert float(g64[0][zero_px[0], 7:11, zero_px[1], zero_px[2]].abs().max()) > 1e10        # the clamp branch did apply


def test_bit_reproducible(gpu_device):
    inputs, cots = _fixture()
    a = _kernel_grads(inputs, cots, 0.3, gpu_device)
    b = _kernel_grads(inputs, cots, 0.3, gpu_device)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_rasterizer_gradients_reach_net_out(gpu_device):
    """The junction: splat_head -> render_predicted_more_v2_gof -> loss.backward() fills net_out.grad in every channel group.
    (a) With the cotangents the rasterizer's backward delivered to the head's outputs, net_out.grad follows the tolerance rule against
        the float64 restatement.
    (b) It equals the gradient of routing the same net_out through the float32 torch restatement on the GPU into the same renderer call.
        That path's own outputs differ from the kernel's in the last bit and the rasterizer's backward adds with atomics, so it is run
        twice: allowed is the larger of the E_ref bound and twice its observed run-to-run spread (both printed)."""
    dev = gpu_device
    cfg = cameras.default_cfg(32)
    rig = cameras.OrbitRig(cfg)
    cano, ob = rig.canonical, rig.orbit(8)
    gen = torch.Generator().manual_seed(1)
    net0 = torch.randn(1, 23, 32, 32, generator=gen) * 0.5
    net0[:, 4:7] = net0[:, 4:7] * 0.3 + np.log(0.01)
    depth = torch.rand(1, 1, 32, 32, generator=gen) * 2.0 + 6.667
    from oracle import splat_head as sh_oracle
    ray_dirs = torch.from_numpy(sh_oracle.init_ray_dirs(32, cfg["model"]["fov"]))
    inputs = {"net_out": net0, "depth": depth, "ray_dirs": ray_dirs, "v2w": cano.view_to_world_transforms[0, 0].reshape(1, 4, 4),
              "quat": cano.source_cv2wT_quat[0, 0].reshape(1, 4)}
    cam = tuple(t[2:3].to(dev) for t in (ob.world_view_transforms, ob.full_proj_transforms, ob.camera_centers))
    w1 = torch.rand(3, 32, 32, generator=gen).to(dev)
    w2 = torch.rand(1, 32, 32, generator=gen).to(dev)

    def run(head):
        net = net0.to(dev).requires_grad_()
        pc = head(net)
        for k in ("xyz", "opacity", "scaling", "rotation", "features_dc", "features_rest"):
            pc[k].retain_grad()
        r = f3d.render_predicted_more_v2_gof(pc, 0, *cam, torch.zeros(1, 3, device=dev), cfg)
        loss = (r["render"] * w1).sum() + (r["rendered_depth"] * w2).sum()
        loss.backward()
        return net.grad, {k: (pc[k].grad.detach().cpu() if k != "unet_depth" and pc[k].grad is not None else None) for k in KEYS}

    kernel_head = lambda net: f3d.splat_head(net, depth.to(dev), ray_dirs.to(dev), inputs["v2w"].to(dev), inputs["quat"].to(dev))
    torch_head = lambda net: T.splat_head_torch(net, depth.to(dev), ray_dirs, inputs["v2w"], inputs["quat"])
    gk, cots = run(kernel_head)
    assert bool(torch.isfinite(gk).all())
    for name, sl in T.GROUPS.items():
        assert float(gk[:, sl].abs().max()) > 0, name
    # (a) the head's own part, exactly: same cotangents through the float64 restatement
    zero_d = torch.zeros(1, 1, 32, 32)
    g32, g64 = T.restatement_grads(inputs, cots, 10000.0, torch.float32), T.restatement_grads(inputs, cots, 10000.0, torch.float64)
    fig = T.check_groups((gk, zero_d), (g32[0], zero_d), (g64[0], zero_d.double()), label="junction/head")
    # (b) against the restatement routed into the same renderer call
    gt1, _ = run(torch_head)
    gt2, _ = run(torch_head)
    bad = []
    for name, sl in T.GROUPS.items():
        m = float(g64[0][:, sl].abs().max())
        spread = float((gt1[:, sl] - gt2[:, sl]).abs().max())
        diff = float((gk[:, sl] - gt1[:, sl]).abs().max())
        bound = max(4 * fig[name][0] * m, 2 * spread)
        print(f"junction/route {name:8s} |kernel - torch route| {diff:.3e}  run-to-run spread {spread:.3e}  E_ref bound {4 * fig[name][0] * m:.3e}  max|g| {m:.3e}")
        if not diff <= bound:
            bad.append((name, diff, bound))
    assert not bad, bad


class _TinyNet(torch.nn.Module):
    """Stands in for the SongUNet (same call signature): one 1x1 convolution 4 -> 23."""

    def __init__(self):
        super().__init__()
        self.conv = torch.nn.Conv2d(4, 23, 1)

    def forward(self, x, film_camera_emb=None, N_views_xa=1):
        return self.conv(x)


def test_predictor_level(gpu_device):
    """GaussianSplatPredictor_gtunet.forward under grad with a tiny network: the convolution's weight / bias gradients equal those obtained
    through the restatement head (multi_view_union's reshape keeps the graph), and the same forward under no_grad builds no graph and
    leaves no gradient. Truth is the float64 CPU evaluation of the whole chain; errors are taken per parameter tensor and output-channel
    group, relative to that cell's max|g64|. Every cell is the same kind of 4096-term float32 sum and some cells hold one to four
    values, too few for a stable worst case of their own, so E_ref is the largest relative float32 error of the restatement chain over
    all cells, on the CPU and on the GPU (the convolution's own float32 error is part of both); the kernel path passes within 4 * E_ref."""
    dev = gpu_device
    cfg = cameras.default_cfg(32)
    cfg["model"]["base_dim"] = 32
    torch.manual_seed(3)
    pred = f3d.GaussianSplatPredictor_gtunet(cfg).eval()
    pred.network_with_offset = _TinyNet()
    with torch.no_grad():
        pred.network_with_offset.conv.bias[4:7] += float(np.log(0.01))
    pred = pred.to(dev)
    conv = pred.network_with_offset.conv
    B, Nv, HW = 2, 2, 1024
    gen = torch.Generator().manual_seed(4)
    x = torch.rand(B, Nv, 4, 32, 32, generator=gen)
    depth = torch.rand(B * Nv, 1, 32, 32, generator=gen) * 2.0 + 6.667
    ob = cameras.OrbitRig(cfg).orbit(8)
    v2w, quat = ob.view_to_world_transforms[:4, 0].reshape(B, Nv, 4, 4), ob.source_cv2wT_quat[:4, 0].reshape(B, Nv, 4)
    ws = {k: torch.randn((B, Nv * HW) + f3d.gaussian_predictor._KEY_SHAPE[k], generator=gen) for k in KEYS}

    def chain(conv_w, conv_b, device, dtype):
        """conv -> restatement head -> multi-view union -> weighted sum; returns (dL/dweight, dL/dbias)."""
        w, b = conv_w.detach().to(device, dtype).requires_grad_(), conv_b.detach().to(device, dtype).requires_grad_()
        net = torch.nn.functional.conv2d(x.reshape(B * Nv, 4, 32, 32).to(device, dtype), w, b)
        out = T.splat_head_torch(net, depth.to(device, dtype), pred.ray_dirs.cpu(), v2w.reshape(B * Nv, 4, 4), quat.reshape(B * Nv, 4))
        loss = sum((out[k].reshape(ws[k].shape) * ws[k].to(device, dtype)).sum() for k in KEYS)
        return torch.autograd.grad(loss, [w, b])

    out = pred(x.to(dev), v2w.to(dev), quat.to(dev), unet_depth=depth.to(dev))
    assert all(out[k].shape == ws[k].shape and out[k].grad_fn is not None for k in KEYS)
    sum((out[k] * ws[k].to(dev)).sum() for k in KEYS).backward()
    got = (conv.weight.grad.detach().clone(), conv.bias.grad.detach().clone())
    g64 = chain(conv.weight, conv.bias, "cpu", torch.float64)
    c32, d32 = chain(conv.weight, conv.bias, "cpu", torch.float32), chain(conv.weight, conv.bias, dev, torch.float32)
    rel = lambda a, t64, sl: float((a[sl].double().cpu() - t64[sl]).abs().max()) / float(t64[sl].abs().max())
    cells = [(i, name, gname, sl) for i, name in enumerate(("weight", "bias")) for gname, sl in T.GROUPS.items()]
    e_ref = max(max(rel(c32[i], g64[i], sl), rel(d32[i], g64[i], sl)) for i, _, _, sl in cells)
    bad = []
    for i, name, gname, sl in cells:
        err = rel(got[i], g64[i], sl)
        print(f"predictor {name:6s} {gname:8s} kernel path {err:.3e}  torch route cpu {rel(c32[i], g64[i], sl):.3e} gpu {rel(d32[i], g64[i], sl):.3e}  E_ref {e_ref:.3e}")
        if not err <= 4 * e_ref:
            bad.append((name, gname, err))
    assert not bad, (bad, e_ref)
    # inference path: no graph, no gradient, same values
    conv.weight.grad = None
    conv.bias.grad = None
    with torch.no_grad():
        out_ng = pred(x.to(dev), v2w.to(dev), quat.to(dev), unet_depth=depth.to(dev))
    assert all(out_ng[k].grad_fn is None and not out_ng[k].requires_grad for k in KEYS)
    assert conv.weight.grad is None and conv.bias.grad is None
    # (the values are not compared bit for bit: in inference the predictor runs its network channels-last, so the convolution may be
    # another kernel; that the head itself returns the same bits with and without a graph is test_errors_and_inference_forms' job)
    assert all(out_ng[k].shape == out[k].shape and bool(torch.isfinite(out_ng[k]).all()) for k in KEYS)


def test_errors_and_inference_forms(gpu_device):
    dev = gpu_device
    inputs, _ = _fixture()
    t = {k: v.to(dev) for k, v in inputs.items()}
    net = t["net_out"].clone().requires_grad_()
    for name in ("v2w", "quat", "ray_dirs"):
        args = dict(t)
        args[name] = t[name].clone().requires_grad_()
        with pytest.raises(NotImplementedError, match={"v2w": "view_to_world", "quat": "cam_quat", "ray_dirs": "ray_dirs"}[name]):
            f3d.splat_head(net, args["depth"], args["ray_dirs"], args["v2w"], args["quat"])
    from f3dgaus_amd.gaussian_predictor import allocate_gaussians
    merged = allocate_gaussians(2, 3 * 1024, dev)
    with pytest.raises(RuntimeError, match="inference"):
        f3d.splat_head(net, t["depth"], t["ray_dirs"], t["v2w"], t["quat"], out=merged, n_offset=1024)
    with pytest.raises(RuntimeError, match="inference"):
        f3d.splat_head(t["net_out"], t["depth"].clone().requires_grad_(), t["ray_dirs"], t["v2w"], t["quat"], out=merged, n_offset=1024)
    # under no_grad out= still works on a grad-requiring input, and is bit-identical to the allocating call -- with or without autograd
    with torch.no_grad():
        for k in KEYS:
            merged[k].fill_(-7.0)
        f3d.splat_head(net, t["depth"], t["ray_dirs"], t["v2w"], t["quat"], out=merged, n_offset=1024)
        plain = f3d.splat_head(net, t["depth"], t["ray_dirs"], t["v2w"], t["quat"])
    graph = f3d.splat_head(net, t["depth"], t["ray_dirs"], t["v2w"], t["quat"])
    for k in KEYS:
        assert torch.equal(merged[k][:, 1024:2048], plain[k]) and torch.equal(graph[k].detach(), plain[k]), k
        assert float(merged[k][:, :1024].max()) == -7.0 and float(merged[k][:, 2048:].min()) == -7.0
        assert plain[k].grad_fn is None and graph[k].grad_fn is not None
    # depth alone requiring grad: d_depth is produced, net_out gets none
    dep = t["depth"].clone().requires_grad_()
    o = f3d.splat_head(t["net_out"], dep, t["ray_dirs"], t["v2w"], t["quat"])
    (o["xyz"].sum() + o["unet_depth"].sum()).backward()
    assert dep.grad is not None and bool(torch.isfinite(dep.grad).all()) and float(dep.grad.abs().max()) > 0
