"""Training through the cycle aggregation: the hand-off's adjoint kernel (``f3dg_cycle_inputs_backward`` behind ``cycle_inputs``), the
one-node merge of K splat-head passes (``splat_head_merge``) and ``cycle_aggregate(differentiable=True)``.

The two kernels are held bit for bit: the hand-off's adjoint against torch.autograd of the clamp / slices / cat / transpose it replaces,
the merge against K autograd ``splat_head`` calls + ``torch.cat`` (the head kernels are one thread per pixel without atomics).

The loop (route F) is held against the same loop composed in this file from the public pieces that existed before it (route C):
``head=False`` -> ``splat_head`` -> ``render_views(differentiable=True, epilogue=False)`` -> torch clamp / cat / transpose -> V passes ->
``torch.cat`` of the 1 + V ``splat_head`` outputs. Both hand bit-identical inputs to the same kernels, so the merged sets are
``torch.equal``; the gradients differ only by the order of the compositing backward's atomics and of MIOpen's, so their yardstick is
route C run twice. Bar per group (convolution weight, bias, images): max|F - C| / max|C| <= 1e-4, the project's bar for view-summed
gradients; a group whose run-to-run distance of route C, as recorded on an MI355X in ``C_RUN_TO_RUN`` (and DESIGN.md section 3e),
is above 2.5e-5 gets 4 x that recorded distance. The test prints route C's run-to-run distance on every run (``pytest -s``) and uses it
for no bar."""
import numpy as np
import pytest
import torch
import torch.nn as nn

import f3dgaus_amd as f3d
from f3dgaus_amd import _lib, cameras
from f3dgaus_amd.gaussian_predictor import GAUSSIAN_KEYS, _KEY_SHAPE
from f3dgaus_amd.gaussian_renderer import cycle_inputs, render_views

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------ hand-off adjoint
HB, HV, HH, HW_ = 3, 2, 40, 28          # B != V, H != W; 280 float4 per plane: two workgroups, the second partly filled
_SPECIAL = (0.0, 1.0, -0.0, 1.0 + 2.0 ** -23, -1e-30, float("inf"), float("-inf"), float("nan"))
_H = {}


def _handoff(dev):
    if not _H:
        gen = torch.Generator().manual_seed(5)
        r = torch.randn(HB * HV, 9, HH, HW_, generator=gen) * 0.6 + 0.5          # about a third of channels 0..2 outside [0, 1]
        n_pix = HH * HW_
        flat = r.reshape(HB * HV, 9, n_pix)
        # every special value in every colour channel of every frame, in the first and in the (partly filled) second workgroup
        pos = torch.randperm(n_pix, generator=gen)
        lo, hi = pos[pos < 1024], pos[pos >= 1024]
        for n in range(HB * HV):
            for c in range(3):
                for j, val in enumerate(_SPECIAL):
                    flat[n, c, lo[(n * 3 + c) * 8 + j]] = val
                    flat[n, c, hi[((n * 3 + c) * 8 + j) % hi.numel()]] = val
        gx = torch.randn(HV, HB, 4, HH, HW_, generator=gen)
        gz = torch.randn(HV, HB, 1, HH, HW_, generator=gen)
        # non-finite cotangents: under masked and under passing positions alike
        gx_bad = gx.clone()
        sel = torch.rand(gx.shape, generator=gen)
        gx_bad[sel < 0.10] = float("nan")
        gx_bad[(sel >= 0.10) & (sel < 0.15)] = float("inf")
        gx_bad[(sel >= 0.15) & (sel < 0.20)] = float("-inf")
        gz_bad = gz.clone()
        gz_bad[torch.rand(gz.shape, generator=gen) < 0.1] = float("nan")
        _H.update(r=r.to(dev), gx=gx.to(dev), gz=gz.to(dev), gx_bad=gx_bad.to(dev), gz_bad=gz_bad.to(dev))
    return _H


def _torch_handoff(r):
    r5 = r.reshape(HB, HV, 9, HH, HW_)
    return torch.cat([r5[:, :, :3].clamp(0, 1), r5[:, :, 7:8]], 2).transpose(0, 1), r5[:, :, 6:7].transpose(0, 1)


def _bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("used", ["both", "xin", "depth"])
def test_handoff_adjoint_equals_torch_autograd(gpu_device, used):
    h = _handoff(gpu_device)
    r = h["r"].clone().requires_grad_()
    xin, z = cycle_inputs(r, HB, HV)
    assert xin.grad_fn is not None and z.grad_fn is not None and xin.shape == (HV, HB, 4, HH, HW_) and z.shape == (HV, HB, 1, HH, HW_)
    with torch.no_grad():
        xin0, z0 = cycle_inputs(h["r"], HB, HV)
    assert xin0.grad_fn is None and torch.equal(_bits(xin.detach()), _bits(xin0)) and torch.equal(_bits(z.detach()), _bits(z0))
    rr = h["r"].clone().requires_grad_()
    xr, zr = _torch_handoff(rr)
    outs, refs, cots = [], [], []
    if used in ("both", "xin"):
        outs.append(xin); refs.append(xr); cots.append(h["gx"])
    if used in ("both", "depth"):
        outs.append(z); refs.append(zr); cots.append(h["gz"])
    got, = torch.autograd.grad(outs, r, cots)
    ref, = torch.autograd.grad(refs, rr, cots)
    assert got.shape == ref.shape == (HB * HV, 9, HH, HW_)
    assert torch.equal(got, ref)
    assert torch.equal(_bits(got[:, [3, 4, 5, 8]]), torch.zeros_like(_bits(got[:, [3, 4, 5, 8]])))
    if used == "depth":
        assert not bool(_bits(got[:, [0, 1, 2, 7]]).any())
    if used == "xin":
        assert not bool(_bits(got[:, 6]).any())


def test_handoff_adjoint_selects_under_nonfinite_cotangents(gpu_device):
    h = _handoff(gpu_device)
    r = h["r"].clone().requires_grad_()
    xin, z = cycle_inputs(r, HB, HV)
    got, = torch.autograd.grad([xin, z], r, [h["gx_bad"], h["gz_bad"]])
    g = h["gx_bad"].transpose(0, 1).reshape(HB * HV, 4, HH, HW_)          # slot v * B + b -> frame b * V + v
    rgb = h["r"][:, :3]
    mask = (rgb >= 0) & (rgb <= 1)
    # the masks of the special values: 0, 1 and -0.0 pass; the next float above 1, a tiny negative, +-Inf and NaN do not
    probe = torch.tensor(_SPECIAL, device=gpu_device)
    assert ((probe >= 0) & (probe <= 1)).tolist() == [True, True, True, False, False, False, False, False]
    want = torch.where(mask, g[:, :3], torch.zeros_like(g[:, :3]))
    assert torch.equal(_bits(got[:, :3]), _bits(want))                      # the cotangent's own bits where it passes ...
    assert not bool(_bits(got[:, :3])[~mask].any())                         # ... and exactly +0.0 where it does not, NaN / Inf cotangent or not
    assert bool(torch.isnan(g[:, :3][~mask]).any()) and bool(torch.isinf(g[:, :3][~mask]).any()) and bool(torch.isnan(g[:, :3][mask]).any())
    assert torch.equal(_bits(got[:, 7]), _bits(g[:, 3]))
    assert torch.equal(_bits(got[:, 6]), _bits(h["gz_bad"].transpose(0, 1).reshape(HB * HV, HH, HW_)))
    assert not bool(_bits(got[:, [3, 4, 5, 8]]).any())


# ------------------------------------------------------------------------------------------------ merge
MK, MB, MH, MW = 3, 2, 8, 12
_M = {}


def _merge_setup(dev):
    if not _M:
        cfg = cameras.default_cfg(32)
        rig = cameras.OrbitRig(cfg)
        cano, ob = rig.canonical, rig.orbit(8)
        gen = torch.Generator().manual_seed(33)
        nets, depths = [], []
        for _ in range(MK):             # in the style of _setup of tests/test_render_views_autograd_gpu.py
            net = torch.randn(MB, 23, MH, MW, generator=gen) * 0.5
            net[:, 4:7] = net[:, 4:7] * 0.3 + np.log(0.01)
            nets.append(net.to(dev))
            depths.append((torch.rand(MB, 1, MH, MW, generator=gen) * 2.0 + 6.667).to(dev))
        ys, xs = torch.meshgrid(torch.linspace(0.11, -0.11, MH), torch.linspace(-0.17, 0.17, MW), indexing="ij")
        ray_dirs = torch.stack([xs, ys, torch.ones_like(xs)]).unsqueeze(0).to(dev)
        v2ws = [cano.view_to_world_transforms[0, 0]] + [ob.view_to_world_transforms[i, 0] for i in (2, 5)]
        quats = [cano.source_cv2wT_quat[0, 0]] + [ob.source_cv2wT_quat[i, 0] for i in (2, 5)]
        v2ws = [m.reshape(1, 4, 4).repeat(MB, 1, 1).to(dev) for m in v2ws]
        quats = [q.reshape(1, 4).repeat(MB, 1).to(dev) for q in quats]
        w = {k: torch.randn((MB, MK * MH * MW) + _KEY_SHAPE[k], generator=gen).to(dev) for k in GAUSSIAN_KEYS}
        _M.update(nets=nets, depths=depths, ray_dirs=ray_dirs, v2ws=v2ws, quats=quats, w=w)
    return _M


def _leaves(m, depth0_grad=True):
    nets = [t.clone().requires_grad_() for t in m["nets"]]
    depths = [t.clone().requires_grad_(depth0_grad or k > 0) for k, t in enumerate(m["depths"])]
    return nets, depths


@pytest.mark.parametrize("squre_clip", [10000.0, 0.5])
@pytest.mark.parametrize("case", ["all_keys", "xyz_opacity_only", "depth0_is_data"])
def test_merge_equals_k_heads_and_cat(gpu_device, squre_clip, case):
    m = _merge_setup(gpu_device)
    HW = MH * MW
    keys = ("xyz", "opacity") if case == "xyz_opacity_only" else GAUSSIAN_KEYS
    loss = lambda pc: sum((pc[k] * m["w"][k]).sum() for k in keys)
    L = _lib.lib()

    nets, depths = _leaves(m, depth0_grad=case != "depth0_is_data")
    L.f3dg_debug_launch_count(1)
    merged = f3d.splat_head_merge(nets, depths, m["ray_dirs"], m["v2ws"], m["quats"], squre_clip)
    assert L.f3dg_debug_launch_count(1) == MK                       # K head launches, nothing else from the library
    fns = {merged[k].grad_fn for k in GAUSSIAN_KEYS}
    assert len(fns) == 1 and None not in fns                        # ONE autograd node
    # forward: the out= / n_offset loop
    with torch.no_grad():
        loop = f3d.gaussian_predictor.allocate_gaussians(MB, MK * HW, gpu_device)
        for k in range(MK):
            f3d.splat_head(m["nets"][k], m["depths"][k], m["ray_dirs"], m["v2ws"][k], m["quats"][k], squre_clip, out=loop, n_offset=k * HW)
        plain = f3d.splat_head_merge(m["nets"], m["depths"], m["ray_dirs"], m["v2ws"], m["quats"], squre_clip)
    for k in GAUSSIAN_KEYS:
        assert merged[k].shape == (MB, MK * HW) + _KEY_SHAPE[k], k
        assert torch.equal(_bits(merged[k].detach()), _bits(loop[k])) and torch.equal(_bits(plain[k]), _bits(loop[k])), k
        assert plain[k].grad_fn is None
    if squre_clip < 10:
        assert bool((loop["xyz"][..., :2].abs() == squre_clip).any()) and bool((loop["xyz"][..., :2].abs() < squre_clip).any())
    L.f3dg_debug_launch_count(1)
    loss(merged).backward()
    assert L.f3dg_debug_launch_count(1) == MK                       # K backward launches on the merged cotangents

    rn, rd = _leaves(m, depth0_grad=case != "depth0_is_data")
    sets = [f3d.splat_head(rn[k], rd[k], m["ray_dirs"], m["v2ws"][k], m["quats"][k], squre_clip) for k in range(MK)]
    loss({k: torch.cat([s[k] for s in sets], 1) for k in GAUSSIAN_KEYS}).backward()
    for k in range(MK):
        assert torch.equal(nets[k].grad, rn[k].grad), k
        assert float(nets[k].grad.abs().max()) > 0
        if k == 0 and case == "depth0_is_data":
            assert depths[0].grad is None and rd[0].grad is None
        else:
            assert torch.equal(depths[k].grad, rd[k].grad), k
            assert float(depths[k].grad.abs().max()) > 0


def test_merge_skips_passes_of_data_and_refuses_cameras(gpu_device):
    m = _merge_setup(gpu_device)
    L = _lib.lib()
    nets = [m["nets"][0], m["nets"][1].clone().requires_grad_(), m["nets"][2]]
    depths = [m["depths"][0], m["depths"][1], m["depths"][2].clone().requires_grad_()]
    merged = f3d.splat_head_merge(nets, depths, m["ray_dirs"], m["v2ws"], m["quats"])
    L.f3dg_debug_launch_count(1)
    sum((merged[k] * m["w"][k]).sum() for k in GAUSSIAN_KEYS).backward()
    assert L.f3dg_debug_launch_count(1) == 2                        # pass 0 holds data only: no launch for it
    assert nets[1].grad is not None and depths[2].grad is not None and depths[1].grad is None
    rn, rd = m["nets"][1].clone().requires_grad_(), m["depths"][2].clone().requires_grad_()
    a = f3d.splat_head(rn, m["depths"][1], m["ray_dirs"], m["v2ws"][1], m["quats"][1])
    b = f3d.splat_head(m["nets"][2], rd, m["ray_dirs"], m["v2ws"][2], m["quats"][2])
    HW = MH * MW
    (sum((a[k] * m["w"][k][:, HW:2 * HW]).sum() for k in GAUSSIAN_KEYS) + sum((b[k] * m["w"][k][:, 2 * HW:]).sum() for k in GAUSSIAN_KEYS)).backward()
    assert torch.equal(nets[1].grad, rn.grad) and torch.equal(depths[2].grad, rd.grad)

    nets, depths = _leaves(m)
    for name, which, i in (("view_to_worlds", "v2ws", 1), ("cam_quats", "quats", 2)):
        cams = {"v2ws": list(m["v2ws"]), "quats": list(m["quats"])}
        cams[which][i] = cams[which][i].clone().requires_grad_()
        with pytest.raises(NotImplementedError, match=name + r"\[%d\]" % i):
            f3d.splat_head_merge(nets, depths, m["ray_dirs"], cams["v2ws"], cams["quats"])
    with pytest.raises(NotImplementedError, match="ray_dirs"):
        f3d.splat_head_merge(nets, depths, m["ray_dirs"].clone().requires_grad_(), m["v2ws"], m["quats"])


# ------------------------------------------------------------------------------------------------ the loop
RES, LB, LV = 32, 2, 2
GROUPS = ("weight", "bias", "images")
# max|C - C'| / max|C| of route C run twice, per group, as measured on an MI355X. A group above 2.5e-5 is held
# to 4 x its figure here, every other one to 1e-4: constants, so that a noisier route cannot widen its own bar.
C_RUN_TO_RUN = {"full": {"weight": 2.641e-07, "bias": 0.0, "images": 0.0},
                "detached": {"weight": 3.302e-07, "bias": 0.0, "images": 0.0}}
_L = {}


def _bar(label, name):
    d = C_RUN_TO_RUN[label][name]
    return 4 * d if d > 2.5e-5 else 1e-4


class _StandIn(nn.Module):
    """One seeded 3 x 3 convolution in place of the SongUNet backbone (one convolution shape for MIOpen to find)."""

    def __init__(self):
        super().__init__()
        self.conv = nn.Conv2d(4, 23, 3, padding=1)
        gen = torch.Generator().manual_seed(77)
        with torch.no_grad():
            w = torch.randn(23, 4, 3, 3, generator=gen) * 0.15
            w[4:7] *= 0.3
            b = torch.randn(23, generator=gen) * 0.1
            b[4:7] = float(np.log(0.01))            # the scale channels where _setup of tests/test_render_views_autograd_gpu.py puts them
            self.conv.weight.copy_(w)
            self.conv.bias.copy_(b)

    def forward(self, x, film_camera_emb=None, N_views_xa=1):
        return self.conv(x)


def _loop_setup(dev):
    if not _L:
        cfg = cameras.default_cfg(RES)
        cfg["model"]["backbone_layout"] = "nchw"        # (the inference calls convolve in the layout of the autograd ones: one MIOpen problem)
        model = f3d.Unet_GS_gtunet(cfg, renderer=None).eval()
        model.gaussian_predictor.network_with_offset = _StandIn()
        model = model.to(dev)
        rig = cameras.OrbitRig(cfg)
        ob = rig.orbit(8)
        gen = torch.Generator().manual_seed(91)
        images = torch.rand(LB, 3, RES, RES, generator=gen).to(dev)
        depth = (torch.rand(LB, 1, RES, RES, generator=gen) * 2.0 + 6.667).to(dev)
        cams = tuple(t[[2, 5], 0].contiguous().to(dev) for t in (ob.world_view_transforms, ob.full_proj_transforms, ob.camera_centers))
        w = {k: torch.randn(LB * 2, c, RES, RES, generator=gen).to(dev) for k, c in (("render", 3), ("rendered_depth", 1), ("rendered_alpha", 1))}
        _L.update(cfg=cfg, model=model, rig=rig, images=images, depth=depth, cams=cams, w=w, bg=torch.tensor([0.2, 0.5, 0.3], device=dev))
    return _L


def _route_f(s, images, **kw):
    return f3d.cycle.cycle_aggregate(s["model"], images, s["depth"], s["cfg"], rig=s["rig"], num_views=LV, differentiable=True, **kw)


def _route_c(s, images, detach=False):
    """The loop of cycle_aggregate from the public pieces that were there before it."""
    model, cfg, dev = s["model"], s["cfg"], images.device
    cano, orbit = s["rig"].canonical, s["rig"].orbit(LV, 0.25, 0.15)
    bg0 = torch.zeros(3, device=dev)
    clip = cfg["opt"]["squre_clip"]
    ray_dirs = model.gaussian_predictor.ray_dirs
    x0 = torch.cat([images, torch.ones_like(images[:, :1])], 1).unsqueeze(1)
    v2w0 = cano.view_to_world_transforms.reshape(1, 1, 4, 4).expand(LB, 1, 4, 4).to(dev)
    q0 = cano.source_cv2wT_quat.reshape(1, 1, 4).expand(LB, 1, 4).to(dev)
    net0, d0 = model(x0, bg0, v2w0, q0, squre_clip=clip, unet_depth=s["depth"], head=False)
    sets = [f3d.splat_head(net0, d0, ray_dirs, v2w0.reshape(LB, 4, 4), q0.reshape(LB, 4), clip)]
    wv, fp, cc = (t.to(dev) for t in (orbit.world_view_transforms, orbit.full_proj_transforms, orbit.camera_centers))
    r = render_views(sets[0], None, wv, fp, cc, bg0, cfg, differentiable=True, epilogue=False)["raster"]
    r5 = r.reshape(LB, LV, 9, RES, RES)
    xin = torch.cat([r5[:, :, :3].clamp(0, 1), r5[:, :, 7:8]], 2).transpose(0, 1)
    zmed = r5[:, :, 6:7].transpose(0, 1)
    if detach:
        xin, zmed = xin.detach(), zmed.detach()
    v2w, quat = orbit.view_to_world_transforms.to(dev), orbit.source_cv2wT_quat.to(dev)
    for v in range(LV):
        cam, q = v2w[v:v + 1].expand(LB, 1, 4, 4), quat[v:v + 1].expand(LB, 1, 4)
        net, d = model(xin[v].unsqueeze(1), bg0, cam, q, squre_clip=clip, unet_depth=zmed[v], head=False)
        sets.append(f3d.splat_head(net, d, ray_dirs, cam.reshape(LB, 4, 4), q.reshape(LB, 4), clip))
    return {k: torch.cat([t[k] for t in sets], 1) for k in GAUSSIAN_KEYS}


def _grads(s, route, **kw):
    """(merged set detached, {group: gradient}) of the seeded linear functional of the merged set's render from two cameras."""
    conv = s["model"].gaussian_predictor.network_with_offset.conv
    images = s["images"].clone().requires_grad_()
    merged = route(s, images, **kw)
    out = render_views(merged, None, *s["cams"], s["bg"], s["cfg"], differentiable=True)
    loss = sum((out[k] * s["w"][k]).sum() for k in s["w"])
    g = torch.autograd.grad(loss, [conv.weight, conv.bias, images])
    return {k: v.detach() for k, v in merged.items()}, dict(zip(GROUPS, g))


def _dist(a, b):
    return {n: float((a[n] - b[n]).abs().max()) / float(b[n].abs().max()) for n in GROUPS}


def _routes(dev):
    """Every route once, shared by the tests below and left unchanged."""
    s = _loop_setup(dev)
    if "runs" not in _L:
        _L["runs"] = dict(F=_grads(s, _route_f), C=_grads(s, _route_c), C2=_grads(s, _route_c),
                          Fd=_grads(s, _route_f, grad_through_renders=False), Cd=_grads(s, _route_c, detach=True),
                          Cd2=_grads(s, _route_c, detach=True))
    return s, _L["runs"]


def test_loop_forward_equals_the_composition(gpu_device):
    s, runs = _routes(gpu_device)
    N = (1 + LV) * RES * RES
    for k in GAUSSIAN_KEYS:
        assert runs["F"][0][k].shape == (LB, N) + _KEY_SHAPE[k], k
        assert torch.equal(runs["C"][0][k], runs["C2"][0][k]), ("route C is not bit-reproducible in its forward", k)
        assert torch.equal(runs["F"][0][k], runs["C"][0][k]), k
        assert torch.equal(runs["Fd"][0][k], runs["C"][0][k]), k          # detaching changes no forward value


@pytest.mark.parametrize("label", ["full", "detached"])
def test_loop_gradients_match_the_composition(gpu_device, label):
    s, runs = _routes(gpu_device)
    F, Cr, C2 = (runs[n][1] for n in (("F", "C", "C2") if label == "full" else ("Fd", "Cd", "Cd2")))
    for n in GROUPS:
        assert bool(torch.isfinite(F[n]).all()) and float(F[n].abs().max()) > 0, n
    noise, err = _dist(C2, Cr), _dist(F, Cr)
    for n in GROUPS:
        print(f"{label:8s} {n:7s} max|C| {float(Cr[n].abs().max()):.3e}  route C run to run {noise[n]:.3e}  |F - C| / max|C| {err[n]:.3e}  "
              f"bar {_bar(label, n):.3e}")
    bad = [(n, err[n], _bar(label, n)) for n in GROUPS if not err[n] <= _bar(label, n)]
    assert not bad, (label, bad)
    if label == "detached":         # the renders as data is another gradient: pass 0 loses what came back through the hand-off
        far = _dist(runs["Fd"][1], runs["F"][1])
        print("detached vs full: " + "  ".join(f"{n} {far[n]:.3e}" for n in GROUPS))
        assert all(far[n] > _bar("full", n) for n in GROUPS), far


def test_loop_inference_forms(gpu_device):
    s = _loop_setup(gpu_device)
    args = (s["model"], s["images"], s["depth"], s["cfg"])
    with torch.no_grad():
        a, ra = f3d.cycle.cycle_aggregate(*args, rig=s["rig"], num_views=LV, differentiable=True, return_renders=True)
        b, rb = f3d.cycle.cycle_aggregate(*args, rig=s["rig"], num_views=LV, return_renders=True)
    for k in GAUSSIAN_KEYS:
        assert torch.equal(a[k], b[k]) and a[k].grad_fn is None, k
    for k in ("rgb", "alpha", "depth"):
        assert torch.equal(ra[k], rb[k]), k
    # the default call with grad mode on, parameters and images that require grad: still the inference call
    c, rc = f3d.cycle.cycle_aggregate(s["model"], s["images"].clone().requires_grad_(), s["depth"], s["cfg"], rig=s["rig"], num_views=LV,
                                      return_renders=True)
    for k in GAUSSIAN_KEYS:
        assert c[k].grad_fn is None and not c[k].requires_grad and torch.equal(c[k], b[k]), k
    assert all(t.grad_fn is None for t in rc.values())


def test_loop_keeps_its_own_workspace_and_returns_renders(gpu_device):
    """A differentiable render after ``cycle_aggregate(differentiable=True)`` leaves the novel-view render inside the loop its auxiliary
    planes (that render has a workspace of its own): ``backward()`` through both does not raise."""
    s = _loop_setup(gpu_device)
    images = s["images"].clone().requires_grad_()
    merged, renders = _route_f(s, images, return_renders=True)
    assert renders["rgb"].shape == (LB, LV, 3, RES, RES) and renders["depth"].shape == (LB, LV, 1, RES, RES)
    assert renders["rgb"].grad_fn is not None and merged["xyz"].grad_fn is not None
    out = render_views(merged, None, *s["cams"], s["bg"], s["cfg"], differentiable=True, epilogue=False)
    conv = s["model"].gaussian_predictor.network_with_offset.conv
    g = torch.autograd.grad((out["render"] * s["w"]["render"]).sum() + renders["alpha"].sum(), [conv.weight, images])
    assert all(bool(torch.isfinite(t).all()) and float(t.abs().max()) > 0 for t in g)
