"""``render_views(..., differentiable=True)``: B sets x V views through ONE forward and ONE backward launch sequence
(``_RasterizeViews``: f3dg_forward_sets + the fused epilogue, f3dg_render_epilogue_backward + f3dg_backward_sets) against the existing
differentiable route -- ``render_predicted_more_v2_gof`` per (image, view): the torch epilogue and the one-view backward.

B = 2 sets of 32 x 32 pixel-ordered Gaussians from ``splat_head`` of a seeded ``net_out`` that requires grad, V = 2 cameras at
32 x 32; the loss is a seeded linear functional of ``render``, ``rendered_normal``, ``depth_normal``, ``rendered_depth`` and
``distortion_map``. Bar: ``net_out.grad`` within 1e-4 of its maximum per channel group -- the project's bar for view-summed
gradients (tests/test_raster_backward_gpu.py::test_multi_view_backward_sums_single_view_backwards) --, except for a group in which the
one-view route ITSELF is farther than 1e-4 from a float64 chain: there the bar is twice that route's recorded distance.

That distance (``_route_error``): the one-view route is repeated at the raw level, per (image, view), with every stage that can be
evaluated in float64 on the host evaluated there: the epilogue and its adjoint by ``epilogue_truth.epilogue_torch`` (the raster's
cotangent, rounded to float32 once), the compositing backward by the library (``rasterize_views(save_aux=True)`` +
``rasterize_backward_raw``: its per-view dL_dview2gaussian / dL_dcolors are held to 1e-5 of the oracle elsewhere), the per-Gaussian stage
by ``grad_truth.per_gaussian_truth``, the splat head by ``splat_head_truth.restatement_grads``. The per-Gaussian stage is
cancellation-dominated in float32 for the scale and rotation gradients (1 / s^2 = 1e4 at these scales; SURVEY 0.9,
tests/test_raster_backward_gpu.py holds them to floors of 0.4 and 2e-2), and the two routes hand it cotangents that differ in the last
bits (fused epilogue adjoint against ~20 torch kernels), so those two groups are where the 1e-4 cannot be expected of either route.
The figures are recorded in ``ROUTE_ERROR`` below and in DESIGN.md section 3d, and the bars are constants; the tests print the distance of
both routes again on every run (``pytest -s``) without using it for a bar."""
import copy

import numpy as np
import pytest
import torch

import f3dgaus_amd as f3d
from f3dgaus_amd import cameras
from f3dgaus_amd.diff_gof_rasterization.backward import rasterize_backward_raw
from grad_truth import per_gaussian_truth
import epilogue_truth as E
import splat_head_truth as T

pytestmark = pytest.mark.gpu
B, V, RES = 2, 2, 32
MAPS = {"render": 3, "rendered_normal": 3, "depth_normal": 3, "rendered_depth": 1, "distortion_map": 1}
_CACHE = {}


def _setup(dev):
    if "s" not in _CACHE:
        cfg = cameras.default_cfg(RES)
        rig = cameras.OrbitRig(cfg)
        cano, ob = rig.canonical, rig.orbit(8)
        gen = torch.Generator().manual_seed(21)
        net0 = torch.randn(B, 23, RES, RES, generator=gen) * 0.5
        net0[:, 4:7] = net0[:, 4:7] * 0.3 + np.log(0.01)
        depth = torch.rand(B, 1, RES, RES, generator=gen) * 2.0 + 6.667
        from oracle import splat_head as sh_oracle
        ray_dirs = torch.from_numpy(sh_oracle.init_ray_dirs(RES, cfg["model"]["fov"]))
        v2w = cano.view_to_world_transforms[0, 0].reshape(1, 4, 4).repeat(B, 1, 1)
        quat = cano.source_cv2wT_quat[0, 0].reshape(1, 4).repeat(B, 1)
        cams = tuple(t[[2, 5], 0].contiguous().to(dev) for t in (ob.world_view_transforms, ob.full_proj_transforms, ob.camera_centers))
        w = {k: torch.randn(B * V, c, RES, RES, generator=gen).to(dev) for k, c in MAPS.items()}
        _CACHE["s"] = dict(cfg=cfg, net0=net0, depth=depth.to(dev), ray_dirs=ray_dirs.to(dev), v2w=v2w.to(dev), quat=quat.to(dev), cams=cams, w=w,
                           bg=torch.tensor([0.2, 0.5, 0.3], device=dev))
    return _CACHE["s"]


def _head(s, net):
    return f3d.splat_head(net, s["depth"], s["ray_dirs"], s["v2w"], s["quat"])


def _batched(s, dev, bs=None, **kw):
    net = s["net0"].to(dev).requires_grad_()
    out = f3d.render_views(_head(s, net), bs, *s["cams"], s["bg"], s["cfg"], differentiable=True, **kw)
    return net, out


def _loss(out, w, frames):
    return sum((out[k] * w[k][frames]).sum() for k in MAPS)


def _one_view_route(s, dev, images):
    """The same loss accumulated over render_predicted_more_v2_gof per (image, view)."""
    net = s["net0"].to(dev).requires_grad_()
    pc = _head(s, net)
    loss = 0
    for b in images:
        for v in range(V):
            r = f3d.render_predicted_more_v2_gof(pc, b, *(t[v] for t in s["cams"]), s["bg"], s["cfg"])
            loss = loss + sum((r[k] * s["w"][k][b * V + v]).sum() for k in MAPS)
    loss.backward()
    return net.grad.detach().clone()


def _route_error(s, dev, images, route_grad):
    """Per channel group: max|route_grad - g64| / max|g64| over ``images``, g64 the float64 chain (per-Gaussian stage + splat head) from the
    one-view route's own float32 compositing-stage gradients. See the module docstring."""
    cfg = s["cfg"]
    fov = cfg["model"]["fov"] * np.pi / 180
    tan = float(np.tan(cfg["model"]["fov"] * np.pi / 360))
    with torch.no_grad():
        pc = _head(s, s["net0"].to(dev))
    HW = RES * RES
    cots = {k: torch.zeros((B, HW) + f3d.gaussian_predictor._KEY_SHAPE[k], dtype=torch.float64) for k in T.KEYS}
    wv, fp, cc = s["cams"]
    for b in images:
        shs = torch.cat([pc["features_dc"][b], pc["features_rest"][b]], 1).contiguous()
        scene = dict(means3D=pc["xyz"][b].cpu(), scales=pc["scaling"][b].cpu(), rotations=pc["rotation"][b].cpu(), shs=shs.cpu(),
                     viewmatrix=wv.cpu(), campos=cc.cpu(), sh_degree=1)
        for v in range(V):
            raster, radii, ws = f3d.rasterize_views(pc["xyz"][b], pc["opacity"][b], wv[v:v + 1], fp[v:v + 1], cc[v:v + 1], s["bg"],
                                                    image_height=RES, image_width=RES, tanfovx=tan, tanfovy=tan, sh=shs,
                                                    scales=pc["scaling"][b], rotations=pc["rotation"][b], sh_degree=1, save_aux=True)
            leaf = raster[0].detach().cpu().double().requires_grad_()         # the epilogue and its adjoint in float64 on the host
            nw, dn = E.epilogue_torch(leaf, wv[v].cpu(), RES, RES, fov, fov)
            maps = {"render": leaf[:3], "rendered_normal": nw, "depth_normal": dn, "rendered_depth": leaf[6:7], "distortion_map": leaf[8:9]}
            dpix, = torch.autograd.grad(sum((maps[k] * s["w"][k][b * V + v].cpu().double()).sum() for k in MAPS), leaf)
            dpix = dpix.float().to(dev)
            g = rasterize_backward_raw(ws, pc["xyz"][b], shs, None, pc["scaling"][b], pc["rotation"][b], radii, dpix[None], 1,
                                       wv[v:v + 1], fp[v:v + 1], cc[v:v + 1], s["bg"], tan, tan, 0.0, 1.0)
            t = per_gaussian_truth(scene, v, radii[0].cpu().numpy(), g["dL_dview2gaussian"][0].cpu().numpy(), g["dL_dcolors"][0].cpu().numpy())
            cots["xyz"][b] += torch.from_numpy(t["dL_dmean3D"])
            cots["scaling"][b] += torch.from_numpy(t["dL_dscale"])
            cots["rotation"][b] += torch.from_numpy(t["dL_drot"])
            cots["features_dc"][b] += torch.from_numpy(t["dL_dsh"][:, :1])
            cots["features_rest"][b] += torch.from_numpy(t["dL_dsh"][:, 1:4])
            cots["opacity"][b] += g["dL_dopacity"].double().cpu()           # (a compositing-stage sum: not part of the per-Gaussian chain)
    inputs = {"net_out": s["net0"], "depth": s["depth"].cpu(), "ray_dirs": s["ray_dirs"].cpu(), "v2w": s["v2w"].cpu(), "quat": s["quat"].cpu()}
    g64 = T.restatement_grads(inputs, cots, 10000.0, torch.float64)[0][list(images)]
    got = route_grad[list(images)].double().cpu()
    return {name: float((got[:, sl] - g64[:, sl]).abs().max()) / float(g64[:, sl].abs().max()) for name, sl in T.GROUPS.items()}


# max|one-view route - float64 chain| / max|float64 chain| of the groups in which it exceeds 1e-4, as ``_route_error`` gave it on an
# MI355X (DESIGN.md section 3d has every group's figure). The bars below are twice these: constants, so that a route that gets worse
# cannot widen them.
ROUTE_ERROR = {"bs=None": {"scaling": 1.491e-2, "rotation": 3.132e-3},        # maxima over both images
               "bs=1": {"scaling": 1.180e-2, "rotation": 8.090e-3}}             # over image 1 alone


def _bar(label, name):
    return 2 * ROUTE_ERROR[label][name] if name in ROUTE_ERROR[label] else 1e-4


def _compare(got, ref, label):
    bad = []
    for name, sl in T.GROUPS.items():
        m = float(ref[:, sl].abs().max())
        e = float((got[:, sl] - ref[:, sl]).abs().max()) / m
        print(f"{label} {name:8s} max|g| {m:.3e}  |batched - one-view route| / max {e:.3e}  bar {_bar(label, name):.3e}")
        if not e <= _bar(label, name):
            bad.append((name, e, _bar(label, name)))
    assert not bad, (label, bad)


def _print_route_errors(s, dev, images, label, **routes):
    """For the record (``pytest -s``): each route's distance from the float64 chain, per group. The chain is itself checked where it is
    well conditioned -- opacity passes through, dL_dsh is linear in dL_dcolors (held to 1e-5 of the float64 chain rule by
    test_backward_vs_oracle): a chain wired wrongly shows there."""
    for rname, grad in routes.items():
        err = _route_error(s, dev, images, grad)
        print(f"{label} {rname} route vs float64 chain: " + "  ".join(f"{k} {v:.3e}" for k, v in err.items()))
        assert all(err[k] <= 1e-4 for k in ("opacity", "dc", "rest")), (rname, err)


def test_all_sets_match_the_one_view_route(gpu_device):
    s = _setup(gpu_device)
    net, out = _batched(s, gpu_device)
    for k, c in MAPS.items():
        assert out[k].shape == (B * V, c, RES, RES) and out[k].grad_fn is not None, k
    assert out["raster"].grad_fn is not None and out["rendered_alpha"].grad_fn is not None and not out["radii"].requires_grad
    _loss(out, s["w"], slice(None)).backward()
    got = net.grad.detach().clone()
    assert bool(torch.isfinite(got).all())
    for name, sl in T.GROUPS.items():
        assert float(got[:, sl].abs().max()) > 0, name
    ref = _one_view_route(s, gpu_device, range(B))
    _print_route_errors(s, gpu_device, range(B), "bs=None", one_view=ref, batched=got)
    _compare(got, ref, "bs=None")
    # the forward maps: bit-identical to the inference call in the reference arithmetic
    cfg = copy.deepcopy(s["cfg"])
    cfg["model"]["raster_exact"] = True
    with torch.no_grad():
        inf = f3d.render_views(_head(s, s["net0"].to(gpu_device)), None, *s["cams"], s["bg"], cfg)
    for k in list(MAPS) + ["rendered_alpha", "raster", "radii"]:
        assert torch.equal(out[k].detach(), inf[k]), k


def test_one_set_matches_the_one_view_route(gpu_device):
    s = _setup(gpu_device)
    net, out = _batched(s, gpu_device, bs=1)
    assert out["render"].shape == (V, 3, RES, RES)
    _loss(out, s["w"], slice(V, 2 * V)).backward()
    got = net.grad.detach().clone()
    assert float(got[0].abs().max()) == 0.0             # image 0 is not rendered
    ref = _one_view_route(s, gpu_device, [1])
    _print_route_errors(s, gpu_device, [1], "bs=1", one_view=ref, batched=got)
    _compare(got[1:], ref[1:], "bs=1")


def test_argument_errors(gpu_device):
    s = _setup(gpu_device)
    net = s["net0"].to(gpu_device).requires_grad_()
    pc = _head(s, net)
    with pytest.raises(RuntimeError, match="rgb_depth_alpha|channels"):
        f3d.render_views(pc, None, *s["cams"], s["bg"], s["cfg"], differentiable=True, channels="rgb_depth_alpha")
    for i, name in enumerate(("viewmatrices", "projmatrices", "camposs")):
        cams = list(s["cams"])
        cams[i] = cams[i].clone().requires_grad_()
        with pytest.raises(NotImplementedError, match=name):
            f3d.render_views(pc, None, *cams, s["bg"], s["cfg"], differentiable=True)
    with pytest.raises(NotImplementedError, match="bg"):
        f3d.render_views(pc, None, *s["cams"], s["bg"].clone().requires_grad_(), s["cfg"], differentiable=True)


def test_keywords_of_the_inference_call(gpu_device):
    """``epilogue=False``: no derived maps, the raster still differentiable; ``check=False`` raises (the status is always read)."""
    s = _setup(gpu_device)
    net, out = _batched(s, gpu_device, epilogue=False)
    assert out["rendered_normal"] is None and out["depth_normal"] is None and out["raster"].grad_fn is not None
    (out["raster"] * torch.cat([s["w"]["render"]] * 3, 1)).sum().backward()
    net2, full = _batched(s, gpu_device)
    assert torch.equal(out["raster"].detach(), full["raster"].detach())
    (full["raster"] * torch.cat([s["w"]["render"]] * 3, 1)).sum().backward()
    assert torch.equal(net.grad, net2.grad)                     # same kernels on the same cotangent
    with pytest.raises(RuntimeError, match="check"):
        _batched(s, gpu_device, check=False)


def test_raw_backward_refuses_another_set_count(gpu_device):
    """``rasterize_backward_raw(n_sets=1)`` with ONE set's tensors on a workspace whose forward rendered two sets: every shape agrees
    (means3D has P rows), so only the set count recorded by the forward can tell."""
    s = _setup(gpu_device)
    with torch.no_grad():
        pc = _head(s, s["net0"].to(gpu_device))
    tan = float(np.tan(s["cfg"]["model"]["fov"] * np.pi / 360))
    flat = lambda t: t.reshape((-1,) + tuple(t.shape[2:]))
    shs = torch.cat([pc["features_dc"], pc["features_rest"]], 2).contiguous()
    wv, fp, cc = (t.reshape(V, -1).repeat(B, 1) for t in s["cams"])
    raster, radii, ws = f3d.rasterize_views(flat(pc["xyz"]), flat(pc["opacity"]), wv, fp, cc, s["bg"], image_height=RES, image_width=RES,
                                            tanfovx=tan, tanfovy=tan, sh=flat(shs), scales=flat(pc["scaling"]), rotations=flat(pc["rotation"]),
                                            sh_degree=1, save_aux=True, n_sets=B)
    assert ws.n_sets == B
    with pytest.raises(RuntimeError, match="last forward rendered"):
        rasterize_backward_raw(ws, pc["xyz"][0], shs[0], None, pc["scaling"][0], pc["rotation"][0], radii, torch.zeros_like(raster), 1,
                               wv, fp, cc, s["bg"], tan, tan, 0.0, 1.0)


def test_stale_workspace_makes_the_backward_raise(gpu_device):
    s = _setup(gpu_device)
    net, out = _batched(s, gpu_device)
    ws = out["workspace"]
    net2, out2 = _batched(s, gpu_device, workspace=ws)          # a second forward on the same workspace before the first backward
    assert out2["workspace"] is ws
    with pytest.raises(RuntimeError, match="workspace"):
        out["render"].sum().backward()
    assert net.grad is None
    out2["render"].sum().backward()                             # the planes are the second forward's: its backward runs
    assert net2.grad is not None and float(net2.grad.abs().max()) > 0


def test_no_grad_is_the_inference_call(gpu_device):
    s = _setup(gpu_device)
    net = s["net0"].to(gpu_device).requires_grad_()
    with torch.no_grad():
        pc = _head(s, net)
        a = f3d.render_views(pc, None, *s["cams"], s["bg"], s["cfg"], differentiable=True)
        b = f3d.render_views(pc, None, *s["cams"], s["bg"], s["cfg"])
    for k in list(MAPS) + ["rendered_alpha", "raster", "radii"]:
        assert torch.equal(a[k], b[k]) and a[k].grad_fn is None, k
