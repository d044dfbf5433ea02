"""GPU parity of the host-facing operators: splat head kernel, renderer wrapper / epilogue kernel, drop-in API shapes,
mark_visible, the batched cycle loop vs the reference-shaped per-view loop."""
import math
import os

import numpy as np
import pytest
import torch

import f3dgaus_amd as f3d
from f3dgaus_amd import cameras, synthetic
from helpers import assert_render_parity, make_scene, run_oracle
from oracle import splat_head as sh_oracle

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
KEYS = ("xyz", "opacity", "scaling", "rotation", "features_dc", "features_rest", "unet_depth")


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.abs(a - b).max() / max(1.0, np.abs(b).max())


def test_splat_head_kernel_vs_reference_fixture(gpu_device):
    g = np.load(os.path.join(GOLD, "splat_head.npz"))
    t = lambda k: torch.from_numpy(g[k]).to(gpu_device)
    out = f3d.splat_head(t("net_out"), t("depth"), t("ray_dirs"), t("v2w"), t("quat"))
    for k in KEYS:
        assert out[k].shape == g["out_" + k].shape, k
        assert _rel(out[k].cpu().numpy(), g["out_" + k]) < 3e-6, (k, _rel(out[k].cpu().numpy(), g["out_" + k]))
    gc = np.load(os.path.join(GOLD, "splat_head_clip.npz"))
    outc = f3d.splat_head(t("net_out"), t("depth"), t("ray_dirs"), t("v2w"), t("quat"), squre_clip=0.3)
    assert _rel(outc["xyz"].cpu().numpy(), gc["out_xyz"]) < 3e-6


def test_splat_head_full_size_vs_oracle_and_in_place_aggregation(gpu_device):
    B, res = 3, 256
    g = torch.Generator().manual_seed(7)
    net = torch.randn(B, 23, res, res, generator=g) * 0.5
    depth = torch.rand(B, 1, res, res, generator=g) * 2 + 6.667
    rig = cameras.OrbitRig(cameras.default_cfg())
    ob = rig.orbit(8)
    v2w, quat = ob.view_to_world_transforms[[1, 4, 6], 0], ob.source_cv2wT_quat[[1, 4, 6], 0]
    rd = torch.from_numpy(sh_oracle.init_ray_dirs(res, 13.164))
    want = sh_oracle.splat_head(net.numpy(), depth.numpy(), rd.numpy(), v2w.numpy(), quat.numpy())
    out = f3d.splat_head(net.to(gpu_device), depth.to(gpu_device), rd.to(gpu_device), v2w.to(gpu_device), quat.to(gpu_device))
    for k in KEYS:
        assert _rel(out[k].cpu().numpy(), want[k]) < 3e-6, k
    # in-place write at an offset of a larger aggregated buffer (what replaces the torch.cat chain)
    from f3dgaus_amd.gaussian_predictor import allocate_gaussians
    HW = res * res
    merged = allocate_gaussians(B, 3 * HW, gpu_device)
    for k in KEYS:
        merged[k].fill_(-7.0)
    f3d.splat_head(net.to(gpu_device), depth.to(gpu_device), rd.to(gpu_device), v2w.to(gpu_device), quat.to(gpu_device),
                   out=merged, n_offset=HW)
    for k in KEYS:
        assert torch.equal(merged[k][:, HW:2 * HW], out[k]), k
        assert float(merged[k][:, :HW].max()) == -7.0 and float(merged[k][:, 2 * HW:].min()) == -7.0


def test_renderer_wrapper_vs_reference_postprocessing_fixture(gpu_device):
    """render_predicted_more_v2_gof called exactly as visualize.py calls it ([1,1,4,4] matrices, [1,1,3] centre, [1,3] bg)
    on the fixture's Gaussians; compared with what the REFERENCE wrapper produced around the oracle's raster."""
    g = np.load(os.path.join(GOLD, "renderer_post.npz"))
    cfg = cameras.default_cfg(64)
    pc = {k[2:]: torch.from_numpy(g[k]).unsqueeze(0).repeat(2, *([1] * g[k].ndim)).to(gpu_device) for k in g.files if k.startswith("g_")}
    wv, fp, cc = (torch.from_numpy(g[k]).to(gpu_device) for k in ("wv", "fp", "cc"))
    out = f3d.render_predicted_more_v2_gof(pc, 1, wv, fp, cc, torch.zeros(1, 3, device=gpu_device), cfg)
    assert set(out) == {"render", "rendered_normal", "rendered_depth", "depth_normal", "rendered_alpha",
                        "distortion_map", "viewspace_points", "visibility_filter", "radii"}
    shapes = {"render": (3, 64, 64), "rendered_normal": (3, 64, 64), "rendered_depth": (1, 64, 64),
              "depth_normal": (3, 64, 64), "rendered_alpha": (1, 64, 64), "distortion_map": (1, 64, 64),
              "viewspace_points": (3000, 3), "visibility_filter": (3000,), "radii": (3000,)}
    for k, s in shapes.items():
        assert tuple(out[k].shape) == s, k
    assert out["radii"].dtype == torch.int32 and out["visibility_filter"].dtype == torch.bool
    assert np.array_equal(out["radii"].cpu().numpy(), g["out_radii"])
    assert out["render"].requires_grad          # means2D is a grad sink, exactly as in the reference (gr.py:932-936)
    raster = torch.cat([out["render"], torch.zeros(3, 64, 64, device=gpu_device), out["rendered_depth"],
                        out["rendered_alpha"], out["distortion_map"]]).detach().cpu().numpy()
    ref = g["raster"].copy(); ref[3:6] = 0
    assert_render_parity(raster, ref, "wrapper")
    # post-processing: compare on pixels whose rendered depth agrees (a flipped median-depth pixel moves its 4 neighbours)
    assert (np.abs(out["rendered_normal"].detach().cpu().numpy() - g["out_rendered_normal"]) <= 1e-4).mean() >= 0.999
    assert (np.abs(out["depth_normal"].detach().cpu().numpy() - g["out_depth_normal"]) <= 2e-3).mean() >= 0.995
    dn = out["depth_normal"].detach().cpu().numpy()
    assert not dn[:, 0].any() and not dn[:, -1].any() and not dn[:, :, 0].any() and not dn[:, :, -1].any()


def test_epilogue_kernel_on_exact_raster(gpu_device):
    """Same raster in, so only the post-processing arithmetic differs: tight tolerance."""
    from f3dgaus_amd.gaussian_renderer import _epilogue
    g = np.load(os.path.join(GOLD, "renderer_post.npz"))
    raster = torch.from_numpy(g["raster"]).unsqueeze(0).to(gpu_device)
    fov = 13.164 * np.pi / 180
    nw, dn = _epilogue(raster, torch.from_numpy(g["wv"]).reshape(1, 4, 4).to(gpu_device), 64, 64, fov, fov)
    assert np.abs(nw[0].cpu().numpy() - g["out_rendered_normal"]).max() < 2e-6
    d = np.abs(dn[0].cpu().numpy() - g["out_depth_normal"])
    assert (d <= 1e-3).mean() >= 0.999, (d <= 1e-3).mean()        # cross products of nearly equal points amplify 1-ulp ray differences
    torch_dn = f3d.depth_to_normal(torch.from_numpy(g["wv"]).reshape(4, 4).to(gpu_device), 64, 64, fov, fov, raster[0, 6:7])
    assert torch_dn.shape == (64, 64, 3) and torch.equal(torch_dn.permute(2, 0, 1), dn[0])


def test_mark_visible_and_v3_list_of_dicts(gpu_device):
    scene = make_scene(P=3000, res=(64, 64), s0=0.05, view="oblique", behind_fraction=0.1)
    o = run_oracle(scene)
    S = f3d.GaussianRasterizationSettings_GOF(64, 64, scene["tanfovx"], scene["tanfovy"], 0.0, torch.zeros(0), scene["bg"].to(gpu_device),
                                              1.0, scene["viewmatrix"][0].to(gpu_device), scene["projmatrix"][0].to(gpu_device), 1,
                                              scene["campos"][0].to(gpu_device), False, False)
    vis = f3d.GaussianRasterizer_GOF(S).markVisible(scene["means3D"].to(gpu_device))
    pv = scene["means3D"].numpy() @ scene["viewmatrix"][0].numpy()[:3, 2] + scene["viewmatrix"][0].numpy()[3, 2]
    assert vis.dtype == torch.bool and np.array_equal(vis.cpu().numpy(), pv > 0.2)
    cfg = cameras.default_cfg(64)
    pcs = [{"xyz": scene["means3D"].to(gpu_device), "opacity": scene["opacities"].to(gpu_device),
            "scaling": scene["scales"].to(gpu_device), "rotation": scene["rotations"].to(gpu_device),
            "features_dc": scene["shs"][:, :1].to(gpu_device), "features_rest": scene["shs"][:, 1:].to(gpu_device)}]
    out = f3d.render_predicted_more_v3_gof(pcs, 0, scene["viewmatrix"][:1].unsqueeze(0).to(gpu_device),
                                           scene["projmatrix"][:1].unsqueeze(0).to(gpu_device),
                                           scene["campos"][:1].unsqueeze(0).to(gpu_device), torch.zeros(1, 3, device=gpu_device), cfg)
    assert_render_parity(torch.cat([out["render"], torch.zeros(3, 64, 64, device=gpu_device), out["rendered_depth"],
                                    out["rendered_alpha"], out["distortion_map"]]).detach().cpu().numpy(),
                         np.concatenate([o["out_color"][:3], np.zeros((3, 64, 64), np.float32), o["out_color"][6:]]), "v3")


def test_cycle_loop_batched_equals_reference_shaped_loop(gpu_device):
    """The batched cycle aggregation (one launch sequence per image, in-place merge) must equal the reference-shaped
    loop (visualize.py:283-340) run with the same operators; small resolution here, B = 8 @256x256 in
    test_baseline_configs_gpu.py."""
    from test_baseline_configs_gpu import cycle_loop_check
    B, res = 2, 64
    merged, cfg, rig = cycle_loop_check(gpu_device, B, res)
    orbit = f3d.cycle.render_orbit(merged, cfg, rig=rig, num_views=6, views_per_call=4)
    assert orbit["render"].shape == (B, 6, 3, res, res) and torch.isfinite(orbit["render"]).all()
    assert orbit["rendered_alpha"].mean() > 0.05      # random weights: opacity bias -3 keeps splats faint


def test_group_norm_silu_kernel_matches_torch(gpu_device):
    """f3dg_group_norm_silu_forward vs torch.nn.functional.group_norm (+ silu) in float32 on the shapes the backbone uses."""
    import torch.nn.functional as F
    from f3dgaus_amd.gaussian_predictor import GroupNorm
    torch.manual_seed(0)
    for (N, Cc, H, W) in ((2, 128, 64, 64), (3, 256, 16, 16), (1, 64, 256, 256), (2, 36, 10, 6)):
        gn = GroupNorm(Cc, eps=1e-6).to(gpu_device)
        with torch.no_grad():
            gn.weight.uniform_(0.5, 1.5); gn.bias.uniform_(-0.5, 0.5)
            x = (torch.randn(N, Cc, H, W, device=gpu_device) * 3 + 1.5)
            for silu in (False, True):
                y = gn(x, silu=silu)
                ref = F.group_norm(x.double(), gn.num_groups, gn.weight.double(), gn.bias.double(), gn.eps)
                ref = F.silu(ref) if silu else ref
                t = F.group_norm(x, gn.num_groups, gn.weight, gn.bias, gn.eps)
                t = F.silu(t) if silu else t
                err, err_t = (y.double() - ref).abs().max().item(), (t.double() - ref).abs().max().item()
                assert err <= max(2 * err_t, 2e-6), (N, Cc, H, W, silu, err, err_t)


def test_pack_frames_matches_reference_formula(gpu_device):
    """(255 * np.clip(x, 0, 1)).astype(np.uint8) of visualize.py:416 on the first three planes, HWC order; bit-exact."""
    from f3dgaus_amd.gaussian_renderer import pack_frames
    torch.manual_seed(3)
    for (n, C, H, W) in ((5, 9, 64, 64), (2, 3, 17, 23), (1, 9, 256, 256)):
        x = (torch.rand(n, C, H, W) * 1.6 - 0.3)
        x[0, 0, 0, :4] = torch.tensor([0.0, 1.0, 254.9999 / 255.0, 0.5])
        got = pack_frames(x.to(gpu_device)).cpu().numpy()
        ref = (255 * np.clip(x[:, :3].permute(0, 2, 3, 1).numpy(), 0, 1)).astype(np.uint8)
        assert got.shape == ref.shape and np.array_equal(got, ref), (n, C, H, W)


def test_pack_frames_into_pinned_host_memory(gpu_device):
    """f3dg_pack_frames_host: the same bytes written by the kernel straight into a pinned host tensor -- sizes whose byte stream is
    not a multiple of 16 and whose 16-byte chunks straddle frames, few and many workgroups; pageable or misaligned memory is refused."""
    import ctypes as C
    from f3dgaus_amd import _lib
    from f3dgaus_amd.gaussian_renderer import pack_frames
    torch.manual_seed(4)
    for (n, Cc, H, W) in ((5, 9, 64, 64), (3, 3, 17, 23), (1, 9, 256, 256), (7, 4, 5, 3), (120, 9, 32, 32)):
        x = (torch.rand(n, Cc, H, W) * 1.6 - 0.3)
        ref = (255 * np.clip(x[:, :3].permute(0, 2, 3, 1).numpy(), 0, 1)).astype(np.uint8)
        xd = x.to(gpu_device)
        for wg in (0, 1, 1000):
            host = torch.full((n, H, W, 3), 77, dtype=torch.uint8).pin_memory()
            got = pack_frames(xd, out=host, max_workgroups=wg)
            torch.cuda.synchronize()
            assert got is host and np.array_equal(host.numpy(), ref), (n, Cc, H, W, wg)
    with pytest.raises(RuntimeError):
        pack_frames(xd, out=torch.empty((120, 32, 32, 3), dtype=torch.uint8))             # pageable
    L = _lib.lib()
    pageable = torch.empty(120 * 32 * 32 * 3 + 64, dtype=torch.uint8)
    rc = L.f3dg_pack_frames_host(None, 120, 32, 32, 9, C.c_void_p(xd.data_ptr()), C.c_void_p(pageable.data_ptr()), 0)
    assert rc == _lib.ERR_BAD_ARG
    pinned = torch.empty(120 * 32 * 32 * 3 + 64, dtype=torch.uint8).pin_memory()
    rc = L.f3dg_pack_frames_host(None, 120, 32, 32, 9, C.c_void_p(xd.data_ptr()), C.c_void_p(pinned.data_ptr() + 4), 0)
    assert rc == _lib.ERR_BAD_ARG


def test_cycle_aggregation_matches_the_reference_loop_fixture(gpu_device):
    """tests/golden/cycle_loop.npz was produced by the reference's OWN loop (visualize.py:224-340 executed from where it lies)
    around the reference's own predictor and renderer wrapper, with the C oracle as the rasterizer and formula-defined weights
    (tests/tools/gen_cycle_golden.py). The batched HIP loop with the same weights must reproduce the 8 intermediate renders and
    the merged 9 x 1024 Gaussians of every checked image."""
    import os
    from helpers_weights import formula_state_dict
    gold = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cycle_loop.npz"))
    res, V = 32, 8
    cfg = cameras.default_cfg(res)
    torch.manual_seed(0)
    model = f3d.Unet_GS_gtunet(cfg, renderer=f3d.render_predicted_more_v2_gof).eval()
    sd = model.state_dict()
    keep = {k: v for k, v in sd.items() if k.split(".")[-1] in ("ray_dirs", "sh_to_v_transform", "v_to_sh_transform") or k.endswith("resample_filter")}
    model.load_state_dict(formula_state_dict({k: tuple(v.shape) for k, v in sd.items()}, keep=keep))
    model = model.to(gpu_device)
    images, depth = torch.from_numpy(gold["images"]).to(gpu_device), torch.from_numpy(gold["depth"]).to(gpu_device)
    merged, renders = f3d.cycle.cycle_aggregate(model, images, depth, cfg, rig=cameras.OrbitRig(cfg), num_views=V, return_renders=True)
    sel = [int(i) for i in gold["sel"]]
    rel = lambda a, b: float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))
    for name, ours in (("rendered_8", renders["rgb"]), ("alpha_8", renders["alpha"]), ("depth_8", renders["depth"])):
        e = rel(ours[sel].cpu().numpy(), gold[name])
        assert e <= 2e-4, (name, e)
    for k in ("xyz", "opacity", "scaling", "rotation", "features_dc", "features_rest", "unet_depth"):
        ref = gold["m_" + k]
        assert merged[k][sel].shape == ref.shape, k
        e = rel(merged[k][sel].cpu().numpy(), ref)
        assert e <= 5e-4, (k, e)


def test_image_batched_render_equals_per_image_calls(gpu_device):
    """f3dg_forward_sets (B Gaussian sets x V cameras in one launch sequence) against B separate calls; f3dg_cycle_inputs against
    clamp / cat in torch; render_orbit with images_per_call > 1 against the per-image loop. All bit for bit."""
    from f3dgaus_amd.gaussian_renderer import cycle_inputs, render_views
    from f3dgaus_amd import synthetic
    B, V, res = 3, 5, 64
    cfg = cameras.default_cfg(res)
    gs = [synthetic.make_gaussians(3000, s0=0.05, seed=40 + b, device=gpu_device) for b in range(B)]
    pc = {k: torch.stack([g[k] for g in gs]) for k in gs[0]}
    ob = cameras.OrbitRig(cfg).orbit(V)
    wv, fp, cc = (t.to(gpu_device) for t in (ob.world_view_transforms, ob.full_proj_transforms, ob.camera_centers))
    bg = torch.tensor([0.2, 0.1, 0.4], device=gpu_device)
    allb = render_views(pc, None, wv, fp, cc, bg, cfg)
    assert allb["raster"].shape == (B * V, 9, res, res) and allb["radii"].shape == (B * V, 3000)
    for b in range(B):
        one = render_views(pc, b, wv, fp, cc, bg, cfg)
        for k in ("raster", "rendered_normal", "depth_normal", "radii"):
            assert torch.equal(one[k], allb[k][b * V:(b + 1) * V]), (b, k)
    xin, dep = cycle_inputs(allb["raster"], B, V)
    r = allb["raster"].reshape(B, V, 9, res, res)
    assert torch.equal(xin, torch.cat([r[:, :, :3].clamp(0, 1), r[:, :, 7:8]], 2).transpose(0, 1))
    assert torch.equal(dep, r[:, :, 6:7].transpose(0, 1))
    a = f3d.cycle.render_orbit(pc, cfg, num_views=6, views_per_call=4)
    b = f3d.cycle.render_orbit(pc, cfg, num_views=6, views_per_call=4, images_per_call=2)
    for k in a:
        assert torch.equal(a[k], b[k]), k


def test_backbone_bf16_option(gpu_device):
    """the bf16 option of the backbone (bfloat16 autocast for the convolutions, bf16 activations through the fused
    GroupNorm+SiLU kernel, float32 statistics / attention / splat head). Reports and bounds its error against the reference-generated
    fixture songunet.npz; the float32 default must stay at float32 accuracy."""
    import os
    import torch.nn.functional as F
    from f3dgaus_amd.gaussian_predictor import GaussianSplatPredictor_gtunet, GroupNorm
    from helpers_weights import formula_state_dict
    # the fused kernel on bf16 tensors against float64 torch
    torch.manual_seed(0)
    for (N, Cc, H, W) in ((2, 128, 64, 64), (1, 256, 16, 16), (2, 36, 10, 6)):
        gn = GroupNorm(Cc, eps=1e-6).to(gpu_device)
        with torch.no_grad():
            gn.weight.uniform_(0.5, 1.5); gn.bias.uniform_(-0.5, 0.5)
            x = (torch.randn(N, Cc, H, W, device=gpu_device) * 3 + 1.5).bfloat16()
            for silu in (False, True):
                y = gn(x, silu=silu)
                assert y.dtype == torch.bfloat16
                ref = F.group_norm(x.double(), gn.num_groups, gn.weight.double(), gn.bias.double(), gn.eps)
                ref = F.silu(ref) if silu else ref
                err = (y.double() - ref).abs().max().item()
                assert err <= 2.0 ** -8 * max(1.0, ref.abs().max().item()), (N, Cc, H, W, silu, err)      # one bf16 rounding of the result
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "songunet.npz"))
    pred = GaussianSplatPredictor_gtunet(cameras.default_cfg()).eval()
    sd = pred.state_dict()
    keep = {k: v for k, v in sd.items() if k in ("ray_dirs", "sh_to_v_transform", "v_to_sh_transform") or k.endswith("resample_filter")}
    pred.load_state_dict(formula_state_dict({k: tuple(v.shape) for k, v in sd.items()}, keep=keep))
    pred = pred.to(gpu_device)
    x = torch.from_numpy(g["x"]).to(gpu_device)
    with torch.no_grad():
        y32 = pred.network_with_offset(x, N_views_xa=1)
        with torch.autocast("cuda", dtype=torch.bfloat16):
            y16 = pred.network_with_offset(x, N_views_xa=1).float()
    ref = torch.from_numpy(g["y"]).to(gpu_device)
    e32 = ((y32 - ref).abs().max() / ref.abs().max()).item()
    e16 = ((y16 - ref).abs().max() / ref.abs().max()).item()
    rms16 = ((y16 - ref).pow(2).mean().sqrt() / ref.pow(2).mean().sqrt()).item()
    print(f"SongUNet vs reference fixture: fp32 max rel {e32:.2e}; bf16 option max rel {e16:.2e}, rms rel {rms16:.2e}")
    # measured on MI355X: fp32 2.2e-5; bf16 1.2e-1 max / 6.2e-2 rms on these formula-defined (quasi-random, ~100-layer) weights --
    # the option trades that for a 3x faster backbone and is opt-in (cfg['model']['backbone_dtype'] = 'bf16')
    assert e32 < 5e-5 and e16 < 0.25 and rms16 < 0.12, (e32, e16, rms16)
    # the option is wired through the predictor: same call, bf16 backbone, float32 Gaussians
    cfg = cameras.default_cfg(32)
    cfg['model']['backbone_dtype'] = 'bf16'
    p16 = GaussianSplatPredictor_gtunet(cfg).to(gpu_device).eval()
    assert p16.backbone_dtype == "bf16"
    xin = torch.rand(2, 1, 4, 32, 32, device=gpu_device)
    rig = cameras.OrbitRig(cfg).canonical
    with torch.no_grad():
        out = p16(xin, rig.view_to_world_transforms.expand(2, 1, 4, 4).to(gpu_device), rig.source_cv2wT_quat.expand(2, 1, 4).to(gpu_device),
                  unet_depth=torch.full((2, 1, 32, 32), 7.0, device=gpu_device))
    assert out["xyz"].dtype == torch.float32 and out["xyz"].shape == (2, 1024, 3) and bool(torch.isfinite(out["scaling"]).all())


def test_group_norm_silu_channels_last_kernel(gpu_device):
    """f3dg_group_norm_silu_forward, nhwc = 1: the channels-last GroupNorm (+ SiLU) of the backbone's "nhwc" layout option against float64
    torch, on the channel counts of the backbone (128 / 256 / 384 / 512: 16..128 packets per pixel, incl. the two that do not divide
    the workgroup) and on pixel counts that are not a multiple of a workgroup's run; the output stays channels-last."""
    import torch.nn.functional as F
    from f3dgaus_amd.gaussian_predictor import GroupNorm
    torch.manual_seed(1)
    for (N, Cc, H, W) in ((2, 128, 64, 64), (1, 256, 16, 16), (2, 384, 20, 13), (1, 512, 32, 32), (3, 128, 7, 5), (1, 1024, 9, 9)):
        gn = GroupNorm(Cc, eps=1e-6).to(gpu_device)
        with torch.no_grad():
            gn.weight.uniform_(0.5, 1.5); gn.bias.uniform_(-0.5, 0.5)
            x32 = (torch.randn(N, Cc, H, W, device=gpu_device) * 3 + 1.5).contiguous(memory_format=torch.channels_last)
            for x in (x32, x32.bfloat16()):
                for silu in (False, True):
                    y = gn(x, silu=silu)
                    assert y.dtype == x.dtype and y.is_contiguous(memory_format=torch.channels_last)
                    ref = F.group_norm(x.double(), gn.num_groups, gn.weight.double(), gn.bias.double(), gn.eps)
                    ref = F.silu(ref) if silu else ref
                    err = (y.double() - ref).abs().max().item()
                    if x.dtype == torch.float32:
                        t = F.group_norm(x32.contiguous(), gn.num_groups, gn.weight, gn.bias, gn.eps)
                        t = F.silu(t) if silu else t
                        assert err <= max(2 * (t.double() - ref).abs().max().item(), 2e-6), (N, Cc, H, W, silu, err)
                        # and the NCHW kernel gives the same numbers up to the last bit or two
                        assert (gn(x32.contiguous(), silu=silu) - y).abs().max().item() <= 4e-6 * max(1.0, ref.abs().max().item())
                    else:
                        assert err <= 2.0 ** -8 * max(1.0, ref.abs().max().item()), (N, Cc, H, W, silu, err)


def test_group_norm_channels_last_refuses_an_undersized_scratch(gpu_device):
    """The `moments` scratch of the channels-last GroupNorm grew in round 5 (a partial pair per workgroup): every entry point takes the
    size of the buffer it is handed and answers F3DG_ERR_WORKSPACE instead of writing past the end of one sized by an older header."""
    import ctypes as C
    from f3dgaus_amd import _lib
    L = _lib.lib()
    N, Cc, H, W, groups = 2, 128, 64, 64, 32
    x = torch.randn(N, H * W, Cc, device=gpu_device)
    y = torch.empty_like(x)
    w = torch.ones(Cc, device=gpu_device); b = torch.zeros(Cc, device=gpu_device)
    need = L.f3dg_group_norm_nhwc_scratch_bytes(N, H * W, groups)
    old = 16 * N * groups * 8                                   # the round-4 header's size: too small from 64 x 64 on
    assert need > old
    mom = torch.zeros(need // 8 + 1, dtype=torch.float64, device=gpu_device)
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    args = (s, 0, 1, N, Cc, H * W, groups, _lib.ptr(x), None, _lib.ptr(w), _lib.ptr(b), 1e-6, 1, _lib.ptr(y), None, _lib.ptr(mom))
    assert L.f3dg_group_norm_silu_forward(*args, old) == _lib.ERR_WORKSPACE
    assert L.f3dg_group_norm_silu_forward(*args, need - 1) == _lib.ERR_WORKSPACE
    assert L.f3dg_group_norm_silu_forward(*args, need) == 0
    torch.cuda.synchronize()
    assert torch.isfinite(y).all()



@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_conv_bias_folding_and_residual_join(dtype, gpu_device):
    """GroupNorm(pre_bias=) and residual_join() -- the kernels that take over the convolutions' bias passes and the residual add + scale
    of a block (f3dg_group_norm_silu_forward, f3dg_residual_join_forward) -- against the unfused PyTorch expressions, in both layouts; and a whole
    residual block through the fused path against the same block through the unfused lines."""
    from f3dgaus_amd import gaussian_predictor as gp
    dt = torch.float32 if dtype == "fp32" else torch.bfloat16
    tol = 2e-6 if dtype == "fp32" else 2.0 ** -7
    torch.manual_seed(5)
    for (N, Cc, H, W) in ((2, 128, 32, 32), (1, 384, 12, 10), (2, 36, 10, 6)):
        gn = gp.GroupNorm(Cc, eps=1e-6).to(gpu_device)
        with torch.no_grad():
            gn.weight.uniform_(0.5, 1.5); gn.bias.uniform_(-0.5, 0.5)
            pb = torch.randn(Cc, device=gpu_device)
            x = (torch.randn(N, Cc, H, W, device=gpu_device) * 2 + 0.5).to(dt)
            b = torch.randn(N, Cc, H, W, device=gpu_device).to(dt)
            pb2 = torch.randn(Cc, device=gpu_device)
            for layout in ("nchw", "nhwc"):
                if layout == "nhwc" and Cc % 8:
                    continue
                conv = (lambda t: t.contiguous(memory_format=torch.channels_last)) if layout == "nhwc" else (lambda t: t.contiguous())
                xl, bl = conv(x), conv(b)
                y = gn(xl, silu=True, pre_bias=pb)
                ref = torch.nn.functional.silu(torch.nn.functional.group_norm(x.double() + pb.double().reshape(1, -1, 1, 1), gn.num_groups,
                                                                              gn.weight.double(), gn.bias.double(), gn.eps))
                assert (y.double() - ref).abs().max().item() <= tol * max(1.0, ref.abs().max().item()) * (4 if dtype == "fp32" else 1), (N, Cc, layout)
                for ba, bb in ((pb, pb2), (pb, None), (None, None)):
                    j = gp.residual_join(xl.clone(), ba, bl, bb, 0.70710678)
                    rj = ((x.float() + (0 if ba is None else ba.reshape(1, -1, 1, 1))) + (b.float() + (0 if bb is None else bb.reshape(1, -1, 1, 1)))) * 0.70710678
                    assert j.dtype == dt and (j.float() - rj).abs().max().item() <= tol * max(1.0, rj.abs().max().item()), (N, Cc, layout)
    # a whole block, with a skip convolution (channel change) and without
    for cin, cout in ((128, 256), (256, 256)):
        blk = gp.UNetBlock(cin, cout).to(gpu_device).eval()
        with torch.no_grad():
            for m in blk.modules():
                if isinstance(m, gp.Conv2d) and m.bias is not None:
                    m.bias.uniform_(-0.3, 0.3)
            blk.conv1.weight.mul_(3e4)          # (init_weight 1e-5 would hide conv1 behind the skip path)
            x = torch.randn(2, cin, 32, 32, device=gpu_device)
            with torch.autocast("cuda", dtype=torch.bfloat16, enabled=dtype == "bf16"):
                fused = blk(x)
                blk.train()                      # the unfused lines (dropout p = 0.1 is the only difference: switch it off)
                blk.dropout = 0.0
                plain = blk(x)
                blk.eval()
            err = (fused.float() - plain.float()).abs().max().item() / plain.float().abs().max().item()
            assert err <= (2e-6 if dtype == "fp32" else 3e-2), (cin, cout, err)


def test_backbone_fp16_option_and_deterministic_groupnorm(gpu_device):
    """Round 5: (a) the fp16 option of the backbone (float16 autocast, float16 activations through the fused GroupNorm+SiLU and residual
    join kernels): the kernels against float64 torch at one float16 rounding, the reference-generated fixture songunet.npz at a quarter of
    the bf16 option's bars; (b) the channels-last GroupNorm's statistics are summed in a fixed order (one partial pair per
    workgroup + a second-stage kernel, no atomics): two runs are bit-identical in every activation type."""
    import os
    import torch.nn.functional as F
    from f3dgaus_amd.gaussian_predictor import GaussianSplatPredictor_gtunet, GroupNorm, residual_join
    from helpers_weights import formula_state_dict
    torch.manual_seed(0)
    for dt, ulp in ((torch.float16, 2.0 ** -11), (torch.bfloat16, 2.0 ** -8), (torch.float32, 1e-6)):
        for (N, Cc, H, W), nhwc in (((2, 128, 64, 64), False), ((2, 128, 64, 64), True), ((3, 256, 32, 32), True), ((2, 36, 10, 6), False)):
            gn = GroupNorm(Cc, eps=1e-6).to(gpu_device)
            with torch.no_grad():
                gn.weight.uniform_(0.5, 1.5); gn.bias.uniform_(-0.5, 0.5)
                x = (torch.randn(N, Cc, H, W, device=gpu_device) * 3 + 1.5).to(dt)
                pb = torch.randn(Cc, device=gpu_device) * 0.3
                if nhwc:
                    x = x.contiguous(memory_format=torch.channels_last)
                for silu in (False, True):
                    y = gn(x, silu=silu, pre_bias=pb)
                    y2 = gn(x, silu=silu, pre_bias=pb)
                    assert y.dtype == dt and torch.equal(y, y2), (dt, nhwc, silu)            # (b): run-to-run bit-identical
                    ref = F.group_norm(x.double() + pb.double().reshape(1, -1, 1, 1), gn.num_groups, gn.weight.double(), gn.bias.double(), gn.eps)
                    ref = F.silu(ref) if silu else ref
                    err = (y.double() - ref).abs().max().item()
                    assert err <= 2 * ulp * max(1.0, ref.abs().max().item()), (dt, N, Cc, H, W, nhwc, silu, err)
        a = torch.randn(2, 64, 16, 16, device=gpu_device).to(dt)
        b = torch.randn(2, 64, 16, 16, device=gpu_device).to(dt)
        ba, bb = torch.randn(64, device=gpu_device), torch.randn(64, device=gpu_device)
        want = ((a.double() + ba.double().reshape(1, -1, 1, 1)) + (b.double() + bb.double().reshape(1, -1, 1, 1))) * 0.7071067811865476
        with torch.no_grad():
            got = residual_join(a.clone(), ba, b, bb, 0.7071067811865476)
        assert got.dtype == dt and (got.double() - want).abs().max().item() <= 2 * ulp * want.abs().max().item()
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "songunet.npz"))
    pred = GaussianSplatPredictor_gtunet(cameras.default_cfg()).eval()
    sd = pred.state_dict()
    keep = {k: v for k, v in sd.items() if k in ("ray_dirs", "sh_to_v_transform", "v_to_sh_transform") or k.endswith("resample_filter")}
    pred.load_state_dict(formula_state_dict({k: tuple(v.shape) for k, v in sd.items()}, keep=keep))
    pred = pred.to(gpu_device)
    x = torch.from_numpy(g["x"]).to(gpu_device)
    ref = torch.from_numpy(g["y"]).to(gpu_device)
    errs = {}
    with torch.no_grad():
        for name, xin in (("nchw", x), ("nhwc", x.contiguous(memory_format=torch.channels_last))):
            with torch.autocast("cuda", dtype=torch.float16):
                y16 = pred.network_with_offset(xin, N_views_xa=1).float()
            assert bool(torch.isfinite(y16).all()), name
            errs[name] = (((y16 - ref).abs().max() / ref.abs().max()).item(), ((y16 - ref).pow(2).mean().sqrt() / ref.pow(2).mean().sqrt()).item())
    print("SongUNet fp16 option vs reference fixture (max rel, rms rel):", {k: ("%.2e" % v[0], "%.2e" % v[1]) for k, v in errs.items()})
    # measured on MI355X: NCHW 3.9e-2 max / 1.6e-2 rms, channels-last 1.1e-2 / 7.2e-3 (bf16: 8.4e-2 / 4.1e-2 -- three more mantissa bits buy
    # 2.5-5x on these formula-defined ~100-layer weights, not 8x; profiles/r05_final/fp16_frames.md). The bf16 option's bars are 0.25 / 0.12
    for name, (emax, erms) in errs.items():
        assert emax < 0.0625 and erms < 0.03, (name, emax, erms)
    # wired through the predictor, with chunked passes: 5 images as chunks of 2 + 2 + 1 against one pass of 5
    cfg = cameras.default_cfg(32)
    cfg['model']['backbone_dtype'] = 'fp16'
    cfg['model']['backbone_chunk'] = 2
    p16 = GaussianSplatPredictor_gtunet(cfg).to(gpu_device).eval()
    assert p16.backbone_dtype == "fp16" and p16.backbone_chunk == 2
    xin = torch.rand(5, 1, 4, 32, 32, device=gpu_device)
    rig = cameras.OrbitRig(cfg).canonical
    v2w = rig.view_to_world_transforms.expand(5, 1, 4, 4).to(gpu_device)
    quat = rig.source_cv2wT_quat.expand(5, 1, 4).to(gpu_device)
    depth = torch.rand(5, 1, 32, 32, device=gpu_device) * 2 + 6.667
    with torch.no_grad():
        chunked = p16(xin, v2w, quat, unet_depth=depth)
        p16.backbone_chunk = 0
        whole = p16(xin, v2w, quat, unet_depth=depth)
    for k in whole:
        assert chunked[k].dtype == torch.float32 and chunked[k].shape == whole[k].shape
        assert (chunked[k] - whole[k]).abs().max().item() <= 2e-2 * max(1.0, whole[k].abs().max().item()), k


def test_backbone_channels_last_option(gpu_device):
    """cfg['model']['backbone_layout'] = 'nhwc': the backbone with channels-last activations and filters (MIOpen's NHWC kernels, the
    channels-last GroupNorm+SiLU kernel, no layout conversion in between). float32: the reference-generated fixture songunet.npz at the
    float32 bar of the default layout; bf16: the bar of the bf16 option. The predictor's Gaussians equal the default layout's to float32
    accuracy."""
    import os
    from f3dgaus_amd.gaussian_predictor import GaussianSplatPredictor_gtunet
    from helpers_weights import formula_state_dict
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "songunet.npz"))
    pred = GaussianSplatPredictor_gtunet(cameras.default_cfg()).eval()
    sd = pred.state_dict()
    keep = {k: v for k, v in sd.items() if k in ("ray_dirs", "sh_to_v_transform", "v_to_sh_transform") or k.endswith("resample_filter")}
    pred.load_state_dict(formula_state_dict({k: tuple(v.shape) for k, v in sd.items()}, keep=keep))
    pred = pred.to(gpu_device)
    x = torch.from_numpy(g["x"]).to(gpu_device)
    ref = torch.from_numpy(g["y"]).to(gpu_device)
    with torch.no_grad():
        y_nchw = pred.network_with_offset(x, N_views_xa=1)
        pred.network_with_offset.to(memory_format=torch.channels_last)
        xcl = x.contiguous(memory_format=torch.channels_last)
        y32 = pred.network_with_offset(xcl, N_views_xa=1)
        with torch.autocast("cuda", dtype=torch.bfloat16):
            y16 = pred.network_with_offset(xcl, N_views_xa=1).float()
    e32 = ((y32 - ref).abs().max() / ref.abs().max()).item()
    e16 = ((y16 - ref).abs().max() / ref.abs().max()).item()
    rms16 = ((y16 - ref).pow(2).mean().sqrt() / ref.pow(2).mean().sqrt()).item()
    d = ((y32 - y_nchw).abs().max() / ref.abs().max()).item()
    print(f"SongUNet channels-last vs reference fixture: fp32 max rel {e32:.2e} (vs the NCHW pass {d:.2e}); bf16 max rel {e16:.2e}, rms rel {rms16:.2e}")
    assert e32 < 5e-5 and e16 < 0.25 and rms16 < 0.12, (e32, e16, rms16)
    # wired through the predictor
    cfg = cameras.default_cfg(32)
    cfg['model']['backbone_layout'] = 'nchw'
    p0 = GaussianSplatPredictor_gtunet(cfg).to(gpu_device).eval()
    cfg2 = cameras.default_cfg(32)
    p1 = GaussianSplatPredictor_gtunet(cfg2).to(gpu_device).eval()
    p1.load_state_dict(p0.state_dict())
    assert p1.backbone_layout == "auto" and p0.backbone_layout == "nchw"        # auto: channels-last for this pass of two images
    torch.manual_seed(3)
    xin = torch.rand(2, 1, 4, 32, 32, device=gpu_device)
    rig = cameras.OrbitRig(cfg).canonical
    args = (rig.view_to_world_transforms.expand(2, 1, 4, 4).to(gpu_device), rig.source_cv2wT_quat.expand(2, 1, 4).to(gpu_device))
    with torch.no_grad():
        a = p0(xin, *args, unet_depth=torch.full((2, 1, 32, 32), 7.0, device=gpu_device))
        b = p1(xin, *args, unet_depth=torch.full((2, 1, 32, 32), 7.0, device=gpu_device))
    for k in a:
        assert a[k].shape == b[k].shape and (a[k] - b[k]).abs().max().item() <= 1e-4 * max(1.0, a[k].abs().max().item()), k
    # the channels-last filter copies are kept per convolution until the parameter changes: an in-place update must be seen
    conv = p1.network_with_offset.encoder.enc["64x64_block0"].conv0
    assert conv.__dict__.get("_filter_cache") is not None and conv.__dict__["_filter_cache"][1].is_contiguous(memory_format=torch.channels_last)
    with torch.no_grad():
        delta = 0.05 * torch.randn_like(conv.weight)          # (not a scaling: the GroupNorm behind the convolution would undo it)
        for p in (p0, p1):
            p.network_with_offset.encoder.enc["64x64_block0"].conv0.weight.add_(delta)
        a2 = p0(xin, *args, unet_depth=torch.full((2, 1, 32, 32), 7.0, device=gpu_device))
        b2 = p1(xin, *args, unet_depth=torch.full((2, 1, 32, 32), 7.0, device=gpu_device))
    assert torch.equal(conv.__dict__["_filter_cache"][1], conv.weight) and conv.__dict__["_filter_cache"][0][0] == conv.weight._version
    for k in a2:
        assert (a2[k] - b2[k]).abs().max().item() <= 1e-4 * max(1.0, a2[k].abs().max().item()), k
    # one image per pass stays in torch's layout under "auto"
    with torch.no_grad():
        c1 = p1(xin[:1], args[0][:1], args[1][:1], unet_depth=torch.full((1, 1, 32, 32), 7.0, device=gpu_device))
    for k in c1:
        assert (c1[k] - b2[k][:1]).abs().max().item() <= 1e-4 * max(1.0, c1[k].abs().max().item()), k
    with pytest.raises(ValueError):
        bad = cameras.default_cfg(32)
        bad['model']['backbone_layout'] = 'nchw16'
        GaussianSplatPredictor_gtunet(bad)


def test_unet_gs_in_module_render_loop(gpu_device):
    """Unet_GS_gtunet(..., render=True) (reference src/unet_gs.py:77-93): the frames and median depths it returns are the per-image
    renderer calls, stacked."""
    res, B = 64, 3
    cfg = cameras.default_cfg(res)
    model = f3d.Unet_GS_gtunet(cfg, renderer=f3d.render_predicted_more_v2_gof).to(gpu_device).eval()
    rig = cameras.OrbitRig(cfg)
    cano, ob = rig.canonical, rig.orbit(B)
    torch.manual_seed(2)
    x = torch.rand(B, 1, 4, res, res, device=gpu_device)
    bg = torch.zeros(B, 3, device=gpu_device)
    wv, fp, cc = (t.to(gpu_device) for t in (ob.world_view_transforms, ob.full_proj_transforms, ob.camera_centers))
    with torch.no_grad():
        frames, depths, g = model(x, bg, cano.view_to_world_transforms.expand(B, 1, 4, 4).to(gpu_device),
                                  cano.source_cv2wT_quat.expand(B, 1, 4).to(gpu_device), render=True, world_view_transforms=wv,
                                  full_proj_transforms=fp, camera_centers=cc, config=cfg, image_size=res,
                                  unet_depth=torch.full((B, 1, res, res), 7.0, device=gpu_device))
        assert frames.shape == (B, 3, res, res) and depths.shape == (B, 1, res, res) and g["xyz"].shape == (B, res * res, 3)
        for b in range(B):
            od = f3d.render_predicted_more_v2_gof(g, b, wv[b:b + 1], fp[b:b + 1], cc[b:b + 1], bg[b:b + 1], cfg)
            assert torch.equal(od["render"].reshape(3, res, res), frames[b]) and torch.equal(od["rendered_depth"].reshape(1, res, res), depths[b])
        assert float(frames.max()) > 0 and bool(torch.isfinite(frames).all())


def test_renderer_derived_maps_carry_gradients(gpu_device):
    """rendered_normal / depth_normal are differentiable in the reference (gr.py:1043-1053). With gradients enabled
    the wrapper takes the torch formulation (same values as the fused kernel) and a loss on them reaches the Gaussians."""
    scene = make_scene(P=1500, res=(64, 64), s0=0.08, view="oblique")
    cfg = cameras.default_cfg(64)
    dev = lambda t: t.to(gpu_device)
    pc = {"xyz": dev(scene["means3D"])[None].clone().requires_grad_(True), "opacity": dev(scene["opacities"])[None],
          "scaling": dev(scene["scales"])[None].clone().requires_grad_(True), "rotation": dev(scene["rotations"])[None],
          "features_dc": dev(scene["shs"][:, :1])[None], "features_rest": dev(scene["shs"][:, 1:])[None]}
    args = (dev(scene["viewmatrix"][:1]), dev(scene["projmatrix"][:1]), dev(scene["campos"][:1]), torch.zeros(1, 3, device=gpu_device), cfg)
    out = f3d.render_predicted_more_v2_gof(pc, 0, *args)
    assert out["rendered_normal"].requires_grad and out["depth_normal"].requires_grad
    with torch.no_grad():
        ref = f3d.render_predicted_more_v2_gof({k: v.detach() for k, v in pc.items()}, 0, *args)      # fused kernel
    assert (out["rendered_normal"] - ref["rendered_normal"]).abs().max().item() < 1e-5
    d = (out["depth_normal"] - ref["depth_normal"]).abs()
    assert (d <= 1e-3).float().mean().item() >= 0.999
    (out["rendered_normal"].square().sum() + out["depth_normal"][:, 8:-8, 8:-8].sum()).backward()
    assert pc["xyz"].grad is not None and float(pc["xyz"].grad.abs().max()) > 0 and bool(torch.isfinite(pc["xyz"].grad).all())
    assert float(pc["scaling"].grad.abs().max()) > 0


def test_refilled_buffers_render_their_new_contents(gpu_device):
    """The wrapper concatenates features_dc / features_rest on every call, as the reference does (gr.py:1008). Round 3 cached the
    concatenation while both inputs "looked" unmodified; the package's own in-place writers (`splat_head(out=...)`, raw pointers)
    and `.data` writes do not touch the version counter that test used, so a refilled buffer rendered the previous colours."""
    cfg = cameras.default_cfg(64)
    g = synthetic.make_gaussians(2000, s0=0.05, seed=3, device=gpu_device)
    pc = {k: v.unsqueeze(0).clone() for k, v in g.items()}
    cams = synthetic.orbit_cameras(4, resolution=64, device=gpu_device)
    args = (cams["viewmatrix"][1:2], cams["projmatrix"][1:2], cams["campos"][1:2], torch.zeros(1, 3, device=gpu_device), cfg)
    with torch.no_grad():
        a = f3d.render_predicted_more_v2_gof(pc, 0, *args)["render"].clone()
        pc["features_dc"].data.mul_(-1.0)            # an in-place refill that leaves `_version` alone
        b = f3d.render_predicted_more_v2_gof(pc, 0, *args)["render"].clone()
        pc2 = {k: v.clone() for k, v in pc.items()}
        c = f3d.render_predicted_more_v2_gof(pc2, 0, *args)["render"]
    assert not torch.equal(a, b)
    assert torch.equal(b, c)
    with torch.inference_mode():                      # (reading `_version` of an inference tensor raised in round 3's cache)
        pci = {k: v.clone() for k, v in pc.items()}
        d = f3d.render_predicted_more_v2_gof(pci, 0, *args)["render"]
    assert torch.equal(d, c)


@pytest.mark.parametrize("mode", ["fast", "exact"])
def test_channel_mask_leaves_the_written_channels_bit_identical(mode, gpu_device):
    """`channels="rgb_depth_alpha"` (F3DG_FLAG_SKIP_NORMAL | F3DG_FLAG_SKIP_DISTORTION; used by cycle_aggregate / render_orbit, which
    consume what visualize.py:304-306, 400-402 consume): RGB, median depth and alpha equal the 9-channel render to the bit, the
    normal and distortion planes of the output buffer are not touched."""
    from f3dgaus_amd import _lib
    L = _lib.lib()
    g = synthetic.make_gaussians(20000, s0=0.02, seed=5, device=gpu_device)
    cams = synthetic.orbit_cameras(24, resolution=128, device=gpu_device)
    shs = torch.cat([g["features_dc"], g["features_rest"]], 1).contiguous()
    kw = dict(image_height=128, image_width=128, tanfovx=cams["tanfovx"], tanfovy=cams["tanfovy"], sh=shs, scales=g["scaling"],
              rotations=g["rotation"], sh_degree=1)
    args = (g["xyz"], g["opacity"], cams["viewmatrix"], cams["projmatrix"], cams["campos"], torch.zeros(3, device=gpu_device))
    assert L.f3dg_set_option(b"render_fast", 1 if mode == "fast" else 0) == 0
    try:
        full, _, _ = f3d.rasterize_views(*args, **kw)
        buf = torch.full_like(full, 123.0)
        lean, _, _ = f3d.rasterize_views(*args, out=buf, channels="rgb_depth_alpha", **kw)
    finally:
        L.f3dg_set_option(b"render_fast", 1)
    for c in (0, 1, 2, 6, 7):
        assert torch.equal(lean[:, c], full[:, c]), c
    assert bool((lean[:, 3:6] == 123.0).all()) and bool((lean[:, 8] == 123.0).all())
    assert float(full[:, 3:6].abs().max()) > 0
    with pytest.raises(RuntimeError):
        f3d.rasterize_views(*args, channels="rgb_depth_alpha", save_aux=True, **kw)
