"""Both segmented-scan kernels on the run-structure scenes of helpers.make_run_scene (census: test_run_census.py) against the oracle:
the dense compositing backward (render5_bwd_kernel, option bwd_dense 1) and the lock-step walk (bwd_dense 0) at the gates of
test_raster_backward_gpu.py, and the split-pixel forward (render5_fwd_kernel, render_scan_th 12 and 64) at the north_star's gate of
assert_render_parity and within 2e-5 of the default fast kernel."""
import numpy as np
import pytest
import torch

import f3dgaus_amd as f3d
from f3dgaus_amd import _lib
from f3dgaus_amd.diff_gof_rasterization.backward import rasterize_backward_raw
import helpers
from helpers import assert_render_parity, make_run_scene, run_oracle

pytestmark = pytest.mark.gpu

SCENES = ["wall", "confetti", "mixed", "odd"]


def _rel(a, b):
    m = np.abs(b).max()
    return 0.0 if m == 0 else float(np.abs(a.astype(np.float64) - b).max() / m)


def _args(scene, device):
    dev = lambda t: None if t is None else t.to(device)
    return (dev(scene["means3D"]), dev(scene["opacities"]), dev(scene["viewmatrix"]), dev(scene["projmatrix"]), dev(scene["campos"]), dev(scene["bg"]))


def _kw(scene, device):
    dev = lambda t: None if t is None else t.to(device)
    return dict(image_height=scene["H"], image_width=scene["W"], tanfovx=scene["tanfovx"], tanfovy=scene["tanfovy"], sh=None,
                colors_precomp=dev(scene["colors_precomp"]), scales=dev(scene["scales"]), rotations=dev(scene["rotations"]),
                sh_degree=scene["sh_degree"], scale_modifier=scene["scale_modifier"], kernel_size=scene["kernel_size"])


@pytest.mark.parametrize("name", SCENES)
def test_dense_backward_on_run_scenes(name, gpu_device):
    scene = make_run_scene(name)
    V, H, W = scene["viewmatrix"].shape[0], scene["H"], scene["W"]
    dev = lambda t: None if t is None else t.to(gpu_device)
    dpix = np.random.default_rng(7).standard_normal((V, 9, H, W)).astype(np.float32)
    L = _lib.lib()
    out, radii, ws = f3d.rasterize_views(*_args(scene, gpu_device), save_aux=True, **_kw(scene, gpu_device))
    grads = {}
    try:
        for dense in (1, 0):
            assert L.f3dg_set_option(b"bwd_dense", dense) == 0
            g = rasterize_backward_raw(ws, dev(scene["means3D"]), None, dev(scene["colors_precomp"]), dev(scene["scales"]), dev(scene["rotations"]),
                                       radii, torch.from_numpy(dpix).to(gpu_device), scene["sh_degree"], dev(scene["viewmatrix"]),
                                       dev(scene["projmatrix"]), dev(scene["campos"]), dev(scene["bg"]), scene["tanfovx"], scene["tanfovy"],
                                       scene["kernel_size"], scene["scale_modifier"])
            torch.cuda.synchronize()
            grads[dense] = {k: v.cpu().numpy() for k, v in g.items()}
    finally:
        L.f3dg_set_option(b"bwd_dense", 1)
    opac = 0.0
    for v in range(V):
        o = run_oracle(scene, view=v)
        go = o["oracle"].backward(dpix[v])
        opac = opac + go["dL_dopacity"].astype(np.float64)
        for dense, gh in grads.items():
            assert np.array_equal(radii.cpu().numpy()[v], o["radii"]), (name, v)
            assert _rel(gh["dL_dview2gaussian"][v], go["dL_dview2gaussian"]) <= 1e-5, (name, dense, v)
            assert _rel(gh["dL_dcolors"][v], go["dL_dcolor"]) <= 1e-5, (name, dense, v)
            assert _rel(gh["dL_dmeans2D"][v], go["dL_dmean2D"]) <= 2e-5, (name, dense, v)
    for dense, gh in grads.items():
        assert _rel(gh["dL_dopacity"], opac) <= 1e-5, (name, dense)
        for k in gh:
            assert np.isfinite(gh[k]).all(), (name, dense, k)


def _render(scene, device, scan, th=12):
    L = _lib.lib()
    assert L.f3dg_set_option(b"render_scan_th", th) == 0
    assert L.f3dg_set_option(b"render_lowocc", 0) == 0
    try:
        out, _, _ = f3d.rasterize_views(*_args(scene, device), save_aux=False, exact=False, small_path=False, scan=scan,
                                        out=torch.zeros((scene["viewmatrix"].shape[0], 9, scene["H"], scene["W"]), device=device),
                                        **_kw(scene, device))
        torch.cuda.synchronize()
        kernel = L.f3dg_debug_last_render_kernel()
    finally:
        L.f3dg_set_option(b"render_scan_th", 12)
        L.f3dg_set_option(b"render_lowocc", 1)
    return out.cpu().numpy(), kernel


@pytest.mark.parametrize("name", SCENES)
def test_scan_forward_on_run_scenes(name, gpu_device):
    scene = make_run_scene(name)
    helpers.RENDER_MODE = "fast"
    try:
        base, kb = _render(scene, gpu_device, scan=False)
        assert b"render5" not in kb
        oracle = [run_oracle(scene, view=v)["out_color"] for v in range(scene["viewmatrix"].shape[0])]
        for v, o in enumerate(oracle):
            assert_render_parity(base[v], o, "default fast %s view %d" % (name, v))
        for th in (12, 64):
            out, k = _render(scene, gpu_device, scan=True, th=th)
            assert b"render5_fwd_kernel" in k, k
            assert np.isfinite(out).all()
            for v, o in enumerate(oracle):
                assert_render_parity(out[v], o, "scan th=%d %s view %d" % (th, name, v), dist_big_rtol=2e-3)
            d = np.abs(out[:, [0, 1, 2, 7]] - base[:, [0, 1, 2, 7]])
            assert np.mean(d <= 2e-5) >= 0.9995, (name, th, float(d.max()), float(np.mean(d <= 2e-5)))
    finally:
        helpers.RENDER_MODE = None
