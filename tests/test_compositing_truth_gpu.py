"""Every compositing forward kernel against the float64 truth ON ITS OWN INPUTS (tests/compositing_truth.py; the conditions are held on the
CPU by tests/test_compositing_truth.py).

The call's own exports -- records, sorted list, tile ranges, built without tile culling -- are asserted bit-equal to the oracle's on the
visible Gaussians, so kernel and oracle are measured against ONE truth and the only error left on either side is the rounding of its blend:
K = |x - truth| / (2^-24 A), A = the sum of the magnitudes of the pixel's terms. Per scene, mode and group (rgb, normal, depth, alpha,
distortion; in SAVE_AUX calls also the four final_T planes the backward reads), over the pixels outside the near-tie margins, no floor:

  median, 99th percentile and maximum of K  <=  m x the oracle's for the same scene, group and statistic
      m = 4  reference arithmetic: the project's margin for a float32 kernel against the float32 reference
             (tests/test_epilogue_backward_gpu.py, tests/test_per_gaussian_backward_gpu.py)
      m = 8  fast and scan arithmetic: the same 4, times 2 for v_exp_f32 / v_rcp_f32 / v_rsq_f32 at up to 1 ulp where the oracle has
             division and sqrt at <= 0.5 ulp and expf below 1 ulp
  exact zeros where A = 0 (a pixel with no blended entry is the background to the bit)
  SAVE_AUX: the last contributor identical on every kept pixel, the median contributor on every pixel kept for depth
  helpers.assert_render_parity, as it is, on ALL pixels (it covers the excluded ones)

The image under test is the default, culled call (helpers.run_hip holds it to the unculled one bit for bit; a one- or two-view call takes
the small path there, whose compositing is the same small-launch kernels: render3l was deleted after round 6). The kernel of every mode
is asserted by name. Figures measured on an MI355X: DESIGN.md section 3c-bis -- every bar met, the largest kernel / oracle ratio of any
statistic 1.30 (exact), 2.33 (fast: depth through v_rcp_f32), 2.33 (scan); the factors 4 and 8 are kept as derived."""
import numpy as np
import pytest
import torch

import compositing_truth as CT
import f3dgaus_amd as f3d
from helpers import assert_render_parity, export_workspace, render_options, run_hip

pytestmark = pytest.mark.gpu


def _n_waves(sc):
    return sc["viewmatrix"].shape[0] * ((sc["W"] + 15) // 16) * ((sc["H"] + 15) // 16) * 4


def _assert_inputs_are_the_oracles(name, h):
    CT.assert_inputs_are_the_oracles(name, h, [CT.oracle(name, v) for v in range(CT.n_views(name))])


def _check(name, label, m, out, final_T, n_contrib, failures, dist_big_rtol=1e-3):
    for v in range(CT.n_views(name)):
        t, fig_o = CT.oracle_truth(name, v)
        lab = "%s %s view %d" % (name, label, v)
        assert np.isfinite(out[v]).all(), lab
        fig = CT.figures(t, out[v], None if final_T is None else final_T[v])
        CT.check_bars(lab, t, fig, fig_o, m, failures, out[v], None if final_T is None else final_T[v], None if n_contrib is None else n_contrib[v])
        assert_render_parity(out[v], CT.oracle(name, v)["out_color"], lab, dist_big_rtol=dist_big_rtol)


def _run_variants(name, device, mode, m, variants):
    """Each (options, kernel name) with and without SAVE_AUX through helpers.run_hip, held to the bars at factor m."""
    sc = CT.scene(name)
    failures = []
    for opts, kernel in variants:
        for aux in (False, True):
            with render_options(mode, **opts) as L:
                h = run_hip(sc, device, save_aux=aux)
                k = L.f3dg_debug_last_render_kernel()
            assert kernel in k and (b"SAVE_AUX=true" in k) == aux and (b"FAST=true" in k) == (mode == "fast"), k
            _assert_inputs_are_the_oracles(name, h)
            label = "%s%s %s" % (mode, " SAVE_AUX" if aux else "", kernel.decode())
            _check(name, label, m, h["out_color"], h["final_T"] if aux else None, h["n_contrib"] if aux else None, failures)
    assert not failures, failures


@pytest.mark.parametrize("name", list(CT.SCENES))
def test_exact_kernels_against_float64_on_their_own_inputs(name, gpu_device):
    """The plain transcription (render_fwd_kernel), the rank-packed kernel (render4) and the default of a launch this small (one view's worth
    of quadrants: render3q), m = 4."""
    assert _n_waves(CT.scene(name)) <= 1024
    _run_variants(name, gpu_device, "exact", 4.0, [(dict(reference_kernels=1), b"render_fwd_kernel"), (dict(render_lowocc=0), b"render4_fwd_kernel"),
                                                   (dict(), b"render3q_fwd_kernel")])


@pytest.mark.parametrize("name", list(CT.SCENES))
def test_fast_kernels_against_float64_on_their_own_inputs(name, gpu_device):
    """render3s (the general kernel: option render_lowocc 0) and the default of a small launch (render3p), SAVE_AUX calls in the fast
    arithmetic too (option render_fast 2), m = 8."""
    _run_variants(name, gpu_device, "fast", 8.0, [(dict(render_fast=2, render_lowocc=0), b"render3s_fwd_kernel"),
                                                  (dict(render_fast=2), b"render3p_fwd_kernel")])


def _scan_call(sc, device, tile_cull, small_path):
    """An inference call in the scan mode. small_path=None is the library's default call: a one- or two-view call then bins through the small
    path (csrc/f3dg_small.hip), which hands its per-tile lists to the same f3dg_launch_render with the call's scan flag; small_path=False keeps
    the general launch sequence, whose lists and ranges helpers.export_workspace reads."""
    dev = lambda t: None if t is None else t.to(device)
    out, radii, ws = f3d.rasterize_views(
        dev(sc["means3D"]), dev(sc["opacities"]), dev(sc["viewmatrix"]), dev(sc["projmatrix"]), dev(sc["campos"]), dev(sc["bg"]),
        image_height=sc["H"], image_width=sc["W"], tanfovx=sc["tanfovx"], tanfovy=sc["tanfovy"], sh=dev(sc["shs"]),
        colors_precomp=dev(sc["colors_precomp"]), scales=dev(sc["scales"]), rotations=dev(sc["rotations"]), sh_degree=sc["sh_degree"],
        scale_modifier=sc["scale_modifier"], kernel_size=sc["kernel_size"], save_aux=False, exact=False, small_path=small_path, scan=True,
        tile_cull=tile_cull)
    torch.cuda.synchronize()
    return out, radii, ws


@pytest.mark.parametrize("name", list(CT.SCENES))
def test_scan_kernels_against_float64_on_their_own_inputs(name, gpu_device):
    """The split-pixel schedule: render5 at the fused / dense thresholds 64, 12 and 4 (option render_lowocc 0), render5p (four lanes per pixel)
    on a launch of at most 2,048 quadrant waves; m = 8. Bit-identical to no other kernel, so nothing else in the suite ties these two to
    anything tighter than 1e-4. The mode has no auxiliary planes."""
    sc = CT.scene(name)
    assert _n_waves(sc) <= 2048
    failures = []
    for opts, kernel in ((dict(render_lowocc=0, render_scan_th=64), b"render5_fwd_kernel"), (dict(render_lowocc=0, render_scan_th=12), b"render5_fwd_kernel"),
                         (dict(render_lowocc=0, render_scan_th=4), b"render5_fwd_kernel"), (dict(render_lowocc=1), b"render5p_fwd_kernel")):
        with render_options("fast", **opts) as L:
            out, radii, ws = _scan_call(sc, gpu_device, tile_cull=False, small_path=False)   # the reference's lists: this call's inputs, exported
            assert kernel in L.f3dg_debug_last_render_kernel(), L.f3dg_debug_last_render_kernel()
            h = export_workspace(sc, gpu_device, out, radii, ws, save_aux=False)
            culled, _, ws_c = _scan_call(sc, gpu_device, tile_cull=None, small_path=None)     # the image under test: the default call
            k = L.f3dg_debug_last_render_kernel()
            assert kernel in k and (b"scan_th=%d" % opts["render_scan_th"] in k if "render_scan_th" in opts else True), k
            assert ws_c.num_rendered <= ws.num_rendered
            _assert_inputs_are_the_oracles(name, h)
            label = "scan %s" % k.decode()
            _check(name, label + " unculled", 8.0, h["out_color"], None, None, failures, dist_big_rtol=2e-3)
            _check(name, label, 8.0, culled.cpu().numpy(), None, None, failures, dist_big_rtol=2e-3)
    assert not failures, failures
