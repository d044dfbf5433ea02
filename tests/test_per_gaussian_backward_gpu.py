"""The per-Gaussian stage of the backward (preprocess_bwd_kernel: view2gaussian chain rule, SH backward, per-view register sums,
single-writer adds) against the float64 chain rule ON ITS OWN INPUTS.

The kernel narrows its float64 accumulators to dv[10], writes exactly those floats to dL_dview2gaussian and uses them; in the SH branch
it reads dL_dcolor back from the array the caller gets. A float64 chain rule fed with the call's own exported dL_dview2gaussian /
dL_dcolors therefore sees bit-identical inputs and the only error left is the kernel's float32 arithmetic -- directly comparable with
the oracle's float32 error against the truth built from the oracle's inputs (tests/per_gaussian_fixtures.py, conditions checked on the
CPU by tests/test_per_gaussian_backward.py). No floor:
  (a) per group   max|g - truth| / max|truth| <= 4 e_o           (4: the project's margin for a float32 kernel against the float32
                                                                   reference, tests/test_epilogue_backward_gpu.py)
  (b) per group, over the elements of the Gaussians some view sees, K = err / (2^-24 A), A = sum of the |single-input parts|:
      99th percentile and maximum <= 4 x the oracle's -- low-gradient Gaussians held to their own scale
  dL_dsh          max err / max <= max(4 e_o, 16 * 2^-24): a sum over V <= 3 views of products of at most five rounded factors
  exact zeros for Gaussians no view sees and for SH coefficients above the active degree.
Both compositing backwards (bwd_dense 1 / 0: accumulator records of 16 / 10 doubles), two sets in one call, and the add-into contract
of include/f3dg.h through ctypes. The figures measured on an MI355X are in DESIGN.md section 3d: every bar met, the K percentiles of
kernel and oracle within 5-30 % of each other. Both sides of (a) and the K maxima are maxima of heavy-tailed samples and move with the
last bits of the inputs (the oracle's e_o by 1.6x to 50x); the largest e_h / e_o and K-maximum ratios measured were 3.1
(odd_deg1_of_16 rotation, three_views mean; dense) against the factor 4, which is kept as set."""
import ctypes as C

import numpy as np
import pytest
import torch

import f3dgaus_amd as f3d
import per_gaussian_fixtures as F
from f3dgaus_amd import _lib
from f3dgaus_amd.diff_gof_rasterization.backward import rasterize_backward_raw
from grad_truth import per_gaussian_term_magnitude, per_gaussian_truth_views

pytestmark = pytest.mark.gpu
PER_GAUSS = ("dL_dopacity", "dL_dmeans3D", "dL_dsh", "dL_dscales", "dL_drotations")
GAUSS = ("means3D", "opacities", "scales", "rotations", "shs", "colors_precomp")
CAMS = ("viewmatrix", "projmatrix", "campos")


def _joined(names):
    """The scenes as the sets of one call (one name: that scene)."""
    scenes = [F.scene(n) for n in names]
    sc = dict(scenes[0])
    for k in GAUSS:
        sc[k] = None if scenes[0][k] is None else torch.cat([s[k] for s in scenes], 0).contiguous()
    for k in CAMS:
        sc[k] = torch.cat([s[k] for s in scenes], 0).contiguous()
    return sc, np.concatenate([F.dpix(n) for n in names], 0)


def _forward(sc, device, n_sets):
    dev = lambda t: None if t is None else t.to(device)
    return f3d.rasterize_views(
        dev(sc["means3D"]), dev(sc["opacities"]), dev(sc["viewmatrix"]), dev(sc["projmatrix"]), dev(sc["campos"]), dev(sc["bg"]),
        image_height=sc["H"], image_width=sc["W"], tanfovx=sc["tanfovx"], tanfovy=sc["tanfovy"], sh=dev(sc["shs"]),
        colors_precomp=dev(sc["colors_precomp"]), scales=dev(sc["scales"]), rotations=dev(sc["rotations"]), sh_degree=sc["sh_degree"],
        scale_modifier=sc["scale_modifier"], kernel_size=sc["kernel_size"], save_aux=True, n_sets=n_sets)


def _hip_fwd_bwd(names, dense, device):
    """tests/test_raster_backward_gpu.py's _hip_fwd_bwd under option bwd_dense; the truth and A from THAT call's exports."""
    sc, dpix = _joined(names)
    n_sets = len(names)
    dev = lambda t: None if t is None else t.to(device)
    L = _lib.lib()
    try:
        assert L.f3dg_set_option(b"bwd_dense", dense) == 0
        out, radii, ws = _forward(sc, device, n_sets)
        g = rasterize_backward_raw(ws, dev(sc["means3D"]), dev(sc["shs"]), dev(sc["colors_precomp"]), dev(sc["scales"]), dev(sc["rotations"]),
                                   radii, torch.from_numpy(dpix).to(device), sc["sh_degree"], dev(sc["viewmatrix"]), dev(sc["projmatrix"]),
                                   dev(sc["campos"]), dev(sc["bg"]), sc["tanfovx"], sc["tanfovy"], sc["kernel_size"], sc["scale_modifier"],
                                   n_sets=n_sets)
        torch.cuda.synchronize()
    finally:
        L.f3dg_set_option(b"bwd_dense", 1)
    g = {k: v.cpu().numpy() for k, v in g.items()}
    radii = radii.cpu().numpy().reshape(dpix.shape[0], -1)
    return sc, g, radii, _truth_and_A(sc, g, radii, n_sets)


def _truth_and_A(sc, g, radii, n_sets=1):
    views = range(radii.shape[0])
    args = (sc, views, radii, g["dL_dview2gaussian"], g["dL_dcolors"])
    return per_gaussian_truth_views(*args, n_sets=n_sets), per_gaussian_term_magnitude(*args, n_sets=n_sets)


def _check_against_truth(label, name, g, truth, A, radii, rows, failures):
    """(a), (b) and the dL_dsh bar for the Gaussians `rows` (one set) against the oracle's figures on scene `name`."""
    ref = F.oracle_reference(name)
    assert np.array_equal(radii > 0, ref["radii"] > 0), label           # the same Gaussians are seen: the two error figures cover the same elements
    seen = ref["seen"]
    for k in F.GROUPS:
        gh, t, a = g[F.HIP_KEY[k]][rows], truth[k][rows], A[k][rows]
        e_h, e_o = F.rel(gh, t), ref["e_o"][k]
        kh, ko = F.k_stats(gh, t, a, seen), ref["K"][k]
        print(f"{label} {k}: e_h {e_h:.2e} e_o {e_o:.2e} | K p99 hip {kh[1]:.2f} oracle {ko[1]:.2f} | K max hip {kh[2]:.1f} oracle {ko[2]:.1f}")
        if not e_h <= 4.0 * e_o:
            failures.append((label, k, "(a)", e_h, e_o))
        if not kh[1] <= 4.0 * ko[1]:
            failures.append((label, k, "(b) p99", kh[1], ko[1]))
        if not kh[2] <= 4.0 * ko[2]:
            failures.append((label, k, "(b) max", kh[2], ko[2]))
    if truth["dL_dsh"] is not None:
        e_h, e_o = F.rel(g["dL_dsh"][rows], truth["dL_dsh"][rows]), ref["e_o"]["dL_dsh"]
        print(f"{label} dL_dsh: e_h {e_h:.2e} e_o {e_o:.2e}")
        if not e_h <= max(4.0 * e_o, 16 * F.EPS):
            failures.append((label, "dL_dsh", e_h, e_o))
    # Gaussians no view of their set sees: exact zeros in all five per-Gaussian arrays
    assert (~seen).any() or name not in ("three_views", "three_views_seed1", "odd_deg1_of_16_stretched")
    for k in PER_GAUSS:
        assert not g[k][rows][~seen].any(), (label, k)
    if name.startswith("odd_deg1_of_16"):            # D = 1 of M = 16: the inactive coefficients are never touched
        assert g["dL_dsh"][rows].shape[1] == 16 and not g["dL_dsh"][rows][:, 4:].any() and g["dL_dsh"][rows][:, :4].any()


@pytest.mark.parametrize("dense", [1, 0])
@pytest.mark.parametrize("name", F.FIXTURES)
def test_per_gaussian_stage_against_float64_on_its_own_inputs(name, dense, gpu_device):
    sc, g, radii, (truth, A) = _hip_fwd_bwd([name], dense, gpu_device)
    failures = []
    _check_against_truth(f"{name} dense={dense}", name, g, truth, A, radii, slice(None), failures)
    assert not failures, failures


def test_two_sets_in_one_call_against_float64_on_their_own_inputs(gpu_device):
    """Two different three-view sets through rasterize_views(n_sets=2) / f3dg_backward_sets (always the dense compositing backward): each
    set's rows against the truth of its own three views -- so a set's dL_dscales / dL_drotations do not depend on the other set."""
    names = ["three_views", "three_views_seed1"]
    sc, g, radii, (truth, A) = _hip_fwd_bwd(names, 1, gpu_device)
    P = F.scene(names[0])["P"]
    assert g["dL_dscales"].shape == (2 * P, 3) and radii.shape == (6, P)
    failures = []
    for s, name in enumerate(names):
        _check_against_truth(f"2 sets, set {s}", name, g, truth, A, radii[3 * s:3 * s + 3], slice(s * P, (s + 1) * P), failures)
    assert not failures, failures


def _pattern(shape, magnitude):
    """Deterministic, non-zero, |value| in [0.25, 1) x magnitude, alternating sign."""
    i = np.arange(int(np.prod(shape)), dtype=np.float64)
    v = magnitude * (0.25 + 0.75 * ((i * 0.6180339887498949) % 1.0)) * np.where(i % 2 == 0, 1.0, -1.0)
    return v.astype(np.float32).reshape(shape)


def _raw_backward_into(ws, sc, radii, dpix, device, prefill):
    """f3dg_backward_sets (one set) through ctypes, as tests/test_sets_backward_gpu.py's _raw_backward_sets, with the per-Gaussian
    sums starting from `prefill` (zeros where it has no entry)."""
    P, V, M = sc["P"], sc["viewmatrix"].shape[0], sc["shs"].shape[1]
    e = lambda *s: torch.full(s, float("nan"), dtype=torch.float32, device=device)
    shapes = dict(dL_dopacity=(P, 1), dL_dmeans3D=(P, 3), dL_dsh=(P, M, 3), dL_dscales=(P, 3), dL_drotations=(P, 4))
    g = {k: (torch.from_numpy(prefill[k]).to(device).contiguous() if k in prefill else torch.zeros(s, dtype=torch.float32, device=device))
         for k, s in shapes.items()}
    g.update(dL_dmeans2D=e(V, P, 3), dL_dcolors=e(V, P, 3), dL_dview2gaussian=e(V, P, 10))
    t = {k: sc[k].to(device).contiguous() for k in ("means3D", "shs", "scales", "rotations", "viewmatrix", "projmatrix", "campos", "bg")}
    d = torch.from_numpy(dpix).to(device).contiguous()
    rc = _lib.lib().f3dg_backward_sets(
        C.c_void_p(torch.cuda.current_stream().cuda_stream), C.c_void_p(ws.buffer.data_ptr()), ws.nbytes, ws.max_rendered, 1, V, P,
        sc["sh_degree"], M, _lib.ptr(t["bg"]), sc["W"], sc["H"], _lib.ptr(t["means3D"]), _lib.ptr(t["shs"]), None,
        _lib.ptr(t["scales"]), float(sc["scale_modifier"]), _lib.ptr(t["rotations"]), None, None, _lib.ptr(t["viewmatrix"]),
        _lib.ptr(t["projmatrix"]), _lib.ptr(t["campos"]), float(sc["tanfovx"]), float(sc["tanfovy"]), float(sc["kernel_size"]),
        _lib.ptr(radii), _lib.ptr(d), _lib.ptr(g["dL_dmeans2D"]), None, _lib.ptr(g["dL_dopacity"]), _lib.ptr(g["dL_dcolors"]),
        _lib.ptr(g["dL_dmeans3D"]), None, _lib.ptr(g["dL_dsh"]), _lib.ptr(g["dL_dscales"]), _lib.ptr(g["dL_drotations"]),
        _lib.ptr(g["dL_dview2gaussian"]), 0)
    assert rc == _lib.OK, rc
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in g.items()}


@pytest.mark.parametrize("dense", [1, 0])
def test_per_gaussian_sums_are_added_into_the_callers_arrays(dense, gpu_device):
    """include/f3dg.h: the per-Gaussian sums "are added into and must be zero-filled (or hold running sums) by the caller". Running sums
    of at most max|g| per array: rows no view sees and the SH coefficients above the active degree come back bit-identical; elsewhere
    out - prefill meets bar (a) plus 2^-23 (one rounding of prefill + g, |prefill + g| <= 2 max|g|) against the truth of this run's own
    exports. dL_dopacity belongs to the compositing stage: against the zero-filled run, at the project's bar for two runs of one call."""
    name = "odd_deg1_of_16_stretched"
    sc, dpix, ref = F.scene(name), F.dpix(name), F.oracle_reference(name)
    L = _lib.lib()
    try:
        assert L.f3dg_set_option(b"bwd_dense", dense) == 0
        out, radii, ws = _forward(sc, gpu_device, 1)
        zero = _raw_backward_into(ws, sc, radii, dpix, gpu_device, {})
        prefill = {k: _pattern(zero[k].shape, float(np.abs(zero[k]).max())) for k in PER_GAUSS}
        assert all(np.abs(p).min() > 0 for p in prefill.values())
        got = _raw_backward_into(ws, sc, radii, dpix, gpu_device, prefill)
    finally:
        L.f3dg_set_option(b"bwd_dense", 1)
    radii = radii.cpu().numpy().reshape(1, -1)
    assert np.array_equal(radii > 0, ref["radii"] > 0)
    hidden = ~ref["seen"]
    assert hidden.sum() >= 20
    for k in PER_GAUSS:
        assert np.array_equal(got[k][hidden].view(np.uint32), prefill[k][hidden].view(np.uint32)), k
    assert np.array_equal(got["dL_dsh"][:, 4:].view(np.uint32), prefill["dL_dsh"][:, 4:].view(np.uint32))
    truth, _ = _truth_and_A(sc, got, radii)
    added = {k: got[k].astype(np.float64) - prefill[k] for k in PER_GAUSS}
    failures = []
    for k in F.GROUPS + ("dL_dsh",):
        e_h, e_o = F.rel(added[F.HIP_KEY[k]], truth[k]), ref["e_o"][k]
        bar = (4.0 * e_o if k != "dL_dsh" else max(4.0 * e_o, 16 * F.EPS)) + 2.0 ** -23
        print(f"add-into dense={dense} {k}: e_h {e_h:.2e} e_o {e_o:.2e} bar {bar:.2e}")
        if not e_h <= bar:
            failures.append((k, e_h, e_o))
    e = F.rel(added["dL_dopacity"], zero["dL_dopacity"].astype(np.float64))
    print(f"add-into dense={dense} dL_dopacity vs the zero-filled run: {e:.2e}")
    assert e <= 1e-5 + 2.0 ** -23
    assert not failures, failures
