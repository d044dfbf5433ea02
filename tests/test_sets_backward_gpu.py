"""Several Gaussian sets x several views in one forward and one backward launch sequence (f3dg_forward_sets with
F3DG_FLAG_SAVE_AUX | F3DG_FLAG_SETS_AUX, then f3dg_backward_sets) against f3dg_backward on each set alone.

Shapes: P = 700 (two full 256-blocks and a partial one), 72 x 40 pixels (partial tiles in both axes), three different sets -- one of
them with Gaussians behind the camera --, two different cameras per set. Tolerances are the project's own for the same comparison
across calls (tests/test_raster_backward_gpu.py): dL_dview2gaussian 1e-6, dL_dcolors / dL_dmeans2D 1e-5 (test_multi_view_backward_sums_
single_view_backwards), dL_dopacity / dL_dsh 1e-4, dL_dmeans3D / dL_dscales / dL_drotations 1e-3 (test_autograd_function_matches_raw_backward);
the oracle bars are those of test_backward_vs_oracle (1e-5, 2e-5 for mean2D)."""
import ctypes as C

import numpy as np
import pytest
import torch

import f3dgaus_amd as f3d
from f3dgaus_amd import _lib
from f3dgaus_amd.diff_gof_rasterization.backward import rasterize_backward_raw
from helpers import make_scene, run_oracle

gpu = pytest.mark.gpu
P, RES, NS, VPS = 700, (72, 40), 3, 2
GAUSS = ("means3D", "opacities", "scales", "rotations", "shs")
CAMS = ("viewmatrix", "projmatrix", "campos")
PER_VIEW = {"dL_dview2gaussian": 1e-6, "dL_dcolors": 1e-5, "dL_dmeans2D": 1e-5}
PER_GAUSS = {"dL_dopacity": 1e-4, "dL_dsh": 1e-4, "dL_dmeans3D": 1e-3, "dL_dscales": 1e-3, "dL_drotations": 1e-3}
_CACHE = {}


def _sets():
    """The three sets (never modified)."""
    if "sets" not in _CACHE:
        _CACHE["sets"] = [make_scene(P=P, res=RES, s0=0.05, seed=0, view=[1, 4], bg=(0.3, 0.1, 0.6)),
                          make_scene(P=P, res=RES, s0=0.04, seed=1, view=[2, 6], behind_fraction=0.2, bg=(0.3, 0.1, 0.6)),
                          make_scene(P=P, res=RES, s0=0.06, seed=2, view=[3, 7], bg=(0.3, 0.1, 0.6))]
    return _CACHE["sets"]


def _dpix(n_views, seed=11):
    return np.random.default_rng(seed).standard_normal((n_views, 9, RES[1], RES[0])).astype(np.float32)


def _concat(sets, views=slice(None)):
    sc = dict(sets[0])
    for k in GAUSS:
        sc[k] = torch.cat([s[k] for s in sets], 0).contiguous()
    for k in CAMS:
        sc[k] = torch.cat([s[k][views] for s in sets], 0).contiguous()
    return sc


def _one_set(scene, views=slice(None)):
    sc = dict(scene)
    for k in CAMS:
        sc[k] = scene[k][views].contiguous()
    return sc


def _fwd_bwd(scene, dpix, device, n_sets=1, bg=None):
    """tests/test_raster_backward_gpu.py's _hip_fwd_bwd, with n_sets: one forward that keeps the auxiliary planes, one backward."""
    dev = lambda t: None if t is None else t.to(device)
    bg = scene["bg"] if bg is None else bg
    out, radii, ws = f3d.rasterize_views(
        dev(scene["means3D"]), dev(scene["opacities"]), dev(scene["viewmatrix"]), dev(scene["projmatrix"]),
        dev(scene["campos"]), dev(bg), image_height=scene["H"], image_width=scene["W"],
        tanfovx=scene["tanfovx"], tanfovy=scene["tanfovy"], sh=dev(scene["shs"]),
        colors_precomp=dev(scene["colors_precomp"]), scales=dev(scene["scales"]), rotations=dev(scene["rotations"]),
        sh_degree=scene["sh_degree"], scale_modifier=scene["scale_modifier"], kernel_size=scene["kernel_size"], save_aux=True,
        n_sets=n_sets)
    g = rasterize_backward_raw(ws, dev(scene["means3D"]), dev(scene["shs"]), dev(scene["colors_precomp"]),
                               dev(scene["scales"]), dev(scene["rotations"]), radii, torch.from_numpy(dpix).to(device),
                               scene["sh_degree"], dev(scene["viewmatrix"]), dev(scene["projmatrix"]), dev(scene["campos"]),
                               dev(bg), scene["tanfovx"], scene["tanfovy"], scene["kernel_size"], scene["scale_modifier"],
                               n_sets=n_sets)
    torch.cuda.synchronize()
    res = {k: v.cpu().numpy() for k, v in g.items()}
    res["radii"], res["raster"] = radii.cpu().numpy(), out.cpu().numpy()
    return res, ws


def _rel(a, b):
    m = np.abs(b).max()
    return 0.0 if m == 0 else float(np.abs(a.astype(np.float64) - b).max() / m)


def _reference(device):
    """The batched run and f3dg_backward on each set alone, computed once and shared (read-only)."""
    if "ref" not in _CACHE:
        sets, dpix = _sets(), _dpix(NS * VPS)
        batched, _ = _fwd_bwd(_concat(sets), dpix, device, n_sets=NS)
        alone = [_fwd_bwd(sets[s], dpix[s * VPS:(s + 1) * VPS], device)[0] for s in range(NS)]
        _CACHE["ref"] = (batched, alone, dpix)
    return _CACHE["ref"]


def _assert_agreement(batched, alone, n_sets, vps, label):
    for s in range(n_sets):
        vs, gs = slice(s * vps, (s + 1) * vps), slice(s * P, (s + 1) * P)
        assert np.array_equal(batched["radii"][vs], alone[s]["radii"]), (label, s)
        assert np.array_equal(batched["raster"][vs], alone[s]["raster"]), (label, s)
        for k, tol in PER_VIEW.items():
            for v in range(vps):
                e = _rel(batched[k][s * vps + v], alone[s][k][v])
                assert e <= tol, (label, k, s, v, e)
        for k, tol in PER_GAUSS.items():
            e = _rel(batched[k][gs], alone[s][k])
            print(f"{label} set {s} {k}: {e:.2e}")
            assert e <= tol, (label, k, s, e)


@gpu
def test_batched_sets_agree_with_each_set_alone(gpu_device):
    batched, alone, _ = _reference(gpu_device)
    assert batched["dL_dmeans3D"].shape == (NS * P, 3) and batched["dL_dsh"].shape[0] == NS * P
    assert batched["dL_dview2gaussian"].shape == (NS * VPS, P, 10)
    assert (alone[1]["radii"] == 0).any() and all(np.abs(a["dL_dmeans3D"]).max() > 0 for a in alone)
    _assert_agreement(batched, alone, NS, VPS, "sets")
    # Gaussians no view of their own set sees get nothing, whatever the other sets' views would have seen of them
    for s in range(NS):
        hidden = (alone[s]["radii"] == 0).all(0)
        for k in ("dL_dmeans3D", "dL_dscales", "dL_drotations", "dL_dopacity", "dL_dsh"):
            assert not batched[k][s * P:(s + 1) * P][hidden].any(), (k, s)


@gpu
def test_a_set_inside_the_batch_against_the_oracle(gpu_device):
    batched, _, dpix = _reference(gpu_device)
    s = 2
    for v in range(VPS):
        o = run_oracle(_sets()[s], view=v)
        go = o["oracle"].backward(dpix[s * VPS + v])
        n = s * VPS + v
        assert np.array_equal(batched["radii"][n], o["radii"])
        assert _rel(batched["dL_dview2gaussian"][n], go["dL_dview2gaussian"]) <= 1e-5
        assert _rel(batched["dL_dcolors"][n], go["dL_dcolor"]) <= 1e-5
        assert _rel(batched["dL_dmeans2D"][n], go["dL_dmean2D"]) <= 2e-5


@gpu
def test_sets_are_isolated(gpu_device):
    """Zero cotangent on every view of set 1: its per-Gaussian gradients are exactly zero. Replacing set 1's Gaussians by others leaves
    set 0's and set 2's gradients alone. The compositing backward adds the (pixel, Gaussian) terms of a Gaussian with float atomics in
    a run-dependent order, so two runs of the very same call differ in the last bits of a few rows of dL_dcolors / dL_dview2gaussian:
    bit-identity is asserted for what the per-Gaussian stage computes -- one writer per Gaussian, fixed view order -- from rows that
    did come out equal (dL_dsh given equal dL_dcolors; dL_dmeans3D / dL_dscales / dL_drotations given equal dL_dcolors and
    dL_dview2gaussian); the compositing-stage sums themselves are held to 1e-6 of their maximum, the bar two runs of one call meet
    (test_known_answers_and_kernel_variants)."""
    sets = _sets()
    dpix = _dpix(NS * VPS).copy()
    dpix[VPS:2 * VPS] = 0.0
    a, _ = _fwd_bwd(_concat(sets), dpix, gpu_device, n_sets=NS)
    other = make_scene(P=P, res=RES, s0=0.08, seed=9, view=[2, 6], bg=(0.3, 0.1, 0.6))
    for k in CAMS:
        other[k] = sets[1][k]
    b, _ = _fwd_bwd(_concat([sets[0], other, sets[2]]), dpix, gpu_device, n_sets=NS)
    assert not np.array_equal(a["raster"][VPS:2 * VPS], b["raster"][VPS:2 * VPS])       # set 1 did change
    for run in (a, b):
        for k in PER_GAUSS:
            assert not run[k][P:2 * P].any(), k
    for s in (0, 2):
        vs, gs = slice(s * VPS, (s + 1) * VPS), slice(s * P, (s + 1) * P)
        assert np.array_equal(a["raster"][vs], b["raster"][vs]) and np.array_equal(a["radii"][vs], b["radii"][vs])
        for k in ("dL_dview2gaussian", "dL_dcolors", "dL_dmeans2D"):
            assert _rel(b[k][vs], a[k][vs]) <= 1e-6, (k, s)
        for k in ("dL_dopacity", "dL_dsh"):
            assert _rel(b[k][gs], a[k][gs]) <= 1e-6, (k, s)
        same_col = (a["dL_dcolors"][vs] == b["dL_dcolors"][vs]).all(axis=(0, 2))                    # [P]
        same_v2g = (a["dL_dview2gaussian"][vs] == b["dL_dview2gaussian"][vs]).all(axis=(0, 2))
        seen = (a["radii"][vs] > 0).any(0)
        assert (same_col & same_v2g & seen).any()              # (the bit-identity below is about Gaussians that did receive gradients)
        assert np.array_equal(a["dL_dsh"][gs][same_col], b["dL_dsh"][gs][same_col]), s
        both = same_col & same_v2g
        for k in ("dL_dmeans3D", "dL_dscales", "dL_drotations"):
            assert np.array_equal(a[k][gs][both], b[k][gs][both]), (k, s)
            assert _rel(b[k][gs], a[k][gs]) <= 1e-3, (k, s)


@gpu
def test_two_sets_of_one_view_take_the_general_path(gpu_device):
    """n_sets = 2, views_per_set = 1: two views in all, where a call of ONE set would take the small-call path. The header says which
    path ran (f3dg_debug_export refuses the instance offsets on a small-path workspace)."""
    sets = _sets()[:2]
    dpix = _dpix(2, seed=12)
    batched, ws = _fwd_bwd(_concat(sets, slice(0, 1)), dpix, gpu_device, n_sets=2)
    offsets = torch.empty((2, P), dtype=torch.int32, device=gpu_device)
    rc = _lib.lib().f3dg_debug_export(C.c_void_p(torch.cuda.current_stream().cuda_stream), C.c_void_p(ws.buffer.data_ptr()), P, RES[0], RES[1], 2,
                                      ws.max_rendered, *([None] * 4), _lib.ptr(offsets), *([None] * 7))
    assert rc == _lib.OK, rc           # (ERR_STATE on a small-path workspace)
    alone = [_fwd_bwd(_one_set(sets[s], slice(0, 1)), dpix[s:s + 1], gpu_device)[0] for s in range(2)]
    _assert_agreement(batched, alone, 2, 1, "2x1")


@gpu
def test_per_view_background_with_sets(gpu_device):
    sets = _sets()
    bg = torch.from_numpy(np.random.default_rng(4).uniform(0, 1, (NS * VPS, 3)).astype(np.float32))
    dpix = _dpix(NS * VPS, seed=13)
    batched, _ = _fwd_bwd(_concat(sets), dpix, gpu_device, n_sets=NS, bg=bg)
    alone = [_fwd_bwd(sets[s], dpix[s * VPS:(s + 1) * VPS], gpu_device, bg=bg[s * VPS:(s + 1) * VPS])[0] for s in range(NS)]
    plain, _, _ = _reference(gpu_device)
    assert not np.array_equal(batched["raster"], plain["raster"])
    _assert_agreement(batched, alone, NS, VPS, "bg per view")


def _raw_backward_sets(ws, scene, radii, dpix, device, n_sets, vps):
    """f3dg_backward_sets through ctypes (the wrapper calls f3dg_backward for one set)."""
    dev = lambda t: t.to(device).contiguous()
    V, M = n_sets * vps, scene["shs"].shape[1]
    z = lambda *s: torch.zeros(s, dtype=torch.float32, device=device)
    e = lambda *s: torch.full(s, float("nan"), dtype=torch.float32, device=device)
    g = dict(dL_dmeans2D=e(V, P, 3), dL_dopacity=z(n_sets * P, 1), dL_dcolors=e(V, P, 3), dL_dmeans3D=z(n_sets * P, 3),
             dL_dsh=z(n_sets * P, M, 3), dL_dscales=z(n_sets * P, 3), dL_drotations=z(n_sets * P, 4), dL_dview2gaussian=e(V, P, 10))
    t = {k: dev(scene[k]) for k in GAUSS + CAMS + ("bg",)}
    d = torch.from_numpy(dpix).to(device).contiguous()
    rc = _lib.lib().f3dg_backward_sets(
        C.c_void_p(torch.cuda.current_stream().cuda_stream), C.c_void_p(ws.buffer.data_ptr()), ws.nbytes, ws.max_rendered, n_sets, vps, P,
        scene["sh_degree"], M, _lib.ptr(t["bg"]), scene["W"], scene["H"], _lib.ptr(t["means3D"]), _lib.ptr(t["shs"]), None,
        _lib.ptr(t["scales"]), float(scene["scale_modifier"]), _lib.ptr(t["rotations"]), None, None, _lib.ptr(t["viewmatrix"]),
        _lib.ptr(t["projmatrix"]), _lib.ptr(t["campos"]), float(scene["tanfovx"]), float(scene["tanfovy"]), float(scene["kernel_size"]),
        _lib.ptr(radii), _lib.ptr(d), _lib.ptr(g["dL_dmeans2D"]), None, _lib.ptr(g["dL_dopacity"]), _lib.ptr(g["dL_dcolors"]),
        _lib.ptr(g["dL_dmeans3D"]), None, _lib.ptr(g["dL_dsh"]), _lib.ptr(g["dL_dscales"]), _lib.ptr(g["dL_drotations"]),
        _lib.ptr(g["dL_dview2gaussian"]), 0)
    assert rc == _lib.OK, rc
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in g.items()}


@gpu
def test_backward_sets_of_one_set_is_f3dg_backward(gpu_device):
    scene = _sets()[0]
    dpix = _dpix(VPS, seed=14)
    ref, ws = _fwd_bwd(scene, dpix, gpu_device)                   # f3dg_backward on this workspace ...
    radii = torch.from_numpy(ref["radii"]).to(gpu_device)
    got = _raw_backward_sets(ws, scene, radii, dpix, gpu_device, 1, VPS)        # ... and f3dg_backward_sets(n_sets = 1) on the same planes
    for k, tol in list(PER_VIEW.items()) + list(PER_GAUSS.items()):
        assert np.isfinite(got[k]).all(), k
        e = _rel(got[k], ref[k])
        assert e <= tol, (k, e)


# ---- host-side argument checks: they run before any HIP call
def _forward_sets_rc(n_sets, flags, v2g=False, ws_bytes=1 << 40):
    L = _lib.lib()
    buf = (C.c_char * 1024)()
    p = C.cast(buf, C.c_void_p)
    return L.f3dg_forward_sets(None, p, ws_bytes, 1000, n_sets, 1, 100, 1, 4, p, 64, 64, p, p, None, p, p, 1.0, p, None, p if v2g else None,
                               p, p, p, 0.1, 0.1, 0.0, p, None, flags)


def test_flag_and_forward_argument_checks(f3d):
    assert _lib.FLAG_SETS_AUX == 512
    for n_sets in (1, 2):
        assert _forward_sets_rc(n_sets, _lib.FLAG_SETS_AUX) == _lib.ERR_BAD_ARG                       # SETS_AUX without SAVE_AUX
    assert _forward_sets_rc(2, _lib.FLAG_SAVE_AUX) == _lib.ERR_BAD_ARG                                # the promise is missing
    assert _forward_sets_rc(2, _lib.FLAG_SAVE_AUX, ws_bytes=1024) == _lib.ERR_WORKSPACE                 # (the size is looked at first, as before)
    assert _forward_sets_rc(2, _lib.FLAG_SAVE_AUX | _lib.FLAG_SETS_AUX, v2g=True) == _lib.ERR_BAD_ARG
    assert _forward_sets_rc(2, 0, v2g=True) == _lib.ERR_BAD_ARG
    # both flags with a workspace that is too small
    assert _forward_sets_rc(2, _lib.FLAG_SAVE_AUX | _lib.FLAG_SETS_AUX, ws_bytes=1024) == _lib.ERR_WORKSPACE
    assert _forward_sets_rc(1, _lib.FLAG_SAVE_AUX | _lib.FLAG_SETS_AUX, ws_bytes=1024) == _lib.ERR_WORKSPACE


def test_backward_sets_argument_checks(f3d):
    L = _lib.lib()
    buf = (C.c_char * 1024)()
    p = C.cast(buf, C.c_void_p)

    def rc(n_sets=2, vps=2, ws_bytes=1024, v2g=None, outs=None, **kw):
        o = dict(mean2D=p, opacity=p, color=p, mean3D=p, sh=p, scale=p, rot=p, v2g=p)
        o.update(outs or {})
        a = dict(ws=p, bg=p, means3D=p, vm=p, cp=p, dpix=p)
        a.update(kw)
        return L.f3dg_backward_sets(None, a["ws"], ws_bytes, 1000, n_sets, vps, 100, 1, 4, a["bg"], 64, 64, a["means3D"], p, None, p, 1.0, p,
                                    None, v2g, a["vm"], p, a["cp"], 0.1, 0.1, 0.0, None, a["dpix"], o["mean2D"], None, o["opacity"],
                                    o["color"], o["mean3D"], None, o["sh"], o["scale"], o["rot"], o["v2g"], 0)
    assert rc() == _lib.ERR_WORKSPACE                       # every argument in order: the next check is the workspace size
    assert rc(n_sets=1) == _lib.ERR_WORKSPACE
    for name in ("mean2D", "opacity", "color", "mean3D", "sh", "scale", "rot", "v2g"):
        assert rc(outs={name: None}) == _lib.ERR_BAD_ARG, name
    for name in ("ws", "bg", "means3D", "vm", "cp", "dpix"):
        assert rc(**{name: None}) == _lib.ERR_BAD_ARG, name
    assert rc(n_sets=0) == _lib.ERR_BAD_ARG and rc(vps=0) == _lib.ERR_BAD_ARG
    assert rc(v2g=p) == _lib.ERR_BAD_ARG and rc(n_sets=1, v2g=p) == _lib.ERR_WORKSPACE
