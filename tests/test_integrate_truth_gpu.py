"""The point integration (csrc/f3dg_integrate.hip) against the float64 truth ON ITS OWN INPUTS (tests/integrate_truth.py; the conditions are
held on the CPU by tests/test_integrate_truth.py), and its per-pixel table against the plain transcription bit for bit.

Every call is integrate_prepare + integrate_points, once on the default launch sequence (545 shared rays per tile, the rotating edge wave)
and once under option reference_kernels (integrate_pass1_kernel on every tile). The call's own records, list and ranges (f3dg_debug_export)
are asserted bit-equal to the oracle's on the Gaussians that are in a list, so kernel and oracle are measured against ONE truth; the table
of the per-pixel pass comes from f3dg_debug_integrate_export.

  (a) bars      on the truth's kept pixels the contributor table (contrib_n, ids[:n]), the last contributor and the max-depth channel are
                exactly the truth's; for rgb, alpha, final_T and alpha_integrated the median, 99th percentile and maximum of
                K = |x - truth| / (2^-24 A) are <= 4 x the oracle's for the same scene, group and statistic (4: the project's margin for a
                float32 kernel in the reference's arithmetic against the float32 reference, tests/test_compositing_truth_gpu.py; integrate
                has no fast arithmetic, so no second factor), K exactly 0 where A = 0; color_integrated is the image's pixel at the truth's
                pixel to the bit, rejected points hold the fills (1, 0, 0, 0); helpers_integrate.assert_integrate_parity as it is on everything
  (b) table     100 x 72, 33 x 18, 17 x 17, 16 x 12 and nine cameras at 48 x 48 in one prepare ((tile + view) & 7 takes all eight values): table,
                last contributor, final_T and the nine image channels identical between the two calls over ALL pixels, every camera of the
                batched prepare identical to its single-camera prepare
  (c) wrap      tile lists of 70,000 entries, whose stored 16-bit positions wrap: pixels that stop at a wrapped id, pixels that accept an
                aliased one
  (d) short     lists of 0..5 contributors: each look-ahead slot of the pipelined point loop is the last one once
  (e) alpha_min torch.min(buffer, alpha_integrated) to the bit on every point, rejected ones included, NaN propagating

Measured on an MI355X: every bar met. Kernel K / oracle K, the largest over scenes and the three statistics (the two calls give the same
figures, their tables and images being bit-identical); the factor 4 is kept as derived:
    (a) the five bar scenes   rgb 1.14 (I1, maximum)   alpha 1.04 (one_more, median)   final_T 1.07 (small_bg, p99)   alpha_integrated 1.01
    (c) the wrap scenes       alpha_integrated 1.03 (wrap_stop, p99)
    (d) the short lists       rgb 1.00   alpha 1.55 (short0, maximum: 1.6 ulp of one term)   final_T 1.07   alpha_integrated 1.10 (short1, maximum)
The same table is in DESIGN.md section 3f-bis."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import integrate_truth as IT
from f3dgaus_amd import _lib
from helpers import make_scene
from helpers_integrate import assert_integrate_parity, make_points, npy

pytestmark = pytest.mark.gpu

M = 4.0


def _settings(sc, v, dev):
    from f3dgaus_amd.diff_gof_rasterization import GaussianRasterizationSettings_GOF
    d = lambda t: None if t is None else t.to(dev)
    return GaussianRasterizationSettings_GOF(sc["H"], sc["W"], sc["tanfovx"], sc["tanfovy"], sc["kernel_size"], torch.zeros(0), d(sc["bg"]),
                                             sc["scale_modifier"], d(sc["viewmatrix"][v]), d(sc["projmatrix"][v]), sc["sh_degree"],
                                             d(sc["campos"][v]), False, False)


def _prepare(sc, dev, max_points, view=0, batched=False):
    from f3dgaus_amd.diff_gof_rasterization import integrate_prepare, integrate_prepare_batched
    d = lambda t: None if t is None else t.to(dev)
    if batched:
        return integrate_prepare_batched(d(sc["means3D"]), d(sc["shs"]), d(sc["colors_precomp"]), d(sc["opacities"]), d(sc["scales"]),
                                         d(sc["rotations"]), d(sc["viewmatrix"]), d(sc["projmatrix"]), d(sc["campos"]), d(sc["bg"]),
                                         image_height=sc["H"], image_width=sc["W"], tanfovx=sc["tanfovx"], tanfovy=sc["tanfovy"],
                                         sh_degree=sc["sh_degree"], max_points=max_points, scale_modifier=sc["scale_modifier"],
                                         kernel_size=sc["kernel_size"])
    return integrate_prepare(d(sc["means3D"]), d(sc["shs"]), d(sc["colors_precomp"]), d(sc["opacities"]), d(sc["scales"]), d(sc["rotations"]),
                             None, None, _settings(sc, view, dev), max_points=max_points)


def _export(prep):
    """What the per-pixel pass left in a prepared workspace for the preparation's camera, and the inputs it read, as numpy."""
    L = _lib.lib()
    dev = prep.buffer.device
    HW, T, V, P = prep.H * prep.W, ((prep.W + 15) // 16) * ((prep.H + 15) // 16), prep.n_views, prep.P
    stream = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)
    ws = C.c_void_p(prep.buffer.data_ptr())
    cn = torch.zeros(HW, dtype=torch.int32, device=dev)
    ids = torch.zeros(HW * 1024, dtype=torch.int16, device=dev)
    last = torch.zeros(HW, dtype=torch.int32, device=dev)
    fT = torch.zeros(HW, dtype=torch.float32, device=dev)
    assert L.f3dg_debug_integrate_export(stream(), ws, P, prep.max_points, prep.W, prep.H, V, prep.capacity, prep.view,
                                         *[C.c_void_p(t.data_ptr()) for t in (cn, ids, last, fT)]) == 0
    rec = torch.zeros(V * P * 16, dtype=torch.float32, device=dev)
    plist = torch.zeros(max(prep.capacity, 1), dtype=torch.int32, device=dev)
    ranges = torch.zeros(V * T * 2, dtype=torch.int32, device=dev)
    none = [None] * 6
    assert L.f3dg_debug_export(stream(), ws, P, prep.W, prep.H, V, prep.capacity, C.c_void_p(rec.data_ptr()), *none,
                               C.c_void_p(plist.data_ptr()), C.c_void_p(ranges.data_ptr()), None, None, None) == 0
    torch.cuda.synchronize()
    n = npy(cn).view(np.uint32)
    table = npy(ids).view(np.uint16).reshape(HW, 1024).copy()
    table[np.arange(1024)[None, :] >= n[:, None]] = 0              # only the first contrib_n of a pixel's 1,024 are defined
    rec = npy(rec).reshape(V, P, 16)[prep.view]
    return dict(contrib_n=n, ids=table, last=npy(last).view(np.uint32).reshape(prep.H, prep.W), final_T=npy(fT).reshape(prep.H, prep.W),
                view2gaussian=rec[:, 0:10], opac=rec[:, 10], rgb=rec[:, 12:15], point_list=npy(plist).view(np.uint32)[:prep.num_rendered],
                ranges=npy(ranges).view(np.uint32).reshape(V, T, 2)[prep.view], num_rendered=prep.num_rendered)


def _points_stage(prep, pts, h):
    from f3dgaus_amd.diff_gof_rasterization import integrate_points
    ai, ci = integrate_points(prep, torch.from_numpy(np.array(pts)).to(prep.buffer.device))
    torch.cuda.synchronize()
    h.update(out=npy(prep.color).copy(), ai=npy(ai), ci=npy(ci), radii=npy(prep.radii))
    return h


def _call(sc, pts, dev, reference):
    L = _lib.lib()
    try:
        assert L.f3dg_set_option(b"reference_kernels", int(reference)) == 0
        prep = _prepare(sc, dev, len(pts))
        return _points_stage(prep, pts, _export(prep))
    finally:
        L.f3dg_set_option(b"reference_kernels", 0)


@functools.lru_cache(maxsize=None)
def _run(name, reference):
    return _call(IT.scene(name), IT.points(name), torch.device("cuda:0"), reference)


def _assert_inputs_are_the_oracles(label, h, o):
    """Records, list and ranges of the call, bit for bit the oracle's on the Gaussians that are in a list (the pattern of
    compositing_truth.assert_inputs_are_the_oracles): the truth of the oracle's records is then this call's truth."""
    assert h["num_rendered"] == o["num_rendered"], label
    assert np.array_equal(h["point_list"], o["point_list"]), (label, "point list")
    assert np.array_equal(h["ranges"], o["ranges"]), (label, "ranges")
    assert np.array_equal(h["radii"], o["radii"]), (label, "radii")
    used = np.zeros(len(o["radii"]), bool)
    used[o["point_list"]] = True
    assert used.any(), label
    for k, a, b in (("view2gaussian", h["view2gaussian"], o["view2gaussian"]), ("opacity*coef", h["opac"], o["conic_opacity"][:, 3]), ("rgb", h["rgb"], o["rgb"])):
        assert np.array_equal(np.ascontiguousarray(a[used]).view(np.uint32), np.ascontiguousarray(b[used]).view(np.uint32)), (label, k)


@functools.lru_cache(maxsize=None)
def _truth_table(name):
    p1 = IT.oracle_truth(name)[0]
    n = np.array([len(c) for c in p1["contrib"]], np.uint32)
    table = np.zeros((len(n), 1024), np.uint16)
    for i, c in enumerate(p1["contrib"]):
        table[i, :len(c)] = c & 0xFFFF
    return n, table


def _assert_table_is_the_truths(label, name, h):
    p1 = IT.oracle_truth(name)[0]
    keep = p1["keep"]
    n, table = _truth_table(name)
    k = keep.ravel()
    assert np.array_equal(h["contrib_n"][k], n[k]), (label, "contrib_n", int((h["contrib_n"][k] != n[k]).sum()))
    assert np.array_equal(h["ids"][k], table[k]), (label, "contributor ids", int((h["ids"][k] != table[k]).any(1).sum()))
    assert np.array_equal(h["last"][keep], p1["last"][keep]), (label, "last contributor")


def _check(name, groups=IT.GROUPS, parity=True):
    """The bars of (a) on a scene, for the default call and the plain one. Returns the two results."""
    p1, pt, fig_o = IT.oracle_truth(name)
    o = IT.oracle(name)
    failures, results = [], []
    for reference in (False, True):
        label = "%s %s" % (name, "reference_kernels" if reference else "default")
        h = _run(name, reference)
        results.append(h)
        _assert_inputs_are_the_oracles(label, h, o)
        _assert_table_is_the_truths(label, name, h)
        keep = p1["keep"]
        assert np.array_equal(h["out"][6].astype(np.float64)[keep], p1["out"][6][keep]), (label, "max depth")
        assert np.isfinite(h["out"]).all() and np.isfinite(h["ai"]).all(), label
        fig = IT.figures(p1, pt, h["out"], h["final_T"], h["ai"])
        IT.check_bars(label, p1, pt, fig, fig_o, M, failures, h["out"], h["final_T"], h["ai"], groups=groups)
        for g in groups:
            print("%s %-16s kernel / oracle  %s" % (label, g, " / ".join("%.2f" % (a / b) if b > 0 else "-" for a, b in zip(fig[g], fig_o[g]))))
        ok = pt["ok"]
        assert np.array_equal(h["ci"][ok].view(np.uint32), np.ascontiguousarray(h["out"][:3].reshape(3, -1).T[pt["pix"][ok]]).view(np.uint32)), label
        assert (h["ai"][~ok] == 1.0).all() and not h["ci"][~ok].any(), (label, "fills of the rejected points")
        if parity:
            assert_integrate_parity(o, h, label)
    assert not failures, failures
    return results


@pytest.mark.parametrize("name", list(IT.SCENES))
def test_integrate_against_float64_on_its_own_inputs(name, gpu_device):
    _check(name)


TABLE_SCENES = {"I4": None, "small_bg": None, "one_more": None,                                   # 100 x 72, 33 x 18, 17 x 17 of integrate_truth
                "part_tile": (dict(P=500, res=(16, 12), s0=0.05, view="oblique", bg=(0.4, 0.1, 0.9)), 2000)}   # one tile smaller than a tile


def _assert_same_bits(label, a, b):
    for k in ("contrib_n", "ids", "last", "radii"):
        assert np.array_equal(a[k], b[k]), (label, k)
    for k in ("final_T", "out", "ai", "ci"):
        assert np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), (label, k)


@pytest.mark.parametrize("name", list(TABLE_SCENES))
def test_table_is_the_plain_transcriptions(name, gpu_device):
    """Over ALL pixels: partial tiles, where the `active` / `eactive` logic of the corner and edge rays decides."""
    if TABLE_SCENES[name] is None:
        a, b = _run(name, False), _run(name, True)
    else:
        kw, n = TABLE_SCENES[name]
        sc = make_scene(**kw)
        pts = make_points(sc, n)
        a, b = _call(sc, pts, gpu_device, False), _call(sc, pts, gpu_device, True)
    assert (a["contrib_n"] > 0).mean() > 0.25 and a["out"][8].sum() > 0
    _assert_same_bits(name, a, b)


def test_batched_prepare_table_is_each_cameras_own(gpu_device):
    """Nine cameras at 48 x 48 in one prepare: 9 tiles per view, so the edge wave (tile + view) & 7 takes all eight values, and every view but
    the first reads its table at an offset."""
    sc = make_scene(P=3000, res=(48, 48), s0=0.05, view=range(9))
    V = sc["viewmatrix"].shape[0]
    assert V == 9 and {(t + v) & 7 for t in range(9) for v in range(V)} == set(range(8))
    pts = make_points(sc, 6000)
    L = _lib.lib()
    runs = {}
    for reference in (False, True):
        try:
            assert L.f3dg_set_option(b"reference_kernels", int(reference)) == 0
            runs[reference] = [_points_stage(p, pts, _export(p)) for p in _prepare(sc, gpu_device, len(pts), batched=True)]
        finally:
            L.f3dg_set_option(b"reference_kernels", 0)
    for v in range(V):
        _assert_same_bits("view %d batched, default / plain" % v, runs[False][v], runs[True][v])
        p = _prepare(sc, gpu_device, len(pts), view=v)
        single = _points_stage(p, pts, _export(p))
        _assert_same_bits("view %d batched / single" % v, runs[False][v], single)
        assert (single["contrib_n"] > 0).mean() > 0.25


@pytest.mark.parametrize("name", IT.WRAP_SCENES)
def test_sixteen_bit_positions_wrap_as_in_the_reference(name, gpu_device):
    p1, pt, _ = IT.oracle_truth(name)
    stops, aliased = IT.wrap_census(p1)
    assert int(IT.oracle(name)["ranges"][0, 1]) > 65536 and len(IT.points(name)) >= 4000
    pix_keep = IT.kept_points_per_pixel(p1, pt)
    print("%s: kept points in pixels that stop at a wrapped id %d, that accept an aliased id %d" % (name, pix_keep[stops].sum(), pix_keep[aliased].sum()))
    assert pix_keep[stops].sum() >= 50                              # both kinds of pixel hold kept points
    if name == "wrap_alias":
        assert pix_keep[aliased].sum() >= 50
    a, b = _check(name, groups=("alpha_integrated",), parity=False)      # (256 pixels: the parity gate's 99.9 % is every pixel)
    assert np.array_equal(a["ai"].view(np.uint32), b["ai"].view(np.uint32))
    _assert_same_bits(name, a, b)


@pytest.mark.parametrize("name", IT.SHORT_SCENES)
def test_short_contributor_lists(name, gpu_device):
    p1, pt, _ = IT.oracle_truth(name)
    k = int(name[5:])
    lens = np.array([len(c) for c in p1["contrib"]])
    assert set(lens) == {k, k + 1}
    a, b = _check(name)
    _assert_same_bits(name, a, b)
    if k == 0:       # an in-image point of a pixel with no contributor: exactly 0 and the background, not the fill 1.0
        empty = pt["ok"] & (lens[np.maximum(pt["pix"], 0)] == 0)
        assert empty.sum() >= 100
        bg = IT.scene(name)["bg"].numpy()
        for h in (a, b):
            assert (h["ai"][empty] == 0.0).all() and np.array_equal(h["ci"][empty], np.broadcast_to(bg, (int(empty.sum()), 3)))


def _bits(t):
    return t.view(torch.int32)


def test_alpha_min_is_torch_min_on_every_point(gpu_device):
    from f3dgaus_amd.diff_gof_rasterization import integrate_points
    sc = IT.scene("I1")
    pts_a = torch.from_numpy(np.array(IT.points("I1"))).to(gpu_device)
    pts_b = torch.from_numpy(make_points(sc, len(pts_a), seed=5)).to(gpu_device)
    prep = _prepare(sc, gpu_device, len(pts_a))
    ai_a, _ = integrate_points(prep, pts_a)
    ai_b, _ = integrate_points(prep, pts_b)
    gen = torch.Generator().manual_seed(11)
    before = torch.rand(len(pts_a), generator=gen)
    kind = torch.randint(0, 8, (len(pts_a),), generator=gen)
    before[kind == 0] = float("nan"); before[kind == 1] = 2.0; before[kind == 2] = float("inf"); before[kind == 3] = 1.0; before[kind == 4] = 0.0
    before = before.to(gpu_device)
    rejected = ai_a == 1.0
    for value in (2.0, float("inf")):          # rejected points whose buffer is above the fill 1.0, and accepted ones
        assert (rejected & (before == value)).sum() >= 10 and (~rejected & (before == value)).sum() >= 10
    assert (rejected & before.isnan()).sum() >= 10 and (~rejected & before.isnan()).sum() >= 10
    expect = torch.min(before, ai_a)
    assert expect.isnan().sum() == before.isnan().sum() and not ai_a.isnan().any()
    buf = before.clone()
    ai2, ci2 = integrate_points(prep, pts_a, alpha_min=buf)
    assert torch.equal(_bits(buf), _bits(expect)) and torch.equal(ai2, ai_a)
    quiet = before.clone()
    assert integrate_points(prep, pts_a, alpha_min=quiet, want_outputs=False) == (None, None)
    assert torch.equal(_bits(quiet), _bits(expect))
    integrate_points(prep, pts_b, alpha_min=buf, want_outputs=False)          # a second point set accumulates
    assert torch.equal(_bits(buf), _bits(torch.min(expect, ai_b)))
    assert (buf[~before.isnan()] <= 1.0).all()
