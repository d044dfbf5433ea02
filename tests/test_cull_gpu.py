"""The projection's own conservative culling data, pair by pair and pixel by pixel, against the plain references of tests/cull_truth.py
(whose conditions are held on the CPU by tests/test_cull_truth.py).

preprocess_kernel writes the reference's values (held bit-exact to the oracle by tests/test_raster_forward_gpu.py) and this build's own:
the pre-test constant K (record slot 11), the conservative ellipse (plane `cull`, c in record slot 15), the tile rectangle after tile
culling with the half-tile hints, the small path's chunk boxes. Every later stage trusts them to drop only work whose alpha is certainly
below 1/255. Here each is exported (f3dg_debug_export_cull) and held, on the call's own view2gaussian and opacity -- asserted bit-equal to
the oracle's --, to
  a  conservative: every position of S+ (cull_truth.reach: where a faithful implementation of the reference can blend the Gaussian) has
     ellipse_value64 <= 1 - delta, delta the forward error bound of the consumers' float32 evaluation;
  b  not wider than designed: class, centre and coefficients of the float64 restatement on the well-conditioned pairs;
  c  the pre-test never fires on S+, K two-sided against K0 (1 - 5e-7), the special values;
  d  the tile rectangle holds every tile with a position of S+, lies in the reference's, and is the box of the exported ellipse two-sided;
  e  a hint bit is set only if its half-tile holds no position of S+, and is set whenever the inflated box clears the half;
  f  the chunk boxes are the exact unions;
  g  every branch is exercised (minimum counts: conditions on the scenes, met by the reference alone on the CPU).
Each assertion reports the first offending (view, Gaussian, position)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import cull_truth as cq
import f3dgaus_amd as f3d
from f3dgaus_amd import _lib

pytestmark = pytest.mark.gpu

SCENES = cq.SCENE_NAMES


def _dev(t, device):
    return None if t is None else t.to(device)


@functools.lru_cache(maxsize=None)
def run(name, save_aux=True, tile_cull=True, small_path=False):
    """One rasterize_views call of a scene and what its workspace holds: K, c, view2gaussian, opacity (records), the ellipse plane, the
    rectangles, radii, num_rendered; tiles_touched of a SAVE_AUX call; the chunk boxes (or the error code) as `chunk`."""
    sc = cq.scene(name)
    device = torch.device("cuda:0")
    V, P, W, H = sc["viewmatrix"].shape[0], sc["P"], sc["W"], sc["H"]
    pre = "view2gaussian_precomp" in sc
    out, radii, ws = f3d.rasterize_views(
        _dev(sc["means3D"], device), _dev(sc["opacities"], device), _dev(sc["viewmatrix"], device), _dev(sc["projmatrix"], device),
        _dev(sc["campos"], device), _dev(sc["bg"], device), image_height=H, image_width=W, tanfovx=sc["tanfovx"], tanfovy=sc["tanfovy"],
        sh=_dev(sc["shs"], device), colors_precomp=_dev(sc["colors_precomp"], device), scales=None if pre else _dev(sc["scales"], device),
        rotations=None if pre else _dev(sc["rotations"], device), cov3Ds_precomp=_dev(sc.get("cov3Ds_precomp"), device),
        view2gaussian_precomp=_dev(sc.get("view2gaussian_precomp"), device), sh_degree=sc["sh_degree"], scale_modifier=sc["scale_modifier"],
        kernel_size=sc["kernel_size"], save_aux=save_aux, tile_cull=tile_cull, small_path=small_path)
    e = dict(rec=torch.zeros(V * P * 16, dtype=torch.float32, device=device), tiles=torch.zeros(V * P, dtype=torch.int32, device=device),
             cull=torch.zeros(V * P * 4, dtype=torch.float32, device=device), rects=torch.zeros(V * P * 2, dtype=torch.int32, device=device),
             chunk=torch.zeros(V * ((P + 63) // 64) * 2, dtype=torch.int32, device=device))
    L = _lib.lib()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    wsp = C.c_void_p(ws.buffer.data_ptr())
    p = lambda k: C.c_void_p(e[k].data_ptr())
    assert L.f3dg_debug_export(stream, wsp, P, W, H, V, ws.max_rendered, p("rec"), None, None, p("tiles") if save_aux else None,
                               *([None] * 8)) == 0
    assert L.f3dg_debug_export_cull(stream, wsp, P, W, H, V, ws.max_rendered, p("cull"), p("rects"), None) == 0
    rc_chunk = L.f3dg_debug_export_cull(stream, wsp, P, W, H, V, ws.max_rendered, None, None, p("chunk"))
    torch.cuda.synchronize()
    rec = e["rec"].cpu().numpy().reshape(V, P, 16)
    rects = e["rects"].cpu().numpy().view(np.uint32).reshape(V, P, 2).astype(np.int64)
    x0, x1 = rects[:, :, 0] & cq.COORD, (rects[:, :, 0] >> 16) & cq.COORD
    y0, y1 = rects[:, :, 1] & cq.COORD, (rects[:, :, 1] >> 16) & cq.COORD
    return dict(v2g=rec[:, :, :10], opac=rec[:, :, 10], K=rec[:, :, 11], c=rec[:, :, 15], cull=e["cull"].cpu().numpy().reshape(V, P, 4),
                rects=rects, x0=x0, x1=x1, y0=y0, y1=y1, area=(x1 - x0) * (y1 - y0),
                hints=np.stack([(rects[:, :, 0] & cq.SKIP_LO) != 0, (rects[:, :, 0] & cq.SKIP_HI) != 0,
                                (rects[:, :, 1] & cq.SKIP_LO) != 0, (rects[:, :, 1] & cq.SKIP_HI) != 0], 2),
                radii=radii.cpu().numpy(), num_rendered=int(ws.num_rendered), tiles=e["tiles"].cpu().numpy().view(np.uint32).reshape(V, P),
                chunk=e["chunk"].cpu().numpy().view(np.uint32).reshape(V, -1, 2).astype(np.int64), rc_chunk=rc_chunk,
                out=out.cpu().numpy())


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def assert_inputs_are_the_oracles(name, h, oracle_name=None):
    """view2gaussian and opacity * coef of the call's own records, bit for bit the oracle's on the visible pairs (as
    compositing_truth.assert_inputs_are_the_oracles): kernel and truth then share their inputs."""
    for v in range(cq.n_views(name)):
        o = cq.oracle(oracle_name or name, v)
        vis = o["radii"] > 0
        assert np.array_equal(h["radii"][v] > 0, vis), (name, v, "visibility")
        assert np.array_equal(_bits(h["v2g"][v][vis]), _bits(o["view2gaussian"][vis])), (name, v, "view2gaussian")
        assert np.array_equal(_bits(h["opac"][v][vis]), _bits(o["opac"][vis])), (name, v, "opacity * coef")


@pytest.mark.parametrize("name", SCENES)
def test_planes_do_not_depend_on_the_call(gpu_device, name):
    """save_aux on / off: the planes are identical on the listed pairs (an inference call writes only those; rects always). tile_cull on /
    off: the ellipse and K are identical, only rects differs; without tile culling the coordinates are exactly the oracle's rectangle.
    tiles_touched is the rectangle's area and num_rendered the sum of the areas, in every call."""
    full = run(name, True, True)
    assert_inputs_are_the_oracles(name, full)
    for save_aux in (True, False):
        for tile_cull in (True, False):
            h = run(name, save_aux, tile_cull)
            listed = h["area"] > 0
            assert np.array_equal(h["radii"], full["radii"])
            for k in ("cull", "c", "K", "v2g", "opac"):
                assert np.array_equal(_bits(h[k][listed]), _bits(full[k][listed])), (name, save_aux, tile_cull, k)
            assert h["num_rendered"] == int(h["area"].sum()), (name, save_aux, tile_cull)
            if save_aux:
                assert np.array_equal(h["tiles"].astype(np.int64), h["area"]), (name, tile_cull, "tiles_touched")
            assert np.array_equal(h["rects"], run(name, True, tile_cull)["rects"]), (name, save_aux, tile_cull, "rects")
            if not tile_cull:
                for v in range(cq.n_views(name)):
                    o = cq.oracle(name, v)
                    x0, x1, y0, y1 = o["rect"]
                    vis = o["radii"] > 0
                    for k, ref in (("x0", x0), ("x1", x1), ("y0", y0), ("y1", y1)):
                        assert np.array_equal(h[k][v][vis], ref[vis]), (name, v, k, "the oracle's rectangle")
                    assert np.all(h["area"][v][~vis] == 0), (name, v, "an invisible pair has a rectangle")
                assert h["num_rendered"] == sum(cq.oracle(name, v)["num_rendered"] for v in range(cq.n_views(name)))


@functools.lru_cache(maxsize=None)
def position_checks(name):
    """ONE walk over the positions of S+ of every visible pair (a scene has up to 2e7): the first position the exported ellipse does not
    certainly cover (a), the first position where the pre-test fires (c), and how many positions have ellipse_value64 > 0.9 (g)."""
    h = run(name, True, True)
    uncovered, skipped, near, n = None, None, 0, 0
    for v in range(cq.n_views(name)):
        for g, x, y, AA, bh in cq.walk(name, v):
            n += len(x)
            bad, m = cq.first_uncovered(h["cull"][v, g], h["c"][v, g], (x, y))
            near += m
            if bad is not None and uncovered is None:
                uncovered = (v, g) + bad
            s = cq.pretest_skips(h["K"][v, g], AA, bh)
            if s.any() and skipped is None:
                i = int(np.nonzero(s)[0][0])
                skipped = (v, g, float(x[i]), float(y[i]), float(h["K"][v, g]))
    return dict(uncovered=uncovered, skipped=skipped, near=near, positions=n)


@pytest.mark.parametrize("name", SCENES)
def test_ellipse_is_conservative(gpu_device, name):
    """(a) Every position of S+ -- all pixel centres (compositing's alpha) and the quarter-pixel lattice over the closed image rectangle,
    which holds every ray position of integrate_pass1_rays_kernel (integrate's alpha) -- has ellipse_value64 <= 1 - delta under the
    exported float32 ellipse. (g) At least 100 of them lie in its outer tenth: the edge is exercised."""
    r = position_checks(name)
    print(name, r)
    assert r["uncovered"] is None, "%s: (view, Gaussian, x, y, E64) %r is in S+ but not certainly inside the exported ellipse" % (name, r["uncovered"])
    assert r["near"] >= 100, (name, r["near"])


@pytest.mark.parametrize("name", SCENES)
def test_pretest_never_fires_where_the_reference_blends(gpu_device, name):
    """(c) fl(b b) < fl(K a) -- float32, as the compositing loops and ray_eval compute it -- is false at every position of S+ (both alpha
    variants). Two-sided: |K - K0 (1 - 5e-7)| <= 2^-23 |K0| + 4e-6 with K0 = C + 2 thr from a float64 thr (the float32 narrowing of K and
    the hardware log2 behind thr). K = +inf exactly for opacity <= 0, K = 0 for NaN opacity and wherever K0 <= 0."""
    r = position_checks(name)
    assert r["skipped"] is None, "%s: (view, Gaussian, x, y, K) %r: the pre-test skips a position of S+" % (name, r["skipped"])
    h = run(name, True, True)
    for v in range(cq.n_views(name)):
        o = cq.oracle(name, v)
        vis = o["radii"] > 0
        K, op = h["K"][v].astype(np.float64), o["opac"]
        K0 = cq.pretest_k0(o["view2gaussian"], op)
        with np.errstate(all="ignore"):
            want = np.where(K0 > 0, K0 * (1.0 - 5e-7), 0.0)
            ok = np.where(np.isposinf(K0), np.isposinf(K), np.where(K0 > 0, np.abs(K - want) <= 2.0 ** -23 * np.abs(K0) + 4e-6, K == 0.0))
        # (a K0 within the tolerance of 0 may come out on either side of the clamp)
        ok |= np.isfinite(K0) & (np.abs(K0) <= 4e-6) & (np.abs(K) <= 8e-6)
        bad = np.nonzero(vis & ~ok)[0]
        assert bad.size == 0, (name, v, int(bad[0]), float(K[bad[0]]), float(K0[bad[0]]), float(op[bad[0]]))
        assert np.all(np.isposinf(K[vis & (op <= 0)])) and np.all(K[vis & np.isnan(op)] == 0.0), (name, v)


# minimum counts of exercised branches per scene (g): conditions on the scenes, met by the restatement alone (tests/test_cull_truth.py)
MIN_COUNTS = {"needles": dict(fat=20), "close": dict(everything=10, never=1), "opacity_edges": dict(everything=10, never=1),
              "mixed": dict(culled=50, hint=50)}


@pytest.mark.parametrize("name", SCENES)
def test_ellipse_is_not_wider_than_designed(gpu_device, name):
    """(b) On the well-conditioned pairs (cull_truth.well_conditioned; at most 5 % of a scene's visible pairs may fail that, opacity_edges
    exempt) the exported ellipse is the float64 restatement: the same outcome class, the centre within 2^-23 max(1, |px|) + 1e-6 px,
    a, b, c within cull_truth.coef_rtol -- the kernel's documented approximations (v_rcp_f64, the float32 roots rounded up, the float32
    narrowing; for a fattened pair times its flatness), derived there. A regression that sends
    pairs down an early return ("everything") or widens a margin fails here. (g) Branch counts of the kernel's own classes."""
    h = run(name, True, True)
    counts = dict(fat=0, everything=0, never=0)
    for v in range(cq.n_views(name)):
        t = cq.truth(name, v)
        r, good, vis = t["restated"], t["good"], t["vis"]
        if name != "opacity_edges":
            assert (~good[vis]).mean() <= 0.05, (name, v, "ill-conditioned share", float((~good[vis]).mean()))
        cls = cq.classify(h["cull"][v], h["c"][v])
        sel = vis & good
        bad = np.nonzero(sel & (cls != r["cls"]))[0]
        assert bad.size == 0, "%s view %d Gaussian %d: class %d, restated %d" % (name, v, bad[0], cls[bad[0]], r["cls"][bad[0]])
        e = sel & (cls == cq.ELLIPSE)
        cull, c = h["cull"][v].astype(np.float64), h["c"][v].astype(np.float64)
        with np.errstate(all="ignore"):
            for k, got, ref in (("cx", cull[:, 0], r["cx"]), ("cy", cull[:, 1], r["cy"])):
                tol = 2.0 ** -23 * np.maximum(1.0, np.abs(ref)) + 1e-6
                bad = np.nonzero(e & ~(np.abs(got - ref) <= tol))[0]
                assert bad.size == 0, (name, v, int(bad[0]), k, float(got[bad[0]]), float(ref[bad[0]]), float(tol[bad[0]]))
            rt = cq.coef_rtol(r)
            for k, got, ref, scale in (("a", cull[:, 2], r["a"], r["a"]), ("b", cull[:, 3], r["b"], cq.b_scale(r)), ("c", c, r["c"], r["c"])):
                bad = np.nonzero(e & ~(np.abs(got - ref) <= rt * scale))[0]
                assert bad.size == 0, (name, v, int(bad[0]), k, float(got[bad[0]]), float(ref[bad[0]]), float(abs(got[bad[0]] - ref[bad[0]]) / scale[bad[0]]), float(rt[bad[0]]))
        counts["fat"] += int((vis & r["fat"] & (cls == cq.ELLIPSE)).sum())
        counts["everything"] += int((vis & (cls == cq.EVERYTHING)).sum())
        counts["never"] += int((vis & (cls == cq.NEVER)).sum())
    print(name, counts)
    for k, n in MIN_COUNTS.get(name, {}).items():
        if k in counts:
            assert counts[k] >= n, (name, k, counts[k])


def _rect_checks(name, tile_cull):
    """(d), (e) of one call. Returns the number of visible pairs with a culled tile and with each hint bit."""
    sc = cq.scene(name)
    gx, gy = (sc["W"] + 15) // 16, (sc["H"] + 15) // 16
    h = run(name, True, tile_cull)
    n_culled, n_hint = 0, np.zeros(4, np.int64)
    for v in range(cq.n_views(name)):
        o, t = cq.oracle(name, v), cq.truth(name, v)
        vis, cen = t["vis"], t["centres"]
        rx0, rx1, ry0, ry1 = o["rect"]
        x0, x1, y0, y1 = h["x0"][v], h["x1"][v], h["y0"][v], h["y1"][v]
        first = lambda m: int(np.nonzero(m)[0][0])
        # inside the reference's rectangle; empty rectangles are (0, 0)
        m = vis & (h["area"][v] > 0) & ~((x0 >= rx0) & (x1 <= rx1) & (y0 >= ry0) & (y1 <= ry1))
        assert not m.any(), (name, v, first(m), "outside the reference rectangle")
        m = (h["area"][v] == 0) & ((h["rects"][v] != 0).any(1))
        assert not m.any(), (name, v, first(m), "an empty rectangle is not 0, 0")
        # every tile that holds a position of S+ (pixel centres, compositing's alpha)
        has = vis & (cen[:, 4] > 0)
        tx0, tx1, ty0, ty1 = (cen[:, 0] // 16).astype(np.int64), (cen[:, 1] // 16).astype(np.int64), (cen[:, 2] // 16).astype(np.int64), (cen[:, 3] // 16).astype(np.int64)
        m = has & ~((x0 <= tx0) & (tx1 < x1) & (y0 <= ty0) & (ty1 < y1))
        assert not m.any(), "%s view %d Gaussian %d: S+ spans x %g..%g y %g..%g, rectangle x %d..%d y %d..%d" % (
            (name, v, first(m)) + tuple(cen[first(m), :4]) + (x0[first(m)], x1[first(m)], y0[first(m)], y1[first(m)]))
        # two-sided against the float64 box of the exported ellipse
        hx, hy = cq.box_of(h["cull"][v], h["c"][v])
        cx, cy = h["cull"][v][:, 0].astype(np.float64), h["cull"][v][:, 1].astype(np.float64)
        within = ((rx0, rx1), (ry0, ry1))
        if tile_cull:
            ix = cq.tiles_of(cx, hx, (0.0, 0.0), gx, within[0]); iy = cq.tiles_of(cy, hy, (0.0, 0.0), gy, within[1])
            ox = cq.tiles_of(cx, hx, (cq.BOX_REL, cq.BOX_ABS), gx, within[0]); oy = cq.tiles_of(cy, hy, (cq.BOX_REL, cq.BOX_ABS), gy, within[1])
            inner = (ix[1] > ix[0]) & (iy[1] > iy[0])
            outer = (ox[1] > ox[0]) & (oy[1] > oy[0])
            m = vis & inner & ~((x0 <= ix[0]) & (ix[1] <= x1) & (y0 <= iy[0]) & (iy[1] <= y1))
            assert not m.any(), (name, v, first(m), "misses a tile the float64 box reaches")
            m = vis & (h["area"][v] > 0) & ~(outer & (ox[0] <= x0) & (x1 <= ox[1]) & (oy[0] <= y0) & (y1 <= oy[1]))
            assert not m.any(), (name, v, first(m), "holds a tile the inflated box misses")
            n_culled += int((vis & (h["area"][v] < (rx1 - rx0) * (ry1 - ry0))).sum())
        # hints: relative to the call's own rectangle
        listed = vis & (h["area"][v] > 0)
        finite = np.isfinite(hx)
        for i, (lo, hi, ctr, hh, smin, smax) in enumerate(((x0, x1, cx, hx, cen[:, 0], cen[:, 1]), (y0, y1, cy, hy, cen[:, 2], cen[:, 3]))):
            bit_lo, bit_hi = h["hints"][v][:, 2 * i], h["hints"][v][:, 2 * i + 1]
            m = ~listed & (bit_lo | bit_hi)
            assert not m.any(), (name, v, first(m), "hint on an unlisted pair")
            m = listed & has & bit_lo & (smin < 16 * lo + 8)
            assert not m.any(), (name, v, first(m), "axis %d: SKIP_LO, but S+ begins at %g in tile %d" % (i, smin[first(m)], lo[first(m)]))
            m = listed & has & bit_hi & (smax > 16 * (hi - 1) + 7)
            assert not m.any(), (name, v, first(m), "axis %d: SKIP_HI, but S+ ends at %g" % (i, smax[first(m)]))
            with np.errstate(all="ignore"):
                ext = hh * (1.0 + cq.BOX_REL) + cq.BOX_ABS
                m = listed & finite & (ctr - ext > 16.0 * lo + 7.0) & ~bit_lo
                assert not m.any(), (name, v, first(m), "axis %d: the inflated box clears the first half, SKIP_LO is not set" % i)
                m = listed & finite & (ctr + ext < 16.0 * (hi - 1) + 8.0) & ~bit_hi
                assert not m.any(), (name, v, first(m), "axis %d: the inflated box clears the last half, SKIP_HI is not set" % i)
                # and a set bit is the box's: the exact box must clear the half
                m = listed & bit_lo & ~(finite & (ctr - hh > 16.0 * lo + 7.0))
                assert not m.any(), (name, v, first(m), "axis %d: SKIP_LO, but the float64 box reaches the first half" % i)
                m = listed & bit_hi & ~(finite & (ctr + hh < 16.0 * (hi - 1) + 8.0))
                assert not m.any(), (name, v, first(m), "axis %d: SKIP_HI, but the float64 box reaches the last half" % i)
            n_hint[2 * i] += int((listed & bit_lo).sum()); n_hint[2 * i + 1] += int((listed & bit_hi).sum())
    return n_culled, n_hint


@pytest.mark.parametrize("name", SCENES)
def test_tile_rectangle_and_hints(gpu_device, name):
    """(d) Under tile culling the rectangle holds every tile with a position of S+ inside the reference rectangle, lies inside that
    rectangle, holds every tile the float64 box of the exported ellipse reaches and none that the box misses after inflation by 0.1 % +
    4e-3 px (twice the kernel's 1.0005 / 2e-3 px). (e) A set SKIP_LO / SKIP_HI bit means no position of S+ in that half of the first / last
    tile column or row, and the bit is set whenever the inflated box clears the half -- with tile culling and without. (g) mixed: at least 50
    pairs with a culled tile and with each hint bit."""
    culled, hints = _rect_checks(name, True)
    _, hints_off = _rect_checks(name, False)
    print(name, "pairs with a culled tile", culled, "hint bits", hints.tolist(), "without tile culling", hints_off.tolist())
    need = MIN_COUNTS.get(name, {})
    if "culled" in need:
        assert culled >= need["culled"] and hints.min() >= need["hint"], (name, culled, hints.tolist())


def test_precomputed_view2gaussian_is_never_culled(gpu_device):
    """precomp: the mixed Gaussians passed as cov3Ds_precomp + view2gaussian_precomp. have_scale is false, so every ellipse is "everything",
    no tile is culled (the rectangle is the oracle's) and no hint is set; K is still the pre-test constant of its record."""
    full = run("mixed", True, True)
    for save_aux in (True, False):
        h = run("precomp", save_aux, True)
        assert_inputs_are_the_oracles("precomp", h, "mixed")
        listed = h["area"] > 0
        assert np.all(cq.classify(h["cull"][listed], h["c"][listed]) == cq.EVERYTHING)
        assert not h["hints"].any()
        for v in range(cq.n_views("mixed")):
            o = cq.oracle("mixed", v)
            vis = o["radii"] > 0
            for k, ref in zip(("x0", "x1", "y0", "y1"), o["rect"]):
                assert np.array_equal(h[k][v][vis], ref[vis]), (v, k)
        assert h["num_rendered"] == sum(cq.oracle("mixed", v)["num_rendered"] for v in range(2))
        assert np.array_equal(_bits(h["K"][listed]), _bits(full["K"][listed]))


@pytest.mark.parametrize("P", (37, 130))
def test_chunk_boxes(gpu_device, P):
    """(f) Small-path calls: every full wave's box is the exact union of its 64 rectangles -- hint bits masked out, invisible pairs ignored
    --, the last partial wave holds "everything"; a call that did not take the small path answers F3DG_ERR_STATE."""
    name = "tiny_P%d" % P
    g = run(name, False, True, small_path=False)
    assert g["rc_chunk"] == _lib.ERR_STATE
    for save_aux in (False, True):
        h = run(name, save_aux, True, small_path=True)
        assert h["rc_chunk"] == 0, "the call did not take the small path"
        assert np.array_equal(h["rects"], g["rects"])
        n_chunks = (P + 63) // 64
        assert h["chunk"].shape[1] == n_chunks
        for v in range(h["chunk"].shape[0]):
            for k in range(n_chunks):
                bx = h["chunk"][v, k]
                got = (bx[0] & cq.COORD, (bx[0] >> 16) & cq.COORD, bx[1] & cq.COORD, (bx[1] >> 16) & cq.COORD)
                assert (bx[0] & (cq.SKIP_LO | cq.SKIP_HI)) == 0 and (bx[1] & (cq.SKIP_LO | cq.SKIP_HI)) == 0
                if 64 * (k + 1) > P:
                    assert got == (0, cq.COORD, 0, cq.COORD), (P, v, k, got)
                    continue
                s = slice(64 * k, 64 * k + 64)
                vis = h["area"][v][s] > 0
                want = ((h["x0"][v][s][vis].min(), h["x1"][v][s][vis].max(), h["y0"][v][s][vis].min(), h["y1"][v][s][vis].max()) if vis.any()
                        else (cq.COORD, 0, cq.COORD, 0))
                assert got == tuple(int(w) for w in want), (P, v, k, got, want)
