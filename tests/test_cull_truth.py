"""The references of tests/cull_truth.py, held on the CPU before tests/test_cull_gpu.py relies on them:
  - `reach` brackets the ORACLE: on single-Gaussian scenes the pixels the oracle blends contain S- and lie in S+ (inside the oracle's tile
    rectangle), so the float32 emulation of normal / AA / BB / power is the oracle's;
  - the float64 restatement of the conservative ellipse is conservative ON ITS OWN: every position of S+ of the GPU module's scenes has
    ellipse_value64 <= 1 - delta under the restated ellipse ("the formulas are wrong" is told apart from "the kernel mis-implements them");
  - the conditions on the scenes hold for the reference alone: at most 5 % ill-conditioned pairs, the minimum counts of exercised branches."""
import functools
import math

import numpy as np
import pytest
import torch

import compositing_truth as ct
import cull_truth as cq
import helpers

KINDS = ("isotropic", "needle", "low_opacity", "large", "off_screen", "filter", "modifier", "isotropic_oblique")


def single(kind, i):
    """One Gaussian at 64 x 48."""
    kw = dict(P=1, res=(64, 48), s0=0.05, seed=100 + i, view="oblique" if kind == "isotropic_oblique" or i % 2 else "canonical")
    if kind == "filter":
        kw["kernel_size"] = 0.3
    if kind == "modifier":
        kw["scale_modifier"] = 0.5
    sc = helpers.make_scene(**kw)
    gen = torch.Generator().manual_seed(200 + i)
    r = lambda lo, hi: float(torch.rand(1, generator=gen)) * (hi - lo) + lo
    sc["opacities"] = torch.tensor([[r(0.3, 0.95)]])
    if kind in ("isotropic", "isotropic_oblique", "filter", "modifier"):
        sc["scales"] = torch.full((1, 3), r(0.03, 0.12))
    elif kind == "needle":
        sc["scales"] = torch.tensor([[r(0.2, 0.4), 2e-3, 2e-3]])
    elif kind == "low_opacity":
        sc["scales"] = torch.full((1, 3), r(0.05, 0.15))
        sc["opacities"] = torch.tensor([[r(0.004, 0.02)]])
    elif kind == "large":
        sc["scales"] = torch.tensor([[r(0.3, 0.6), r(0.3, 0.6), r(0.05, 0.6)]])
    elif kind == "off_screen":
        sc["scales"] = torch.tensor([[r(0.25, 0.4), r(0.1, 0.3), r(0.1, 0.3)]])
        sc["means3D"] = sc["means3D"] + torch.tensor([[1.1 if i % 4 < 2 else -1.1, 0.0, 0.0]])
    return sc


@pytest.mark.parametrize("kind", KINDS)
def test_reach_brackets_the_oracle(kind):
    """Five scenes per kind (40 in all): {pixels whose alpha channel the oracle wrote} contains S- and is contained in S+, inside the oracle's
    3-sigma tile rectangle. (One Gaussian: alpha = its own min(0.99, ...) > 0 exactly where it was blended; T = 1 never stops the loop.)"""
    blended = 0
    for i in range(5):
        sc = single(kind, i)
        o = helpers.run_oracle(sc)
        W, H = sc["W"], sc["H"]
        got = np.asarray(o["out_color"])[7] != 0
        if not o["radii"][0] > 0:
            assert not got.any()
            continue
        x0, x1, y0, y1 = (int(v[0]) for v in cq.reference_rect(o["means2D"], o["radii"], W, H))
        assert int(o["tiles_touched"][0]) == (x1 - x0) * (y1 - y0)
        rect = np.zeros((H, W), bool)
        rect[16 * y0:16 * y1, 16 * x0:16 * x1] = True
        xs, ys = np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64)
        rx, ry = ct.rays(W, H, sc["tanfovx"], sc["tanfovy"])
        assert np.array_equal(cq.rays_at(xs, W, sc["tanfovx"]), rx) and np.array_equal(cq.rays_at(ys, H, sc["tanfovy"]), ry)
        _, _, sp, sm, _, _ = cq.reach(dict(view2gaussian=o["view2gaussian"], opac=o["conic_opacity"][:, 3]), W, H, sc["tanfovx"], sc["tanfovy"], (xs, ys))[0]
        assert not (got & ~rect).any()
        miss = sm & rect & ~got
        assert not miss.any(), (kind, i, "in S- but not blended", np.argwhere(miss)[0].tolist())
        extra = got & ~(sp & rect)
        assert not extra.any(), (kind, i, "blended outside S+", np.argwhere(extra)[0].tolist())
        blended += int(got.sum())
    assert blended >= 20, (kind, blended)          # the kind is exercised


@functools.lru_cache(maxsize=None)
def restated_summary(name):
    """One walk of a scene under the RESTATED ellipse: the first position of S+ it does not certainly cover, and the counts of section g."""
    sc = cq.scene(name)
    W, H = sc["W"], sc["H"]
    gx, gy = (W + 15) // 16, (H + 15) // 16
    s = dict(uncovered=None, near=0, ill=0.0, fat=0, everything=0, never=0, culled=0, hints=np.zeros(4, np.int64), positions=0)
    for v in range(cq.n_views(name)):
        t, o = cq.truth(name, v), cq.oracle(name, v)
        r, good, vis = t["restated"], t["good"], t["vis"]
        for g, x, y, _, _ in cq.walk(name, v):
            s["positions"] += len(x)
            if r["cls"][g] == cq.EVERYTHING:
                continue
            cull = (r["cx"][g], r["cy"][g], r["a"][g], r["b"][g]) if r["cls"][g] == cq.ELLIPSE else (-1e9, -1e9, 1e30, 0.0)
            bad, near = cq.first_uncovered(cull, r["c"][g] if r["cls"][g] == cq.ELLIPSE else 1e30, (x, y))
            s["near"] += near
            if bad is not None and s["uncovered"] is None:
                s["uncovered"] = (v, g) + bad
        s["ill"] = max(s["ill"], float((~good[vis]).mean()))
        s["fat"] += int((vis & r["fat"]).sum())
        s["everything"] += int((vis & (r["cls"] == cq.EVERYTHING)).sum())
        s["never"] += int((vis & (r["cls"] == cq.NEVER)).sum())
        cull = np.stack([r["cx"], r["cy"], r["a"], r["b"]], 1)
        hx, hy = cq.box_of(cull, r["c"])
        x0, x1, y0, y1 = o["rect"]
        lx, ux, slx, shx = cq.tiles_of(r["cx"], hx, (cq.BOX_REL, cq.BOX_ABS), gx, (x0, x1))
        ly, uy, sly, shy = cq.tiles_of(r["cy"], hy, (cq.BOX_REL, cq.BOX_ABS), gy, (y0, y1))
        e = vis & (r["cls"] == cq.ELLIPSE)
        s["culled"] += int((e & ((ux - lx) * (uy - ly) < (x1 - x0) * (y1 - y0))).sum())
        s["hints"] += np.array([(e & m).sum() for m in (slx, shx, sly, shy)])
    return s


@pytest.mark.parametrize("name", cq.SCENE_NAMES)
def test_restatement_is_conservative_on_its_own(name):
    """Every position of S+ has ellipse_value64 <= 1 - delta under the restated ellipse (narrowed to float32 as the record is); no pair with a
    position in S+ is restated as "never"."""
    s = restated_summary(name)
    print(name, s)
    assert s["positions"] > 0
    assert s["uncovered"] is None, (name, "(view, Gaussian, x, y, E64)", s["uncovered"])


@pytest.mark.parametrize("name", cq.SCENE_NAMES)
def test_scene_conditions_hold_for_the_reference_alone(name):
    """The caps and minimum counts the GPU module asserts are conditions on the inputs: at most 5 % ill-conditioned pairs per view
    (opacity_edges is exempt by construction), at least 100 positions of S+ in the outer tenth of the ellipse, and per scene the branches
    it was built for."""
    s = restated_summary(name)
    if name != "opacity_edges":
        assert s["ill"] <= 0.05, (name, s["ill"])
    assert s["near"] >= 100, (name, s["near"])
    if name == "needles":
        assert s["fat"] >= 20, s["fat"]
    if name in ("close", "opacity_edges"):
        assert s["everything"] >= 10 and s["never"] >= 1, (name, s["everything"], s["never"])
    if name == "mixed":
        assert s["culled"] >= 50 and s["hints"].min() >= 50, (s["culled"], s["hints"].tolist())


def test_delta_and_boxes_are_what_they_say():
    """delta bounds a float32 evaluation in the kernels' order on random ellipses and offsets (a self-check of the formula against numpy
    float32 with an emulated FMA), tiles_of places the half-tile boundaries at 16 t + 7 / 16 t + 8, box_of is the extent of the form."""
    rng = np.random.default_rng(0)
    f32 = np.float32
    fma = lambda a, b, c: (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(f32)      # one rounding (the product of two float32 is exact in float64; the sum's double rounding is 2^-53 away)
    worst = 0.0
    for _ in range(200):
        lam1, asp, th = 10.0 ** rng.uniform(-4, 1), 10.0 ** rng.uniform(0, 1.5), rng.uniform(0, math.pi)
        lam2 = lam1 / asp ** 2
        cs, sn = math.cos(th), math.sin(th)
        a, b, c = f32(lam1 * cs * cs + lam2 * sn * sn), f32(2 * (lam1 - lam2) * cs * sn), f32(lam1 * sn * sn + lam2 * cs * cs)
        cx, cy = f32(rng.uniform(-10, 2100)), f32(rng.uniform(-10, 70))
        q0x, q0y = np.floor(cx / 8) * 8 + rng.integers(-3, 4) * 8, np.floor(cy / 8) * 8 + rng.integers(-3, 4) * 8
        qs = np.arange(8, dtype=f32)
        u0, v0 = f32(q0x) - cx, f32(q0y) - cy
        dx, dy = (u0 + qs)[None, :], (v0 + qs)[:, None]
        adx = a * dx
        cdy = (c * dy) * dy
        E = fma(np.broadcast_to(dx, (8, 8)), fma(np.broadcast_to(b, (8, 8)), np.broadcast_to(dy, (8, 8)), np.broadcast_to(adx, (8, 8))), np.broadcast_to(cdy, (8, 8)))
        X, Y = np.broadcast_to(q0x + qs.astype(np.float64)[None, :], (8, 8)), np.broadcast_to(q0y + qs.astype(np.float64)[:, None], (8, 8))
        E64 = cq.ellipse_value64((cx, cy, a, b), c, X, Y)
        d = cq.delta((cx, cy, a, b), c, X, Y)
        assert np.all(np.abs(E.astype(np.float64) - E64) <= d)
        worst = max(worst, float((np.abs(E.astype(np.float64) - E64) / d).max()))
    assert worst > 0.01          # the bound is within two orders of what float32 actually does
    lo, hi, slo, shi = cq.tiles_of(np.array([23.5, 23.5, 24.5]), np.array([0.4, 0.6, 0.4]), (0.0, 0.0), 4)
    assert lo.tolist() == [1, 1, 1] and hi.tolist() == [2, 2, 2]
    assert slo.tolist() == [True, False, True] and shi.tolist() == [True, False, False]       # 23.1 > 23 | 22.9 | 24.1; 23.9 < 24 | 24.1 | 24.9
    hx, hy = cq.box_of(np.array([[0, 0, 0.25, 0.0], [0, 0, 0, 0]], np.float32), np.array([1.0, 0.0], np.float32))
    assert hx[0] == 2.0 and hy[0] == 1.0 and np.isinf(hx[1])
