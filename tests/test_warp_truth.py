"""CPU tests of the forward warp's restatement (tests/warp_truth.py): the properties the definition was chosen for, and that the fixture
keeps exercising what the GPU tests rely on. No library call."""
import pytest
import torch

import warp_truth as T


@pytest.mark.parametrize("shape", T.GPU_SHAPES)
def test_identity_view_returns_the_frame(shape):
    """Target 0 is the source camera: every live source pixel lands on itself with weight 1 (float64 rounding), a dead one leaves a hole."""
    c = T.case(shape)
    f, s = c["f"], c["s64"]
    live = T.live_map(f)
    Ws, warped, wdepth, mask = T.resolve(s)
    err_w = float((Ws[:, 0] - live.double()).abs().max())
    img = torch.where(live.unsqueeze(1), f["image"], torch.zeros(())).double()
    dep = torch.where(live, f["depth"], torch.zeros(())).double()
    # (as sums: a dead pixel collects ~1e-14 of weight from its neighbours' rounding, and its mean colour is theirs)
    err_c, err_z = float((s["Csum"][:, 0] - img).abs().max()), float((s["Zsum"][:, 0] - dep).abs().max())
    on = live.unsqueeze(1).expand_as(img)
    assert float((warped[:, 0] - img)[on].abs().max()) <= 1e-11 and float((wdepth[:, 0] - dep)[live].abs().max()) <= 1e-9
    print(f"identity {shape}: |Wsum - live| {err_w:.2e}  |warped - image| {err_c:.2e}  |depth| {err_z:.2e}")
    # rel = inverse(S) S carries ~1e-16 of float64 rounding, rounded to float32: u is an integer to ~1e-13 pixels at most
    assert err_w <= 1e-11 and err_c <= 1e-11 and err_z <= 1e-9
    assert torch.equal(mask[:, 0], live.double())
    assert int(s["count"][:, 0].max()) <= 4


@pytest.mark.parametrize("shape", T.GPU_SHAPES)
@pytest.mark.parametrize("use_valid", [True, False])
def test_float32_meets_float64_outside_the_fragile_set(shape, use_valid):
    """On non-fragile pixels the two restatements see the same contributions, so they differ by the float32 rounding of u, v and z alone:
    u is about a dozen float32 operations on magnitudes up to ~2 max(W, H), taken here as 64 ulps of max(W, H) (a margin of ~4 on the
    operation count); a contribution's weight moves by at most |du| + |dv|, its colour term by that times |c| <= 1, its depth term by
    that times z plus z's own rounding."""
    c = T.case(shape, use_valid=use_valid)
    B, V, H, W = shape
    s32, s64, keep = c["s32"], c["s64"], ~c["fragile"]
    assert c["fragile_share"] <= T.FRAGILE_CAP, c["fragile_share"]
    du = 64 * 2.0 ** -24 * max(H, W)
    n = torch.maximum(s64["count"], s32["count"]).double()          # (a neighbour of weight ~1e-7 in one precision may have weight 0 in the other)
    zmax = float(s64["Zsum"].max() / s64["Wsum"].clamp_min(1e-3).max().clamp_min(1.0)) + 10.0
    assert bool((((s32["Wsum"].double() - s64["Wsum"]).abs() <= 2 * du * n) | ~keep).all())
    assert bool((((s32["Csum"].double() - s64["Csum"]).abs() <= (2 * du * n).unsqueeze(2)) | ~keep.unsqueeze(2)).all())
    assert bool((((s32["Zsum"].double() - s64["Zsum"]).abs() <= (2 * du + 16 * 2.0 ** -24) * zmax * n) | ~keep).all())
    # and the mask: never a disagreement outside the threshold margin and the fragile set
    thr = T.DEFAULTS["threshold"]
    m32, m64 = s32["Wsum"].double() >= thr, s64["Wsum"] >= thr
    outside = keep & ((s64["Wsum"] - thr).abs() >= T.MARGIN)
    assert not bool(((m32 != m64) & outside).any())
    print(f"{shape} valid={use_valid}: fragile share {c['fragile_share']:.4f}  E_ref {c['e_ref']}  n_max {c['n_max']}")


@pytest.mark.parametrize("shape", T.GPU_SHAPES)
def test_fragile_cap_holds_for_every_gpu_case(shape):
    for use_valid, shared, C in ((True, False, 3), (False, False, 3), (True, True, 3), (True, False, 1)):
        c = T.case(shape, use_valid=use_valid, shared=shared, C=C)
        print(f"{shape} valid={use_valid} shared={shared} C={C}: fragile share {c['fragile_share']:.4f}")
        assert c["fragile_share"] <= T.FRAGILE_CAP, (shape, use_valid, shared, C, c["fragile_share"])
    assert T.case((1, 2, 16, 16), special=False)["fragile_share"] <= T.FRAGILE_CAP


def test_the_fixture_exercises_holes_and_pile_ups():
    """The closer camera magnifies (the weight of most pixels stays under the threshold), the farther one minifies (Wsum > 1), the disc
    occludes (some candidate fails a depth test), and the special pixels are there."""
    for shape in T.GPU_SHAPES[:2]:
        c = T.case(shape)
        Ws = c["s64"]["Wsum"]
        share_close = float((Ws[:, 2] >= T.DEFAULTS["threshold"]).double().mean())
        print(f"{shape}: mask share of the closer view {share_close:.3f}, max Wsum of the farther view {float(Ws[:, 3].max()):.3f}")
        assert share_close < 0.5
        assert float(Ws[:, 3].max()) > 1.0
        open_ = T.warp_sums(c["f"], torch.float64, rel=c["rel"], depth_tolerance=1e9)          # no occlusion at all
        assert int(open_["count"].sum()) > int(c["s64"]["count"].sum())
        f = c["f"]
        assert int((f["valid"] == 0).sum()) > 0 and bool(torch.isnan(f["image"]).any()) and int((f["depth"] <= 0).sum()) > 0
        assert not bool(torch.isnan(c["s64"]["Csum"]).any())                                    # a NaN behind valid = 0 reaches nothing
    # without `valid` the NaN pixels are dead by their depth: the same sums
    a, b = T.case(T.GPU_SHAPES[0]), T.case(T.GPU_SHAPES[0], use_valid=False)
    assert torch.equal(a["s64"]["Wsum"], b["s64"]["Wsum"])


def test_the_floor_is_what_keeps_the_identity_warp_whole():
    """Without the floor (occlusion_min_weight = 0) the float32 identity warp loses pixels at depth edges: a nearer neighbour whose u lands
    a rounding past an integer claims the z-buffer with a weight of ~1e-7. With the floor it returns the frame."""
    f = T.make_fixture(1, 1, 33, 37, special=False)
    rel = T.relative(f["src_world_view"], f["dst_world_views"])
    with_floor = T.warp_sums(f, torch.float32, rel=rel)
    assert float((with_floor["Wsum"] - 1).abs().max()) < 1e-4
    without = T.warp_sums(f, torch.float32, rel=rel, occlusion_min_weight=0.0)
    lost = int((without["Wsum"] < 0.5).sum())
    print("identity, float32, no floor: pixels lost", lost)
    assert lost > 0 and int((with_floor["Wsum"] < 0.5).sum()) == 0


@pytest.mark.parametrize("k", [1, 3, 5, 15])
def test_erode_is_the_max_pool_form(k):
    gen = torch.Generator().manual_seed(3)
    m = (torch.rand(2, 3, 19, 37, generator=gen) < 0.9).double()
    want = -torch.nn.functional.max_pool2d(-m, k, 1, k // 2)
    assert torch.equal(T.erode_mask(m, k), want)
    small = (torch.rand(1, 1, 3, 5, generator=gen) < 0.8).double()
    assert torch.equal(T.erode_mask(small, k), -torch.nn.functional.max_pool2d(-small, k, 1, k // 2))
