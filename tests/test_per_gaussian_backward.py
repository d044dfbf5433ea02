"""CPU side of the per-Gaussian backward tests: the oracle on the fixtures of tests/per_gaussian_fixtures.py against the float64
chain rule fed with the oracle's OWN per-view dL_dview2gaussian / dL_dcolor, and the conditions the GPU test
(tests/test_per_gaussian_backward_gpu.py) relies on -- its bars are multiples of the oracle's error on these scenes, so a scene that
drifts towards the ill-conditioned regime has to fail here and not loosen them.

Oracle, max error / max gradient (mean / rot / scale / sh), measured on the CPU:
    oblique_deg1      4.9e-6  3.7e-5  3.7e-4  7e-8          odd_deg3        6.0e-6  5.9e-5  1.0e-4  9e-8
    odd_deg1_of_16    2.1e-6  6.1e-5  2.6e-4  7e-8          precomp         1.2e-5  9.5e-4  1.8e-4  -
    three_views       8.5e-6  1.3e-4  3.1e-4  1.3e-7
    three_views_seed1 7.0e-6  2.5e-4  3.3e-3  1.2e-7        odd_deg1_of_16_stretched  2.3e-6  4.5e-5  2.0e-4  5e-8
The oracle is deterministic, but its forward goes through the C library's expf, whose last bit depends on the CPU: on another host the
per-view dL_dview2gaussian differ in the last bits and the figures above move, because max error / max gradient is the maximum of a
heavy-tailed sample (a few Gaussians whose terms are 1e3 .. 1e4 times the scene's largest gradient carry it). On the host of the MI355X the
same scenes gave, worst first:  precomp 2.8e-5 / 9.5e-4 / 2.8e-3,  three_views_seed1 6.8e-6 / 7.9e-4 / 1.2e-3,  oblique_deg1 3.9e-6 /
3.1e-5 / 7.6e-4; scaling the cotangent by 1 + 3e-7 k (k = 0..11) here moves precomp over 2.5e-6..5.0e-5 / 4.1e-5..1.4e-3 / 1.8e-4..9.4e-3
and the other scenes by factors of 1.6 to 7.
The caps are 1.5 to 3 times the worst figure over both hosts and the scenes' first table (1.2e-5 / 9.5e-4 / 1.5e-3 there):
6e-5 / 2e-3 / 5e-3 -- the first was 2e-5 before the second host's 2.8e-5 was known; the other two are unchanged."""
import numpy as np
import pytest

import per_gaussian_fixtures as F
from grad_truth import per_gaussian_truth_views

CAPS = dict(dL_dmean3D=6e-5, dL_drot=2e-3, dL_dscale=5e-3)


@pytest.mark.parametrize("name", F.FIXTURES + F.EXTRA)
def test_oracle_conditioning_bound(name):
    ref = F.oracle_reference(name)
    for k in F.GROUPS:
        med, p99, mx = ref["K"][k]
        print(f"{name} {k}: oracle-vs-fp64 {ref['e_o'][k]:.2e}  K median {med:.2f} p99 {p99:.2f} max {mx:.1f}")
        assert ref["e_o"][k] <= CAPS[k], (name, k, ref["e_o"][k])
        assert np.isfinite(mx)
    if F.scene(name)["shs"] is not None:
        print(f"{name} dL_dsh: oracle-vs-fp64 {ref['e_o']['dL_dsh']:.2e}")
        assert ref["e_o"]["dL_dsh"] <= 16 * F.EPS


@pytest.mark.parametrize("name", [n for n in F.FIXTURES + F.EXTRA if n != "precomp"])
def test_visible_gaussians_with_a_clamped_channel(name):
    ref = F.oracle_reference(name)
    n = int((ref["clamped"].any(-1) & (ref["radii"] > 0)).sum())
    unclamped = int((~ref["clamped"].any(-1) & (ref["radii"] > 0)).sum())
    assert n >= 50 and unclamped >= 50, (name, n, unclamped)     # (64 .. 298 clamped (view, Gaussian) pairs on these scenes: both sides of the mask)


@pytest.mark.parametrize("name", ["three_views", "three_views_seed1"])
def test_partial_visibility(name):
    vis = F.oracle_reference(name)["radii"] > 0
    partial, hidden = vis.any(0) & ~vis.all(0), ~vis.any(0)
    print(f"{name}: {int(partial.sum())} of {vis.shape[1]} Gaussians seen by some views only, {int(hidden.sum())} by none")
    assert partial.sum() >= 0.1 * vis.shape[1] and hidden.sum() > 0 and vis.all(0).sum() > 0


def test_the_stretched_one_view_scene_has_hidden_gaussians():
    seen = F.oracle_reference("odd_deg1_of_16_stretched")["seen"]
    assert 20 <= (~seen).sum() <= seen.size // 2


@pytest.mark.parametrize("name", F.FIXTURES)
def test_single_input_sensitivity(name):
    """Each column of dL_dview2gaussian alone moves dL_drot and dL_dscale (columns 6..9 also dL_dmean3D; 0..5 are the gradient of
    Sigma, which does not depend on the mean) by at least the maximum of the net gradient: a wrong or missing term in any of them is
    far above the error bars, which are 1e-5 .. 5e-3 of that maximum."""
    ref, sc = F.oracle_reference(name), F.scene(name)
    V = ref["radii"].shape[0]
    net = {k: np.abs(ref["truth"][k]).max() for k in F.GROUPS}
    worst = np.inf
    for c in range(10):
        dv = np.zeros_like(ref["dL_dview2gaussian"])
        dv[..., c] = ref["dL_dview2gaussian"][..., c]
        part = per_gaussian_truth_views(sc, range(V), ref["radii"], dv, np.zeros_like(ref["dL_dcolor"]))
        for k in F.GROUPS:
            ratio = np.abs(part[k]).max() / net[k]
            if k == "dL_dmean3D" and c < 6:
                assert ratio == 0.0
                continue
            worst = min(worst, ratio)
            assert ratio >= 1.0, (name, k, c, ratio)
    print(f"{name}: smallest single-input contribution / max|net gradient| = {worst:.1f}")


def test_inactive_sh_coefficients_are_exactly_zero():
    for name in ("odd_deg1_of_16", "odd_deg1_of_16_stretched"):
        ref = F.oracle_reference(name)
        assert F.scene(name)["shs"].shape[1] == 16 and F.scene(name)["sh_degree"] == 1
        assert not ref["g"]["dL_dsh"][:, 4:].any() and not ref["truth"]["dL_dsh"][:, 4:].any()
        assert ref["g"]["dL_dsh"][:, :4].any()


def test_views_truth_is_the_sum_of_the_one_view_truths_and_sets_are_separate():
    """per_gaussian_truth_views against per_gaussian_truth view by view, and the two-set form against each set alone; the ten
    single-column parts and the colour part add up to the truth, so A >= |truth| element by element."""
    from grad_truth import per_gaussian_truth
    a, b = F.oracle_reference("three_views"), F.oracle_reference("three_views_seed1")
    sa, sb = F.scene("three_views"), F.scene("three_views_seed1")
    one = [per_gaussian_truth(sa, v, a["radii"][v], a["dL_dview2gaussian"][v], a["dL_dcolor"][v]) for v in range(3)]
    for k in F.GROUPS + ("dL_dsh",):
        assert F.rel(a["truth"][k], sum(o[k] for o in one)) <= 1e-13, k
        assert (a["A"][k] >= np.abs(a["truth"][k]) * (1 - 1e-12)).all(), k
    both = dict(sa)
    for k in ("means3D", "scales", "rotations", "shs"):
        both[k] = np.concatenate([np.asarray(sa[k]), np.asarray(sb[k])], 0)
    cat = lambda k: np.concatenate([a[k], b[k]], 0)
    t2 = per_gaussian_truth_views(both, [0, 1, 2, 0, 1, 2], cat("radii"), cat("dL_dview2gaussian"), cat("dL_dcolor"), n_sets=2)
    for k in F.GROUPS + ("dL_dsh",):
        assert np.array_equal(t2[k][:900], a["truth"][k]) and np.array_equal(t2[k][900:], b["truth"][k]), k
