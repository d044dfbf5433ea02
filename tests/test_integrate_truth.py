"""The float64 truth of the point integration (tests/integrate_truth.py) and the conditions under which tests/test_integrate_truth_gpu.py may
use it. CPU only: the oracle against the truth on the oracle's own records and lists.

  * on every scene of the GPU module the oracle takes the truth's decisions outside the stated margins: the last contributor on every kept
    pixel, the max-depth channel to the bit, finite K statistics, and the truth to the bit where no term exists (A = 0);
  * the margins keep at least 0.85 of the pixels and 0.80 of the in-image points of the five bar scenes -- conditions, not measurements
    (the oracle's own minimum: 0.908 / 0.884); a scene that breaks a cap is to be changed, not the margin;
  * the two wrap scenes do wrap: lists longer than 65,536 entries, pixels that stop at a wrapped id and pixels that accept an aliased one;
  * the bars have teeth: alpha_integrated moved by 2e-5 relative, which the suite's absolute gate lets through, breaks them, and so does
    an integration that ignores the 16-bit wrap, on both wrap scenes;
  * the truth agrees with the independent float64 restatement of tests/test_oracle_integrate.py at that test's own tolerance."""
import numpy as np
import pytest

import integrate_truth as IT
from helpers import make_scene
from helpers_integrate import assert_integrate_parity, make_points, oracle_integrate

ALL = list(IT.SCENES) + list(IT.WRAP_SCENES) + list(IT.SHORT_SCENES)


@pytest.mark.parametrize("name", ALL)
def test_oracle_takes_the_truths_decisions(name):
    p1, pt, fig = IT.oracle_truth(name)
    o = IT.oracle(name)
    keep = p1["keep"]
    in_image = pt["ok"]
    print("%s: pixels kept %.3f, in-image points kept %.3f of %d; longest list %d, last contributor up to %d, most contributors %d"
          % (name, keep.mean(), pt["keep"][in_image].mean(), int(in_image.sum()), int((o["ranges"][:, 1].astype(np.int64) - o["ranges"][:, 0]).max()),
             int(p1["last"].max()), max(len(c) for c in p1["contrib"])))
    for g in IT.GROUPS:
        print("%s %-16s oracle K med / p99 / max  %.2f / %.2f / %.1f" % ((name, g) + tuple(fig[g])))
    assert np.array_equal(o["n_contrib"][0][keep], p1["last"][keep])
    assert np.array_equal(o["out"][6].astype(np.float64)[keep], p1["out"][6][keep])
    assert all(np.isfinite(f).all() for f in fig.values())
    failures = []
    IT.check_bars(name + " oracle", p1, pt, fig, fig, 1.0, failures, o["out"], o["final_T"][0], o["ai"], show=False)
    assert not failures, failures                      # (factor 1 against itself: what is asserted are the exact zeros)
    # the oracle rejects the points the truth rejects, and hands every other one the colour of the truth's pixel
    assert o["NI"] == int(in_image.sum())
    assert (o["ai"][~in_image] == 1.0).all() and not o["ci"][~in_image].any()
    assert np.array_equal(o["ci"][in_image], o["out"][:3].reshape(3, -1).T[pt["pix"][in_image]])


@pytest.mark.parametrize("name", list(IT.SCENES))
def test_margins_keep_most_of_a_scene(name):
    p1, pt, _ = IT.oracle_truth(name)
    assert p1["keep"].mean() >= 0.85, p1["keep"].mean()
    assert pt["ok"].sum() >= 0.5 * IT.N_POINTS[name]
    assert pt["keep"][pt["ok"]].mean() >= 0.80, pt["keep"][pt["ok"]].mean()
    assert (p1["last"] > 0).mean() > 0.25              # the scene is not empty


def test_alias_scene_wraps_both_ways():
    p1, pt, _ = IT.oracle_truth("wrap_alias")
    o = IT.oracle("wrap_alias")
    stops, aliased = IT.wrap_census(p1)
    print("list %d entries, kept %.3f, pixels that stop at a wrapped id %d, that accept an aliased id %d"
          % (int(o["ranges"][0, 1]) - int(o["ranges"][0, 0]), p1["keep"].mean(), int(stops.sum()), int(aliased.sum())))
    assert int(o["ranges"][0, 1]) - int(o["ranges"][0, 0]) > 65536
    assert p1["keep"].mean() >= 0.70
    assert stops.sum() >= 64 and aliased.sum() >= 64
    held = IT.kept_points_per_pixel(p1, pt)
    print("kept points in pixels that stop %d, that accept an aliased id %d" % (held[stops].sum(), held[aliased].sum()))
    assert len(IT.points("wrap_alias")) >= 4000 and held[stops].sum() >= 50 and held[aliased].sum() >= 50


def test_wrap_stop_scene_has_contributors_past_65535():
    p1, pt, _ = IT.oracle_truth("wrap_stop")
    stops, aliased = IT.wrap_census(p1)
    print("last contributor > 65535 on %d pixels; stop %d, aliased %d" % (int((p1["last"] > 65535).sum()), int(stops.sum()), int(aliased.sum())))
    assert (p1["last"] > 65535).sum() >= 100
    assert (IT.oracle("wrap_stop")["n_contrib"][0] > 65535).sum() >= 100
    assert len(IT.points("wrap_stop")) >= 4000 and IT.kept_points_per_pixel(p1, pt)[stops].sum() >= 50


@pytest.mark.parametrize("name", IT.SHORT_SCENES)
def test_short_scenes_have_the_list_lengths_they_are_built_for(name):
    p1, pt, _ = IT.oracle_truth(name)
    k = int(name[5:])
    lens = np.array([len(c) for c in p1["contrib"]])
    assert set(lens) == {k, k + 1}, sorted(set(lens))
    assert (lens == k).sum() >= 128 and p1["keep"].mean() >= 0.85
    for n in (k, k + 1):                               # kept points in pixels of either length
        assert (pt["keep"] & pt["ok"] & (lens[np.maximum(pt["pix"], 0)] == n)).sum() >= 5, n


def test_truth_agrees_with_the_independent_float64_restatement():
    """Written from different starting points -- numpy_integrate from the maths of the kernel in float64 throughout, points_truth from the
    decision sequence on the float32 inputs -- the two must describe the same integrals: at tests/test_oracle_integrate.py's own tolerance."""
    from test_oracle_integrate import numpy_integrate
    scene = make_scene(P=1500, res=(64, 64), s0=0.05, view="oblique")
    pts = make_points(scene, 3000)
    o = oracle_integrate(scene, pts)
    it = o["oracle"].intermediates()
    ref, valid, _ = numpy_integrate(scene, pts, it)
    rec = dict(view2gaussian=it["view2gaussian"], opac=it["conic_opacity"][:, 3], rgb=it["rgb"])
    shape = (scene["W"], scene["H"], scene["tanfovx"], scene["tanfovy"])
    p1 = IT.pass1_truth(rec, it["point_list"], it["ranges"], *shape, scene["bg"].numpy())
    pt = IT.points_truth(rec, it["point_list"], it["ranges"], p1, pts, scene["viewmatrix"][0].numpy(), *shape)
    assert (valid == pt["ok"]).mean() >= 0.999
    both = valid & pt["ok"]
    d = np.abs(ref[both] - pt["ai"][both])
    assert (d <= 1e-3).mean() >= 0.995, f"max {d.max()}, frac {(d <= 1e-3).mean()}"
    assert np.median(d) <= 1e-4


def test_the_bars_have_teeth():
    p1, pt, fig_o = IT.oracle_truth("I1")
    o = IT.oracle("I1")
    moved = dict(o, ai=np.where(pt["ok"], o["ai"] * np.float32(1 + 2e-5), o["ai"]))
    assert_integrate_parity(o, moved, "perturbed alpha_integrated")          # today's gate lets it through
    failures = []
    IT.check_bars("perturbed", p1, pt, IT.figures(p1, pt, o["out"], o["final_T"][0], moved["ai"]), fig_o, 4.0, failures, o["out"], o["final_T"][0],
                  moved["ai"], show=False)
    assert failures and all(f[1] == "alpha_integrated" for f in failures), failures


@pytest.mark.parametrize("name", IT.WRAP_SCENES)
def test_wrap_scenes_tell_the_wrap_from_full_positions(name):
    p1, pt, fig_o = IT.oracle_truth(name)
    sc, o = IT.scene(name), IT.oracle(name)
    full = IT.points_truth(IT.records_of(o), o["point_list"], o["ranges"], p1, IT.points(name), sc["viewmatrix"][0].numpy(), sc["W"], sc["H"],
                           sc["tanfovx"], sc["tanfovy"], wrap=False)
    ai = full["ai"].astype(np.float32)
    differ = pt["keep"] & (np.abs(ai - pt["ai"]) > 1e-4)
    print("%s: kept points whose integral differs by more than 1e-4 without the wrap: %d" % (name, int(differ.sum())))
    # (measured: 22 and 594. wrap_stop's splats are sub-pixel and its late contributors lie behind nearly everything, so few points feel
    # them; ten, so that the scene does not hang on a single point)
    assert differ.sum() >= 10
    failures = []
    IT.check_bars(name, p1, pt, IT.figures(p1, pt, o["out"], o["final_T"][0], ai), fig_o, 4.0, failures, o["out"], o["final_T"][0], ai,
                  groups=("alpha_integrated",), show=False)
    assert failures
