"""The float64 truth of the contribution statistics (tests/contribution_truth.py), its float32 yardstick, and the claim the pruning rests on.
CPU only: the oracle's records and lists of the twelve scenes of tests/compositing_truth.py (14 views).

  * the cap on clean Gaussians: on the ten scenes the truth bars of tests/test_contribution_gpu.py use, the Gaussians with no uncertain pair
    are at least 90 % of the touched ones in every view -- a condition, not a measurement; a scene that breaks it is to be changed, not the
    cap (depth_spread and wall, where large Gaussians reach many dirty pixels, are left out of those bars only);
  * the replay takes the truth's decisions on every clean Gaussian;
  * a Gaussian that no pixel blends AND that stops no pixel has no effect: with those removed (by the replay's counts, kept rows in input
    order) the CPU oracle's nine channels are bit-identical on all 14 views;
  * "never blended" alone is not enough: removing the stop-only Gaussians too changes odd, filter_precomp and depth_spread -- the pixel they
    stopped blends on. This is the test's teeth;
  * every scene but deep and wall loses Gaussians."""
import numpy as np
import pytest

import compositing_truth as CT
import contribution_truth as KT
from helpers import run_oracle

TRUTH_SCENES = ("tiny", "odd", "small_splats", "aniso_bg", "filter_precomp", "pixel_ordered", "deep", "mixed", "odd3", "thin")
CLEAN_CAP = 0.90
VIEWS = [(n, v) for n in CT.SCENES for v in range(3 if n == "odd3" else 1)]
TRUTH_VIEWS = [nv for nv in VIEWS if nv[0] in TRUTH_SCENES]
STOP_ONLY_MATTERS = ("odd", "filter_precomp", "depth_spread")


def clean_share(t):
    touched = (t["blended"] + t["stops"] + t["uncertain"]) > 0
    return float(((t["uncertain"] == 0) & touched).sum()) / max(int(touched.sum()), 1), int(touched.sum())


@pytest.mark.parametrize("name,view", TRUTH_VIEWS, ids=["%s-v%d" % nv for nv in TRUTH_VIEWS])
def test_clean_gaussians_are_most_of_the_touched_ones(name, view):
    t = KT.oracle_truth(name, view)
    share, touched = clean_share(t)
    print("%s view %d: clean %.4f of %d touched Gaussians; dirty pixels %.3f %%" % (name, view, share, touched, 100 * t["dirty"].mean()))
    assert touched > 0 and share >= CLEAN_CAP


@pytest.mark.parametrize("name,view", VIEWS, ids=["%s-v%d" % nv for nv in VIEWS])
def test_replay_takes_the_truths_decisions_on_clean_gaussians(name, view):
    t, r = KT.oracle_truth(name, view), KT.oracle_replay(name, view)
    clean = t["uncertain"] == 0
    assert np.array_equal(r["blended"][clean], t["blended"][clean]) and np.array_equal(r["stops"][clean], t["stops"][clean])
    # everywhere else the replay's counters lie between the certain pairs and all the pairs that could go either way
    for k in ("blended", "stops"):
        assert (r[k] >= t[k]).all() and (r[k] <= t[k] + t["uncertain"]).all(), k
    # the replay walks as the reference does: its T is the oracle's up to the expf of the two (numpy's correctly rounded one here, libm's
    # there: they differ by an ulp on about one argument in 1,500, and T carries the product of up to ~1,600 factors)
    o = CT.oracle(name, view)
    ref = np.asarray(o["final_T"][0], np.float64)
    rel = np.abs(r["final_T"].astype(np.float64) - ref) / ref
    print("%s view %d replay: final_T differs from the oracle's on %d pixels, at most %.1e relative" % (name, view, int((rel > 0).sum()), rel.max()))
    assert rel.max() <= 2.0 ** -18
    fig = KT.weight_figures(t, r["max_w"], r["sum_w"])
    print("%s view %d replay: max_weight rel med / p99 / max %.2e / %.2e / %.2e   sum_weight %.2e / %.2e / %.2e"
          % ((name, view) + fig["max_weight"] + fig["sum_weight"]))


def _same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, dtype=np.float32).view(np.uint32), np.ascontiguousarray(b, dtype=np.float32).view(np.uint32))


def _oracle_of_pruned(name, keep):
    sc = KT.prune_scene(CT.scene(name), keep)
    return [run_oracle(sc, view=v)["out_color"] for v in range(CT.n_views(name))]


@pytest.mark.parametrize("name", list(CT.SCENES))
def test_pruning_the_untouched_leaves_the_oracle_bit_identical(name):
    blended, stops = KT.replay_counts(name)
    keep = (blended + stops) > 0
    P = keep.size
    print("%s: kept %d of %d (%d stop-only)" % (name, int(keep.sum()), P, int(((blended == 0) & (stops > 0)).sum())))
    if name not in ("deep", "wall"):
        assert keep.sum() < P
    for v, out in enumerate(_oracle_of_pruned(name, keep)):
        assert _same_bits(out, CT.oracle(name, v)["out_color"]), (name, v)


@pytest.mark.parametrize("name", STOP_ONLY_MATTERS)
def test_pruning_by_blended_alone_changes_the_render(name):
    blended, stops = KT.replay_counts(name)
    stop_only = (blended == 0) & (stops > 0)
    assert stop_only.any()
    outs = _oracle_of_pruned(name, blended > 0)
    diff = [float(np.abs(out[7].astype(np.float64) - CT.oracle(name, v)["out_color"][7]).max()) for v, out in enumerate(outs)]
    print("%s: %d stop-only Gaussians; max |alpha difference| per view %s" % (name, int(stop_only.sum()), diff))
    assert any(not _same_bits(out, CT.oracle(name, v)["out_color"]) for v, out in enumerate(outs))
    # the stopped pixel goes on with T (1 - alpha) < 1e-4 and alpha <= 0.99, so T < 1e-2 bounds what its alpha channel can still gain
    assert max(diff) <= 1e-2
