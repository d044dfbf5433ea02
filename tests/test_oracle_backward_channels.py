"""The oracle's compositing backward, cotangent group by cotangent group and output group by output group, against the float64 truth
of tests/grad_truth.py on the oracle's own state (CPU only; fixtures and groups: tests/channel_cases.py).

The yardstick is DESIGN.md section 4's: two independent float32 evaluations of one formula. t32 is the truth function run in float32,
E32 = max|t32 - t64| / max|t64| its own error; the oracle must lie within max(4 E32, 1e-5) of the truth. For the depth (plane 6) and
distortion (plane 8) cotangents this is the first judge that is not a restatement of backward.cu's lines: measured (oracle / t32),
  case        plane 6             plane 8
  A           3e-8 / 4e-8         1.4e-5 / 1.5e-5
  B           4e-8 / 7e-8         1.4e-4 / 8e-5
  C view 0    7e-8 / 1.3e-7       1.3e-4 / 1.4e-4
  C view 1    1.5e-7 / 1.6e-7     7e-5 / 6e-5
  D view 0    1.3e-7 / 2.6e-7     6e-5 / 1.0e-4
  D view 1    7e-8 / 1.8e-7       3e-5 / 4e-5
(the larger of the Sigma and B column groups; notes/compositing_backward_channels.md has the mutations that these bars catch)."""
import numpy as np
import pytest

import channel_cases as cc
from helpers import frac_within

CASES = [(name, v) for name in cc.FIXTURES for v in range(cc.n_views(name))]
IDS = [f"{n}-view{v}" for n, v in CASES]


@pytest.mark.parametrize("name,view", CASES, ids=IDS)
def test_no_pair_is_left_undecided(name, view):
    """The truth takes the skip decisions in float64. A pair within 1e-5 of a threshold is decided by the state's own final
    transmittance; none may stay undecided (its Gaussian would have to be left out of the comparison: the allowed share is zero)."""
    t = cc.oracle_case(name, view)["t64"]["depth"]
    print(f"{name} view {view}: {t['pairs']} in-range pairs, {t['guard_pairs']} within 1e-5 of a threshold, {t['guard_resolved']} decided by final T")
    assert t["pairs"] > 1e5
    assert t["guard_resolved"] == t["guard_pairs"] and t["guard_ids"] == []


@pytest.mark.parametrize("name,view", CASES, ids=IDS)
def test_truth_forward_is_the_oracles_forward(name, view):
    """What ties the surrogate that plane 8's cotangent differentiates to the forward: the truth's float64 plane 6 is the oracle's, and
    A D2 - D1^2 with ATTACHED weights, normalised by (1 - T)^2 + 1e-7, is the oracle's plane 8 -- within the bars of
    tests/test_oracle_forward_fp64.py (median depth rel 1e-5, distortion abs 2e-6 + rel 5e-2, both on 99 % of the pixels; where the
    distortion is well conditioned, above 1e-4, rel 1e-3 on 99 %)."""
    case = cc.oracle_case(name, view)
    val, out = case["t64"]["depth"]["value"], case["o"]["out_color"].astype(np.float64)
    assert (val[6] > 0).sum() > 100
    assert np.array_equal(val[6] > 0, out[6] > 0)                       # the same pixels have a median contributor
    assert frac_within(out[6], val[6], 0.0, 1e-5) >= 0.99, frac_within(out[6], val[6], 0.0, 1e-5)
    assert frac_within(out[8], val[8], 2e-6, 5e-2) >= 0.99, frac_within(out[8], val[8], 2e-6, 5e-2)
    big = val[8] > 1e-4
    if name == "A":         # test_oracle_distortion_on_a_depth_spread_scene's scene
        assert big.sum() > 1000 and val[8].max() > 5e-4, (big.sum(), val[8].max())
    if big.any():
        assert frac_within(out[8][big], val[8][big], 0.0, 1e-3) >= 0.99, frac_within(out[8][big], val[8][big], 0.0, 1e-3)
    # the colour, normal and alpha planes of the same evaluation, for completeness: the bars of that file's s0 = 0.3 scenes
    for ch in (slice(0, 3), slice(3, 6), slice(7, 8)):
        assert frac_within(out[ch], val[ch], 2e-4) >= 0.995, (ch, frac_within(out[ch], val[ch], 2e-4))


@pytest.mark.parametrize("group", cc.GROUP_NAMES)
@pytest.mark.parametrize("name,view", CASES, ids=IDS)
def test_oracle_backward_per_group_against_fp64(name, view, group):
    case = cc.oracle_case(name, view)
    go, t64 = case["grads"][group], cc.split_truth(case["t64"][group])
    got = cc.split(go["dL_dopacity"], go["dL_dcolor"], go["dL_dview2gaussian"], go["dL_dmean2D"])
    for k in cc.TRUTH_OUT:
        e_o, e32 = case["e_oracle"][group][k], case["e32"][group][k]
        print(f"{name} view {view} {group:10s} {k:9s} max|t64| {np.abs(t64[k]).max():.2e}  oracle {e_o:.1e}  t32 {e32:.1e}")
        if cc.is_zero(t64[k]):
            assert cc.is_zero(got[k]), (group, k)
            continue
        assert e_o <= max(cc.MARGIN * e32, cc.FLOOR), (group, k, e_o, e32)
        if group in ("depth", "distortion"):        # a badly conditioned fixture fails instead of passing emptily
            assert cc.MARGIN * max(e_o, e32) <= cc.CONDITION, (group, k, e_o, e32)
    # the structure, exactly
    for k in cc.ZERO_OUT[group]:
        assert cc.is_zero(got[k]), (group, k)
        assert k not in t64 or cc.is_zero(t64[k]), (group, k)
    if group in ("depth", "alpha", "distortion"):
        assert cc.is_zero(go["dL_dsh"]), group
    if group == "alpha":
        for k, v in go.items():
            assert cc.is_zero(v), k
    else:
        assert not cc.is_zero(got["v2g_Sigma"]) and not cc.is_zero(got["v2g_B"]), group
    if group == "depth":
        rows = cc.median_rows(case["t64"][group], case["weights"][group])
        assert len(rows) > 10
        assert np.array_equal(cc.nonzero_rows(go["dL_dview2gaussian"]), rows)
        assert np.array_equal(cc.nonzero_rows(case["t64"][group]["dL_dview2gaussian"]), rows)


def test_median_rows_of_fixture_c():
    assert [len(cc.median_rows(cc.oracle_case("C", v)["t64"]["depth"], cc.oracle_case("C", v)["weights"]["depth"])) for v in (0, 1)] == [24, 55]


def test_float32_truth_takes_the_same_decisions():
    """dtype only changes the arithmetic: the float32 run blends the same pairs (same forward planes up to float32, same medians)."""
    case = cc.oracle_case("C", 1)
    a, b = case["t64"]["depth"], case["t32"]["depth"]
    assert np.array_equal(a["median_id"], b["median_id"]) and a["pairs"] == b["pairs"]
    assert np.abs(a["value"] - b["value"])[0:8].max() <= 1e-3 and not np.array_equal(a["value"], b["value"])
