"""Per-Gaussian contribution statistics and set pruning on the GPU (csrc/f3dg_contribution.hip, f3dgaus_amd/contribution.py), on the scenes
of tests/compositing_truth.py; the truth, its yardstick and the conditions are held on the CPU by tests/test_contribution_truth.py.

  truth bars   on the ten scenes where clean Gaussians are >= 90 % of the touched ones, after a call whose records, lists and ranges are
               asserted bit-equal to the oracle's: blended and stops equal the truth's on clean Gaussians and lie in
               [certain, certain + uncertain] on the others; the relative errors of max_weight and sum_weight on the clean touched
               Gaussians (median, 99th percentile, maximum) are each <= max(4 x the replay's own statistic, 2^-23): 4 is the project's
               margin for a float32 kernel against a float32 reference, 2^-23 one float32 ulp, and the sum's absolute error is first
               relieved of blended x 2^-33, the rounding of its fixed point;
  identity     final_T is plane 0 of the exact SAVE_AUX forward's, to the bit; per view the sum of all sum_weight is the sum of the
               alpha channel within the recursive-summation bound plus the fixed-point rounding;
  one definition  all 32 bytes per Gaussian are the same whatever lists, path, arithmetic of the forward or chunking of the views;
  pruning      touched >= 1 leaves an exact render bit-identical, a fast one within helpers.assert_render_parity; the compaction's
               ids, gathers, thresholds, mask, K = 0 and P = 0."""
import numpy as np
import pytest
import torch

import compositing_truth as CT
import contribution_truth as KT
import f3dgaus_amd as f3d
from f3dgaus_amd import cameras, synthetic
from helpers import assert_render_parity, export_workspace, run_hip
from test_contribution_truth import TRUTH_SCENES

pytestmark = pytest.mark.gpu


def _forward(sc, device, views=None, **kw):
    """rasterize_views of the scene (of the views `views` only when given); returns (out, radii, workspace)."""
    dev = lambda t: None if t is None else t.to(device)
    sel = (lambda t: t) if views is None else (lambda t: t[list(views)].contiguous())
    out, radii, ws = f3d.rasterize_views(
        dev(sc["means3D"]), dev(sc["opacities"]), dev(sel(sc["viewmatrix"])), dev(sel(sc["projmatrix"])), dev(sel(sc["campos"])), dev(sc["bg"]),
        image_height=sc["H"], image_width=sc["W"], tanfovx=sc["tanfovx"], tanfovy=sc["tanfovy"], sh=dev(sc["shs"]),
        colors_precomp=dev(sc["colors_precomp"]), scales=dev(sc["scales"]), rotations=dev(sc["rotations"]), sh_degree=sc["sh_degree"],
        scale_modifier=sc["scale_modifier"], kernel_size=sc["kernel_size"], **kw)
    return out, radii, ws


def _contribution(sc, ws, stats=None, final_T=None):
    return f3d.contribution_raw(ws, sc["P"], sc["W"], sc["H"], ws.n_views, sc["tanfovx"], sc["tanfovy"], stats=stats, final_T=final_T)


def _stats(sc, device, views=None, stats=None, **kw):
    _, _, ws = _forward(sc, device, views=views, **kw)
    return _contribution(sc, ws, stats=stats)


def _pc(sc, device):
    """The scene as a Gaussian dict [1,P,...] (any keys: prune_gaussians gathers them all)."""
    pc = {"xyz": sc["means3D"], "opacity": sc["opacities"], "scaling": sc["scales"], "rotation": sc["rotations"]}
    pc["shs" if sc["shs"] is not None else "rgbs"] = sc["shs"] if sc["shs"] is not None else sc["colors_precomp"]
    return {k: v.to(device)[None].contiguous() for k, v in pc.items()}


def _scene_of(sc, pc):
    """The scene dict of a (pruned) Gaussian dict."""
    out = dict(sc)
    out.update(means3D=pc["xyz"][0], opacities=pc["opacity"][0], scales=pc["scaling"][0], rotations=pc["rotation"][0],
               shs=pc["shs"][0] if "shs" in pc else None, colors_precomp=pc["rgbs"][0] if "rgbs" in pc else None, P=pc["xyz"].shape[1])
    return out


# ---- truth bars -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", TRUTH_SCENES)
def test_statistics_against_float64_on_their_own_inputs(name, gpu_device):
    sc, V = CT.scene(name), CT.n_views(name)
    h = run_hip(sc, gpu_device, save_aux=True)
    CT.assert_inputs_are_the_oracles(name, h, [CT.oracle(name, v) for v in range(V)])
    s = _contribution(sc, h["workspace"])
    truths, replays = [KT.oracle_truth(name, v) for v in range(V)], [KT.oracle_replay(name, v) for v in range(V)]
    t = dict(blended=sum(x["blended"] for x in truths), stops=sum(x["stops"] for x in truths), uncertain=sum(x["uncertain"] for x in truths),
             sum_w=sum(x["sum_w"] for x in truths), max_w=np.max([x["max_w"] for x in truths], axis=0))
    r_max, r_sum = np.max([x["max_w"] for x in replays], axis=0), sum(x["sum_w"] for x in replays)
    blended, stops = s.blended.cpu().numpy(), s.stops.cpu().numpy()
    clean = t["uncertain"] == 0
    assert np.array_equal(blended[clean], t["blended"][clean]) and np.array_equal(stops[clean], t["stops"][clean])
    for got, k in ((blended, "blended"), (stops, "stops")):
        assert (got >= t[k]).all() and (got <= t[k] + t["uncertain"]).all(), k
    stop_only = clean & (t["blended"] == 0)
    assert not s.max_weight.cpu().numpy()[stop_only].any() and not s.sum_fixed.cpu().numpy()[stop_only].any()
    fig = KT.weight_figures(t, s.max_weight.cpu().numpy(), s.sum_weight.cpu().numpy())
    fig_r = KT.weight_figures(t, r_max, r_sum)
    failures = []
    for k in ("max_weight", "sum_weight"):
        print("%s %-10s rel med / p99 / max  kernel %.2e / %.2e / %.2e   replay %.2e / %.2e / %.2e   (%d clean touched of %d)"
              % ((name, k) + fig[k] + fig_r[k] + (int(KT.clean_touched(t).sum()), int(((blended + stops) > 0).sum()))))
        for stat, a, b in zip(("median", "p99", "max"), fig[k], fig_r[k]):
            if not a <= max(4.0 * b, KT.REL_FLOOR):
                failures.append((name, k, stat, a, max(4.0 * b, KT.REL_FLOOR)))
    assert not failures, failures


# ---- identity with the forward ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CT.SCENES))
def test_identity_with_the_exact_forward(name, gpu_device):
    sc, V = CT.scene(name), CT.n_views(name)
    H, W = sc["H"], sc["W"]
    for v in range(V):
        out, radii, ws = _forward(sc, gpu_device, views=[v], save_aux=True, exact=True, small_path=False)
        e = export_workspace(dict(sc, viewmatrix=sc["viewmatrix"][v:v + 1]), gpu_device, out, radii, ws, True)
        fT = torch.full((1, H, W), -1.0, device=gpu_device)
        s = _contribution(sc, ws, final_T=fT)
        assert np.array_equal(fT.cpu().numpy()[0].view(np.uint32), np.ascontiguousarray(e["final_T"][0, 0]).view(np.uint32)), (name, v)
        total = sum(int(x) for x in s.sum_fixed.cpu().numpy().tolist()) / 4294967296.0
        alpha = e["out_color"][0, 7].astype(np.float64)
        pairs = int(s.blended.sum().item())
        bound = float((e["n_contrib"][0, 0].astype(np.float64) * 2.0 ** -24 * alpha).sum()) + pairs * 2.0 ** -33
        print("%s view %d: sum of sum_weight %.9g, of the alpha channel %.9g, |difference| %.3g, bound %.3g, %d blended pairs, %d stops"
              % (name, v, total, alpha.sum(), abs(total - alpha.sum()), bound, pairs, int(s.stops.sum().item())))
        assert abs(total - alpha.sum()) <= bound
        assert s.views == 1 and s.pixels == H * W


# ---- one definition, every path ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CT.SCENES))
def test_every_path_gives_the_same_32_bytes(name, gpu_device):
    sc, V = CT.scene(name), CT.n_views(name)
    base = _stats(sc, gpu_device).raw
    assert int(base.view(torch.int64)[:, 1].ne(0).sum()) > 0                                   # something was counted
    assert not base[:, 5:].any()                                                               # the padding stays clear
    variants = dict(again=dict(), unculled=dict(tile_cull=False), general_path=dict(small_path=False), exact=dict(exact=True), fast=dict(exact=False),
                    save_aux=dict(save_aux=True), unculled_general_exact=dict(tile_cull=False, small_path=False, exact=True))
    for label, kw in variants.items():
        assert torch.equal(_stats(sc, gpu_device, **kw).raw, base), (name, label)
    if V > 1:       # one three-view call against three accumulated one-view calls (each takes the small-call path), and against 2 + 1
        acc = None
        for v in range(V):
            acc = _stats(sc, gpu_device, views=[v], stats=acc)
        assert torch.equal(acc.raw, base) and acc.views == V and acc.pixels == V * sc["W"] * sc["H"]
        acc = _stats(sc, gpu_device, views=[2], stats=_stats(sc, gpu_device, views=[0, 1]))
        assert torch.equal(acc.raw, base)


def test_overflowed_workspace_adds_nothing(gpu_device):
    sc = CT.scene("tiny")
    _, _, ws = _forward(sc, gpu_device, max_rendered=64, check=False, small_path=False)
    fT = torch.zeros(1, sc["H"], sc["W"], device=gpu_device)
    s = _contribution(sc, ws, final_T=fT)
    assert not s.raw.any() and bool((fT == 1).all())


# ---- pruning ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CT.SCENES))
def test_pruning_the_untouched_keeps_the_render(name, gpu_device):
    sc = CT.scene(name)
    pc = _pc(sc, gpu_device)
    stats = _stats(sc, gpu_device)
    pruned, kept = f3d.prune_gaussians(pc, 0, stats)
    P, K = sc["P"], kept.numel()
    want = torch.nonzero(stats.touched > 0).reshape(-1)
    assert kept.dtype == torch.int32 and torch.equal(kept.long(), want)                        # ascending, the touched ones
    blended, stops = KT.replay_counts(name)
    print("%s: kept %d of %d (the replay keeps %d)" % (name, K, P, int(((blended + stops) > 0).sum())))
    assert K < P or name in ("deep", "wall")
    assert set(pruned) == set(pc)
    for k in pc:
        assert pruned[k].shape == (1, K) + tuple(pc[k].shape[2:]) and torch.equal(pruned[k][0], pc[k][0][want]), k
    small = _scene_of(sc, pruned)
    full_exact, pruned_exact = _forward(sc, gpu_device, exact=True)[0], _forward(small, gpu_device, exact=True)[0]
    assert torch.equal(pruned_exact.view(torch.int32), full_exact.view(torch.int32))           # all nine channels, to the bit
    full_fast, pruned_fast = _forward(sc, gpu_device, exact=False)[0].cpu().numpy(), _forward(small, gpu_device, exact=False)[0].cpu().numpy()
    for v in range(CT.n_views(name)):
        assert_render_parity(pruned_fast[v], full_fast[v], "%s view %d pruned, fast" % (name, v))


@pytest.mark.parametrize("name", ["mixed", "odd3"])
def test_threshold_modes_and_masks(name, gpu_device):
    sc = CT.scene(name)
    pc = _pc(sc, gpu_device)
    s = _stats(sc, gpu_device)
    P = sc["P"]
    mw, sw, tc = s.max_weight, s.sum_weight, s.touched
    mid_m, mid_s = float(mw[mw > 0].median()), float(sw[sw > 0].median())                      # inclusive: the median itself stays
    gen = torch.Generator().manual_seed(3)
    mask = (torch.rand(P, generator=gen) < 0.6).to(gpu_device)
    cases = [(dict(min_touched=1, min_max_weight=0.05), (tc >= 1) & (mw >= 0.05)),
             (dict(min_touched=1, min_max_weight=mid_m), (tc >= 1) & (mw >= mid_m)),
             (dict(min_touched=1, min_sum_weight=mid_s), (tc >= 1) & (sw >= mid_s)),
             (dict(min_touched=10), tc >= 10),
             (dict(min_touched=0, min_max_weight=0.01, min_sum_weight=0.5), (mw >= 0.01) & (sw >= 0.5)),
             (dict(min_touched=1, keep=mask), (tc >= 1) & mask),
             (dict(min_touched=1 << 40), torch.zeros(P, dtype=torch.bool, device=gpu_device))]
    for kw, want in cases:
        pruned, kept = f3d.prune_gaussians(pc, 0, s, **kw)
        ids = torch.nonzero(want).reshape(-1)
        assert torch.equal(kept.long(), ids), kw
        assert 0 < ids.numel() < P or kw["min_touched"] == 1 << 40, kw                         # every case but the last cuts, and keeps
        for k in pc:
            assert torch.equal(pruned[k][0], pc[k][0][ids]), (kw, k)
    # the mask alone, as bool and as bytes; nothing kept; nothing to keep from
    for m in (mask, mask.to(torch.uint8)):
        pruned, kept = f3d.prune_gaussians(pc, 0, keep=m)
        assert torch.equal(kept.long(), torch.nonzero(mask).reshape(-1)) and torch.equal(pruned["xyz"][0], pc["xyz"][0][mask])
    pruned, kept = f3d.prune_gaussians(pc, 0, keep=torch.zeros(P, dtype=torch.bool, device=gpu_device))
    assert kept.numel() == 0 and all(pruned[k].shape == (1, 0) + tuple(pc[k].shape[2:]) for k in pc)
    empty = {k: v[:, :0].contiguous() for k, v in pc.items()}
    pruned, kept = f3d.prune_gaussians(empty, 0, f3d.GaussianContribution(0, gpu_device))
    assert kept.numel() == 0 and pruned["xyz"].shape == (1, 0, 3)


# ---- the Python entries -----------------------------------------------------------------------------------------------------------------
def test_gaussian_contribution_does_not_depend_on_the_chunking(gpu_device):
    res, V = 48, 3
    cfg = cameras.default_cfg(res)
    g = synthetic.make_gaussians(3000, s0=0.05, seed=11, device=gpu_device)
    pc = {k: v.unsqueeze(0).contiguous() for k, v in g.items()}
    pc["opacity"][0, :200] = 1e-4                                       # alpha < 1/255 wherever they land: nothing ever sees them
    ob = cameras.OrbitRig(cfg).orbit(V)
    wv, fp, cc = (t.to(gpu_device) for t in (ob.world_view_transforms, ob.full_proj_transforms, ob.camera_centers))
    bg = torch.zeros(3, device=gpu_device)
    one = f3d.gaussian_contribution(pc, 0, wv, fp, cc, bg, cfg, views_per_call=1)
    three = f3d.gaussian_contribution(pc, 0, wv, fp, cc, bg, cfg, views_per_call=3)
    two = f3d.gaussian_contribution(pc, 0, wv, fp, cc, bg, cfg, views_per_call=2)
    assert torch.equal(one.raw, three.raw) and torch.equal(two.raw, three.raw)
    assert one.views == three.views == V and one.pixels == V * res * res and int(three.touched.gt(0).sum()) > 0
    # accumulation over calls: twice the views, twice the integers, the same maximum
    twice = f3d.gaussian_contribution(pc, 0, wv, fp, cc, bg, cfg, stats=f3d.gaussian_contribution(pc, 0, wv, fp, cc, bg, cfg))
    assert torch.equal(twice.blended, 2 * three.blended) and torch.equal(twice.stops, 2 * three.stops) and torch.equal(twice.sum_fixed, 2 * three.sum_fixed)
    assert torch.equal(twice.max_weight, three.max_weight) and twice.views == 2 * V
    # an exact render_views of the pruned set is the full set's
    pruned, kept = f3d.prune_gaussians(pc, 0, three)
    assert 0 < kept.numel() <= 2800 and int(kept[0]) >= 200
    cfg_exact = cameras.default_cfg(res)
    cfg_exact["model"]["raster_exact"] = True
    full = f3d.render_views(pc, 0, wv, fp, cc, bg, cfg_exact)["raster"]
    assert torch.equal(f3d.render_views(pruned, 0, wv, fp, cc, bg, cfg_exact)["raster"].view(torch.int32), full.view(torch.int32))


def test_python_error_paths_raise_before_any_launch(gpu_device):
    L = f3d._lib.lib()
    sc = CT.scene("tiny")
    pc = _pc(sc, gpu_device)
    _, _, ws = _forward(sc, gpu_device)
    s = _contribution(sc, ws)
    two = CT.scene("mixed")         # two copies of a set through two copies of its camera: a several-sets call
    both = dict(two, means3D=torch.cat([two["means3D"]] * 2), opacities=torch.cat([two["opacities"]] * 2), scales=torch.cat([two["scales"]] * 2),
                rotations=torch.cat([two["rotations"]] * 2), colors_precomp=torch.cat([two["colors_precomp"]] * 2),
                viewmatrix=two["viewmatrix"].repeat(2, 1, 1), projmatrix=two["projmatrix"].repeat(2, 1, 1), campos=two["campos"].repeat(2, 1))
    _, _, ws2 = _forward(both, gpu_device, n_sets=2)
    raw = torch.zeros(two["P"], 8, dtype=torch.int32, device=gpu_device)
    host_pc = {k: v.cpu() for k, v in pc.items()}
    torch.cuda.synchronize()
    assert L.f3dg_debug_launch_count(1) > 0
    with pytest.raises(RuntimeError, match="stats=.*keep="):
        f3d.prune_gaussians(pc, 0)
    with pytest.raises(RuntimeError, match="HIP device"):
        f3d.prune_gaussians(host_pc, 0, s)
    with pytest.raises(RuntimeError, match="shape"):
        f3d.prune_gaussians(pc, 0, f3d.GaussianContribution(sc["P"] - 1, gpu_device))
    with pytest.raises(RuntimeError, match="keep must be"):
        f3d.prune_gaussians(pc, 0, keep=torch.ones(sc["P"] + 1, dtype=torch.bool, device=gpu_device))
    with pytest.raises(RuntimeError, match="keep must be"):
        f3d.prune_gaussians(pc, 0, keep=torch.ones(sc["P"], device=gpu_device))
    with pytest.raises(RuntimeError, match="holds"):
        f3d.prune_gaussians(dict(pc, opacity=pc["opacity"][:, :-1]), 0, s)
    with pytest.raises(RuntimeError, match="NaN"):
        f3d.prune_gaussians(pc, 0, s, min_max_weight=float("nan"))
    with pytest.raises(RuntimeError, match="last call"):
        f3d.contribution_raw(ws, sc["P"], sc["W"] + 16, sc["H"], 1, sc["tanfovx"], sc["tanfovy"])
    with pytest.raises(RuntimeError, match="shape"):
        f3d.contribution_raw(ws, sc["P"], sc["W"], sc["H"], 1, sc["tanfovx"], sc["tanfovy"], stats=f3d.GaussianContribution(sc["P"] + 1, gpu_device))
    with pytest.raises(RuntimeError, match="final_T"):
        f3d.contribution_raw(ws, sc["P"], sc["W"], sc["H"], 1, sc["tanfovx"], sc["tanfovy"], final_T=torch.zeros(1, 3, 3, device=gpu_device))
    full = f3d.GaussianContribution(sc["P"], gpu_device)
    full.pixels = (1 << 31) - sc["W"] * sc["H"]
    with pytest.raises(RuntimeError, match="2\\^31"):
        f3d.contribution_raw(ws, sc["P"], sc["W"], sc["H"], 1, sc["tanfovx"], sc["tanfovy"], stats=full)
    with pytest.raises(RuntimeError, match="several-sets"):
        f3d.contribution_raw(ws2, two["P"], two["W"], two["H"], 2, two["tanfovx"], two["tanfovy"])
    # ... and the library refuses such a workspace on its own (the header says how many sets the forward rendered)
    import ctypes as C
    rc = L.f3dg_contribution(C.c_void_p(torch.cuda.current_stream().cuda_stream), C.c_void_p(ws2.buffer.data_ptr()), ws2.nbytes, ws2.max_rendered, 2, two["P"],
                             two["W"], two["H"], two["tanfovx"], two["tanfovy"], C.c_void_p(raw.data_ptr()), None)
    assert rc == f3d._lib.ERR_BAD_ARG and not raw.any()
    assert L.f3dg_debug_launch_count(0) == 0                                        # none of the refusals launched anything
