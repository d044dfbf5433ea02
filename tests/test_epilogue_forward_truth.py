"""The render epilogue's forward against float64, on the host: the truth, the error scales, the condition number and
the cases of tests/epilogue_truth.py, proven on the float32 restatement of the reference's lines before a kernel meets them
(tests/test_epilogue_forward_gpu.py), and the wrappers' refusals of wrong shapes.

    K = |x - truth| / (2^-24 A)      normal_world: per element, A = sum_j |C[i][j] n^_j|
                                     depth_normal: per pixel, the max-norm of the 3-vector's error over |A_c| / |c| + 1

Prints median / p99 / max of K per group, case and entry-point form (``pytest -s``)."""
import math

import numpy as np
import pytest
import torch

import epilogue_truth as T
import forward_bars as FB

CASES = tuple(T.forward_cases())
POOLED = tuple(n for n in CASES if T.forward_cases()[n]["pooled"])
# torch's float32 inverse of world_view^T (an LU solve) is not one rounding from the float64 inverse: two more units on normal_world,
# whose scale holds C once (the depth normal's count has that room already)
LU_ALLOWANCE = 2.0


def test_cases_meet_their_conditions():
    """From the truth alone: at most 0.5 % of a case's interior pixels are fragile (cond < 64); the background case has its exact-zero
    class and an ordinary rim; 2 x 5 has no interior pixel; FoVx != FoVy with W != H is there; the far camera is far."""
    for name in CASES:
        c = T.forward_cases()[name]
        for given in (False, True):
            tr = T.case_truth(name, given)[0]
            n_int, n_frag = int(tr["interior"].sum()), int(tr["fragile"].sum())
            held = tr["interior"] & ~tr["zero_class"]
            print(f"{name:11s} interior {n_int}  fragile {n_frag}  exact-zero {int(tr['zero_class'].sum())}  smallest cond "
                  f"{float(tr['cond'][held].min()) if bool(held.any()) else float('nan'):.3g}")
            assert n_frag <= FB.FRAGILE_CAP * n_int, (name, n_frag, n_int)
            assert n_int == c["raster"].shape[0] * max(c["H"] - 2, 0) * max(c["W"] - 2, 0)
    tr = T.case_truth("background")[0]
    assert int(tr["zero_class"].sum()) == 5 + 13 + 1                    # diamonds of radius 2, 3, 1: their inside of radius 1, 2, 0
    zero_depth = T.forward_cases()["background"]["raster"][:, 6:7] == 0
    rim = tr["interior"] & ~tr["zero_class"] & (zero_depth | torch.nn.functional.max_pool2d(zero_depth.float(), 3, 1, 1).bool())
    assert int(rim.sum()) > 40 and not bool((rim & tr["fragile"]).any()) and float(tr["cond"][rim].min()) > 1e4
    assert int(T.case_truth("2x5")[0]["interior"].sum()) == 0 and int(T.case_truth("3x3")[0]["interior"].sum()) == 1
    c = T.forward_cases()["17x33_fov"]
    fx, fy = T.focal32(c["W"], c["H"], c["FoVx"], c["FoVy"])
    assert c["W"] != c["H"] and abs(fx - fy) > 1.0
    assert float(T.forward_cases()["far"]["c2w"][:, :3, 3].abs().max()) > 500.0
    nrm = T.forward_cases()["degenerate"]["raster"][:, 3:6].norm(dim=1)
    assert int((nrm == 0).sum()) > 100 and int(((nrm > 0) & (nrm < 1e-19)).sum()) > 100


@pytest.mark.parametrize("given_c2w", [False, True], ids=["from_view", "c2w_given"])
@pytest.mark.parametrize("name", CASES)
def test_restatement_within_the_a_priori_bound(name, given_c2w):
    """The float32 restatement on the host, in both entry-point forms: every K within the count of float32 roundings (``OP_COUNT``),
    borders and exact-zero pixels exactly 0, a zero accumulated normal exactly 0."""
    tr, ks, bad, _ = T.case_truth(name, given_c2w)
    assert not bad, bad
    for g in T.K_GROUPS:
        bound = T.OP_COUNT[g] + (LU_ALLOWANCE if g == "normal_world" and not given_c2w else 0.0)
        print(f"epilogue restatement {name:11s} {'c2w given' if given_c2w else 'from view'} {g:13s} K {FB.fmt(FB.k_stats(ks[g]))}   n {ks[g].numel()}   bound {bound:g}")
        assert FB.k_stats(ks[g])[2] <= bound, (name, g, FB.k_stats(ks[g]))


def test_the_bars_have_teeth():
    """Perturbations of the restatement's float32 output that today's gates pass (normal_world within 2e-6 absolute, 99.9 % of the depth
    normal's elements within 1e-3). Each must break a bar; the unperturbed restatement breaks none."""
    ref = {name: T.case_truth(name)[1] for name in CASES}
    assert FB.hold_to_bars(ref, ref, POOLED, "teeth/none") == []
    # one depth normal in 1,000 turned by 1e-4 rad
    ks = {}
    for name in CASES:
        tr, _, _, (nw, dn) = T.case_truth(name)
        dn = dn.clone()
        flat = dn.permute(0, 2, 3, 1).reshape(-1, 3)                    # a copy: written back below
        idx = torch.nonzero(tr["interior"].reshape(-1) & ~tr["zero_class"].reshape(-1)).flatten()[::1000]
        n = flat[idx]
        t = torch.linalg.cross(n, torch.tensor([[0.3, -0.5, 0.8]]).expand_as(n))
        flat[idx] = n * math.cos(1e-4) + t / t.norm(dim=1, keepdim=True) * math.sin(1e-4)
        turned = flat.reshape(dn.shape[0], dn.shape[2], dn.shape[3], 3).permute(0, 3, 1, 2)
        assert float((turned - dn).abs().max()) <= 1e-3                  # today's gate sees nothing
        ks[name], bad = T.forward_K(nw, turned, tr, name)
        assert not bad
    broken = FB.hold_to_bars(ks, ref, POOLED, "teeth/one depth normal in 1,000 turned by 1e-4 rad")
    print("teeth/turned:", broken)
    assert broken and all("depth_normal" in b for b in broken)
    # normal_world through the TRANSPOSED c2w, on a camera whose rotation is symmetric to 1e-6
    f = T.make_fixture(1, 20, 35, seed=5)
    axis = torch.tensor([0.6, -0.64, 0.48], dtype=torch.float64)
    Kx = torch.tensor([[0., -axis[2], axis[1]], [axis[2], 0., -axis[0]], [-axis[1], axis[0], 0.]], dtype=torch.float64)
    wv = torch.eye(4, dtype=torch.float64)
    wv[:3, :3] = (torch.eye(3, dtype=torch.float64) + 5e-7 * Kx).T
    wv[3, :3] = torch.tensor([0.2, -0.1, 2.0], dtype=torch.float64)
    f["world_view"] = wv.float().reshape(1, 4, 4)
    tr = T.forward_truth(f["raster"], T.c2w_truth(f["world_view"]), *T.focal32(35, 20, f["FoVx"], f["FoVy"]))
    good = T.epilogue_torch(f["raster"][0], f["world_view"][0], 35, 20, f["FoVx"], f["FoVy"])
    c2w_t = T.c2w_truth(f["world_view"])[0].float()
    c2w_t[:3, :3] = c2w_t[:3, :3].T.clone()
    wrong = T.epilogue_torch(f["raster"][0], None, 35, 20, f["FoVx"], f["FoVy"], c2w=c2w_t)
    assert 1e-7 < float((wrong[0] - good[0]).abs().max()) < 2e-6          # today's gate sees nothing
    k_good, _ = T.forward_K(good[0][None], good[1][None], tr)
    k_wrong, _ = T.forward_K(wrong[0][None], wrong[1][None], tr)
    broken = FB.hold_to_bars({"near_symmetric": k_wrong}, {"near_symmetric": k_good}, ("near_symmetric",), "teeth/transposed c2w")
    print("teeth/transposed:", broken)
    assert any("normal_world" in b for b in broken)


# ------------------------------------------------------------------------------------------------ the wrappers' refusals (pure Python)
def test_epilogue_wrappers_refuse_wrong_shapes_before_any_launch(f3d):
    """Every check runs before the library is touched, so host tensors show them: a wrong shape or dtype is a ValueError; a well-shaped
    host raster ends at the device check (RuntimeError: no CPU fallback)."""
    from f3dgaus_amd.gaussian_renderer import _epilogue, depth_to_normal
    V, H, W = 2, 4, 6
    raster, wv, fov = torch.zeros(V, 9, H, W), torch.eye(4).repeat(V, 1, 1), 0.8
    with pytest.raises(RuntimeError, match="HIP device"):
        _epilogue(raster, wv, W, H, fov, fov)
    for bad in (torch.zeros(V, 9, W, H), torch.zeros(V, 8, H, W), torch.zeros(9, H, W), torch.zeros(V, 9, H, W + 1), torch.zeros(0, 9, H, W)):
        with pytest.raises(ValueError, match="raster must be"):
            _epilogue(bad, wv, W, H, fov, fov)
    with pytest.raises(ValueError, match="float32"):
        _epilogue(raster.double(), wv, W, H, fov, fov)
    with pytest.raises(ValueError, match="world_view"):
        _epilogue(raster, wv[:1], W, H, fov, fov)
    good = torch.zeros(V, 3, H, W)
    for pair in ((torch.zeros(V, 3, W, H), good), (good, torch.zeros(V, 1, H, W)), (good.double(), good), (good, good[:1]), (good, good[:, :, :, ::2])):
        with pytest.raises(ValueError, match="out "):
            _epilogue(raster, wv, W, H, fov, fov, out=pair)
    with pytest.raises(ValueError, match="pair"):
        _epilogue(raster, wv, W, H, fov, fov, out=(good,))
    with pytest.raises(RuntimeError, match="HIP device"):
        _epilogue(raster, wv, W, H, fov, fov, out=(good, None))
    # depth_to_normal: the launch uses image_width / image_height, so a depth map of another size is refused
    for depth in (torch.ones(1, W, H), torch.ones(1, H, W + 1), torch.ones(2, H, W)):
        with pytest.raises(ValueError, match="depth must be"):
            depth_to_normal(torch.eye(4), W, H, fov, fov, depth)
    with pytest.raises(RuntimeError, match="HIP device"):
        depth_to_normal(torch.eye(4), W, H, fov, fov, torch.ones(1, H, W))
