"""The splat head's forward against float64, on the host: the truth, the error scales and the cases of
tests/splat_head_truth.py, proven on the float32 restatement of the reference's lines before a kernel meets them
(tests/test_splat_head_forward_gpu.py), and the wrappers' refusals of wrong shapes.

    K = |x - truth| / (2^-24 A)      truth: the restatement in float64 on the call's own float32 inputs;  A: the element's error scale

Prints median / p99 / max of K per group and case (``pytest -s``)."""
import numpy as np
import pytest
import torch

import forward_bars as FB
import splat_head_truth as T

CASES = tuple(T.forward_cases())
POOLED = tuple(n for n in CASES if T.forward_cases()[n][2])


def test_scales_bound_the_truth_and_cases_meet_their_conditions():
    """A >= |truth| in every group (each scale holds the element's own magnitude); the fragile clip elements stay within the cap, from the
    truth alone; every case with B > 1 has distinct cameras and quaternions; the perspective case's w3 lies in 0.5 .. 2; the clip cases
    do reach beyond 10 and clamp what their threshold says."""
    for name in CASES:
        inputs, clip, _ = T.forward_cases()[name]
        tr = T.case_truth(name)[0]
        for g in T.K_GROUPS:
            t, A = tr["out"][g], tr["A"][g]
            fin = torch.isfinite(t) & torch.isfinite(A)
            assert bool((A[fin] >= t[fin].abs() * (1 - 1e-12)).all()), (name, g)
        n_xy = tr["fragile"][..., :2].numel()
        assert int(tr["fragile"].sum()) <= FB.FRAGILE_CAP * n_xy, (name, int(tr["fragile"].sum()), n_xy)
        B = inputs["net_out"].shape[0]
        for b in range(1, B):
            assert not torch.equal(inputs["v2w"][b], inputs["v2w"][0]) and not torch.equal(inputs["quat"][b], inputs["quat"][0]), name
    den = T.case_truth("289px_persp")[0]["den"]
    assert 0.5 < float(den.min()) and float(den.max()) < 2.0 and float(den.max() - den.min()) > 0.5
    X = T.case_truth("clip_10")[0]["out"]["xyz"][..., :2].abs()
    n_beyond = int((X > 10.0).sum())
    assert n_beyond > 20 and int((X < 0.3).sum()) > 20
    assert int(T.case_truth("clip_10")[0]["clamped"].sum()) == 0                         # the `< 10` switch: at 10.0 nothing is clamped
    assert int(T.case_truth("clip_9.999")[0]["clamped"].sum()) == n_beyond               # (no |X| lies between 9.999 and 10)
    assert int(T.case_truth("clip_0.3")[0]["clamped"].sum()) > n_beyond
    assert not T.case_truth("clip_9.999")[0]["clamped"][..., 2].any()                    # z is never clamped


def test_special_value_classes_are_populated():
    """The saturation and quaternion cases do contain what they are for: results under 2^-126 and over the float32 maximum, zero scales
    (a zero quaternion), active clamps, and cancelling components."""
    tr = T.case_truth("saturation")[0]
    assert int((tr["A"]["opacity"] < FB.TINY).sum()) >= 6 and int((tr["A"]["scaling"] < FB.TINY).sum()) >= 6
    assert int((tr["out"]["scaling"] > FB.F32_MAX).sum()) >= 6 and int((tr["out"]["scaling"] > 1e38).sum()) >= 12      # 89, and 88 below the maximum
    tr = T.case_truth("quaternions")[0]
    assert int((tr["A"]["rotation"] == 0).sum()) >= 4 * 8
    exact, near = T.conj_pixels(5, 7)
    vec = tr["out"]["rotation"][:, :, 1:]
    assert float(vec[:, exact].abs().max()) < 1e-15 and 1e-7 < float(vec[:, near].abs().max()) < 3e-6
    assert float(tr["A"]["rotation"][:, exact].min()) > 0.1                              # the scale holds the products, not the result


@pytest.mark.parametrize("name", CASES)
def test_restatement_within_the_a_priori_bound(name):
    """The float32 restatement on the host: every K within the group's count of float32 roundings (``OP_COUNT``: the bound of any
    correct float32 evaluation, to first order), copies bit-equal, clamped x / y bit-equal to +-float32(squre_clip), special values by
    their rule."""
    inputs, clip, _ = T.forward_cases()[name]
    tr, ks, bad, r32 = T.case_truth(name)
    for g in T.K_GROUPS:
        print(f"splat head restatement {name:12s} {g:13s} K {FB.fmt(FB.k_stats(ks[g]))}   n {ks[g].numel()}   bound {T.OP_COUNT[g]:g}")
    assert not bad, bad
    assert T.copies_bit_equal(r32, inputs)
    for g in T.K_GROUPS:
        assert FB.k_stats(ks[g])[2] <= T.OP_COUNT[g], (name, g, FB.k_stats(ks[g]))


def _perturbed(fn):
    """{case: {group: K}} of the restatement's float32 outputs after ``fn(name, outputs)`` changed a copy of them, and the broken rules."""
    ks, bad = {}, []
    for name in CASES:
        out = {k: v.clone() for k, v in T.case_truth(name)[3].items()}
        fn(name, out)
        ks[name], b = T.forward_K(out, T.case_truth(name)[0], name)
        bad += b
    return ks, bad


def test_the_bars_have_teeth():
    """Perturbations of the restatement's float32 output that the whole-tensor gate max|a - b| / max(1, max|b|) < 3e-6 passes. Each must
    break a bar; the unperturbed restatement breaks none."""
    ref = {name: T.case_truth(name)[1] for name in CASES}
    assert FB.hold_to_bars(ref, ref, POOLED, "teeth/none") == []

    def gate_passes(name, out):
        r32 = T.case_truth(name)[3]
        for k in T.KEYS:
            a, b = out[k].double(), r32[k].double()
            fin = torch.isfinite(b)
            assert float((a[fin] - b[fin]).abs().max()) / max(1.0, float(b[fin].abs().max())) < 3e-6, (name, k)

    def xyz_scaled(name, out):
        out["xyz"] *= (1 + 2e-6)
        if name == "fixture":
            gate_passes(name, out)

    def scaling_scaled(name, out):
        out["scaling"] *= (1 + 1e-6)
        if name == "fixture":
            gate_passes(name, out)

    def one_opacity_in_1000(name, out):
        o = out["opacity"].view(-1)
        o[::1000] += 1e-6
        if name == "fixture":
            gate_passes(name, out)

    def small_rotations_zeroed(name, out):
        if name == "quaternions":
            _, near = T.conj_pixels(5, 7)
            r = out["rotation"][:, near]
            out["rotation"][:, near] = torch.where(r.abs() < 3e-6, torch.zeros(()), r)
            gate_passes(name, out)

    for label, fn in (("xyz x (1 + 2e-6)", xyz_scaled), ("scaling x (1 + 1e-6)", scaling_scaled),
                      ("one opacity in 1,000 off by 1e-6", one_opacity_in_1000), ("cancelling rotation components zeroed", small_rotations_zeroed)):
        ks, _ = _perturbed(fn)
        broken = FB.hold_to_bars(ks, ref, POOLED, f"teeth/{label}")
        print(f"teeth/{label}: {broken}")
        assert broken, label


# ------------------------------------------------------------------------------------------------ the wrappers' refusals (pure Python)
def _good():
    B, H, W = 2, 3, 4
    return {"net_out": torch.zeros(B, 23, H, W), "depth": torch.ones(B, 1, H, W), "ray_dirs": torch.ones(1, 3, H, W),
            "view_to_world": torch.eye(4).repeat(B, 1, 1), "cam_quat": torch.tensor([[1., 0., 0., 0.]]).repeat(B, 1)}


def test_splat_head_refuses_wrong_shapes_before_any_launch(f3d):
    """Every check runs before the library is touched, so host tensors show them: a wrong shape is a ValueError; well-shaped host tensors
    end at the device check (RuntimeError: no CPU fallback)."""
    from f3dgaus_amd.gaussian_predictor import allocate_gaussians
    g = _good()
    with pytest.raises(RuntimeError, match="HIP device"):
        f3d.splat_head(**g)
    for key, bad in (("depth", torch.ones(2, 3, 4)), ("depth", torch.ones(2, 1, 4, 3)), ("depth", torch.ones(1, 1, 3, 4)),
                     ("ray_dirs", torch.ones(1, 3, 3, 3)), ("ray_dirs", torch.ones(1, 2, 3, 4)),
                     ("view_to_world", torch.eye(4).reshape(1, 4, 4)), ("cam_quat", torch.ones(2, 3))):
        with pytest.raises(ValueError, match=key):
            f3d.splat_head(**{**g, key: bad})
    with pytest.raises(RuntimeError, match="23-channel"):
        f3d.splat_head(**{**g, "net_out": torch.zeros(2, 22, 3, 4)})
    ok = allocate_gaussians(2, 36, "cpu")
    with pytest.raises(RuntimeError, match="HIP device"):
        f3d.splat_head(**g, out=ok, n_offset=24)
    for n_offset in (-1, 25, 36):
        with pytest.raises(ValueError, match="n_offset"):
            f3d.splat_head(**g, out=ok, n_offset=n_offset)
    with pytest.raises(ValueError, match="n_offset"):
        f3d.splat_head(**g, n_offset=12)
    for key, shape in (("xyz", (2, 36, 1)), ("xyz", (2, 36)), ("rotation", (2, 36, 3)), ("features_rest", (2, 36, 9)), ("opacity", (2, 35, 1)),
                       ("unet_depth", (1, 36, 1)), ("features_dc", (2, 36, 3))):
        with pytest.raises(ValueError, match=key):
            f3d.splat_head(**g, out={**ok, key: torch.zeros(shape)})
    with pytest.raises(RuntimeError, match="float32"):
        f3d.splat_head(**g, out={**ok, "scaling": torch.zeros(2, 36, 3, dtype=torch.float64)})
    with pytest.raises(ValueError, match="lack"):
        f3d.splat_head(**g, out={k: v for k, v in ok.items() if k != "opacity"})


def test_splat_head_merge_refuses_wrong_shapes_before_any_launch(f3d):
    g = _good()
    args = lambda **kw: ([kw.get("net_out", g["net_out"])] * 2, [g["depth"], kw.get("depth", g["depth"])], kw.get("ray_dirs", g["ray_dirs"]),
                         [g["view_to_world"], kw.get("view_to_world", g["view_to_world"])], [g["cam_quat"]] * 2)
    with pytest.raises(RuntimeError, match="HIP device"):
        f3d.splat_head_merge(*args())
    with pytest.raises(ValueError, match="pass 1: depth"):
        f3d.splat_head_merge(*args(depth=torch.ones(2, 1, 4, 3)))
    with pytest.raises(ValueError, match="pass 0: ray_dirs"):
        f3d.splat_head_merge(*args(ray_dirs=torch.ones(1, 3, 2, 4)))
    with pytest.raises(ValueError, match="pass 1: view_to_world"):
        f3d.splat_head_merge(*args(view_to_world=torch.eye(4)))
    with pytest.raises(RuntimeError, match="like pass 0"):
        f3d.splat_head_merge([g["net_out"], torch.zeros(2, 23, 4, 3)], [g["depth"]] * 2, g["ray_dirs"], [g["view_to_world"]] * 2, [g["cam_quat"]] * 2)
