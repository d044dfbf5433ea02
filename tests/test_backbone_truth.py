"""CPU checks of tests/backbone_truth.py, the float64 truth and the bounds of the backbone kernels' device tests: the data has the
conditioning it claims, the truth is the definition, and a CORRECT float32 implementation (torch's own, on the host) stays inside the
bounds -- so that no device run is spent finding that out."""
import numpy as np
import pytest
import torch

import backbone_truth as T

SHAPES = T.NCHW_SHAPES + T.NHWC_SHAPES
CASES = [(s, c) for s in SHAPES for c in T.contents()]
IDS = ["%s-%s" % ("x".join(map(str, s)), c[0]) for s, c in CASES]


def _case(shape, content, seed=11):
    label, ratio, kind = content
    return T.make_case(shape, ratio, seed, kind)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_make_case_slabs_have_the_conditioning_asked_for(shape):
    for ratio in T.RATIOS:
        c = T.make_case(shape, ratio, 3, "normal")
        s = c["x"].double().reshape(shape[0], c["groups"], -1)
        mean, std = s.mean(-1), s.std(-1, unbiased=False)
        got = mean.abs() / std
        assert float((std - 1).abs().max()) < 1e-4                                           # (float32 rounding of values up to 120)
        assert float((got - c["slab_ratio"]).abs().max()) <= 1e-4 * max(1.0, ratio)          # what each slab was given ...
        assert float(got.min()) >= (1 - T.JITTER) * ratio * (1 - 1e-4) and float(got.max()) <= (1 + T.JITTER) * ratio * (1 + 1e-4)
        if c["groups"] * shape[0] >= 16:
            assert bool((mean > 0).any()) and bool((mean < 0).any())                         # ... with both signs in one tensor
    c = T.make_case(shape, 0.0, 3, "near_constant")
    s = c["x"].double().reshape(shape[0], c["groups"], -1)
    assert float((s.mean(-1) - 8).abs().max()) < 1e-5 and float((s.std(-1, unbiased=False) / 1e-3 - 1).abs().max()) < 1e-2
    c = T.make_case(shape, 0.0, 3, "constant")
    s = c["x"].reshape(shape[0], c["groups"], -1)
    assert bool((s == s[..., :1]).all()) and s[..., 0].unique().numel() == s[..., 0].numel()
    assert float(c["weight"].min()) >= 0.5 and float(c["weight"].max()) <= 1.5 and float(c["bias"].abs().max()) <= 0.5


@pytest.mark.parametrize("shape,content", CASES, ids=IDS)
def test_truth_is_the_two_pass_definition(shape, content):
    c = _case(shape, content)
    for silu in (False, True):
        for pb in (None, c["pre_bias"]):
            a = T.truth(c["x"], pb, c["weight"], c["bias"], c["groups"], T.EPS, silu)
            b = T.truth_two_pass(c["x"], pb, c["weight"], c["bias"], c["groups"], T.EPS, silu)
            assert float((a - b).abs().max()) <= 1e-12 * max(1.0, float(b.abs().max())), (silu, pb is not None)


def test_join_truth_and_spacing():
    g = torch.Generator().manual_seed(2)
    a, b = torch.randn(2, 6, 3, 5, generator=g), torch.randn(2, 6, 3, 5, generator=g)
    ba, bb = torch.randn(6, generator=g), torch.randn(6, generator=g)
    want = ((a.double().numpy() + ba.double().numpy()[None, :, None, None]) + (b.double().numpy() + bb.double().numpy()[None, :, None, None])) * 0.5
    assert np.array_equal(T.join_truth(a, ba, b, bb, 0.5).numpy(), want)
    assert torch.equal(T.join_truth(a, None, b, None, 2.0), (a.double() + b.double()) * 2.0)
    # spacing: the distance to the next value up, against the type's own arithmetic, from the subnormals to the top binade
    for dt in (torch.bfloat16, torch.float16):
        tiny = torch.finfo(dt).smallest_normal
        v = torch.tensor([0.0, tiny / 8, tiny / 2, tiny, 1.5 * tiny, 0.75, 1.0, 1.75, 2.0, 100.0, 30000.0], dtype=torch.float64)
        up = torch.nextafter(v.to(dt), torch.tensor(float("inf"), dtype=dt)).double()
        assert torch.equal(T.spacing(v, dt), up - v.to(dt).double()), dt
        assert torch.equal(T.spacing(-v, dt), T.spacing(v, dt))
    assert torch.equal(T.ulp32(torch.tensor([1.0, 1.5, 2.0, 0.0])), torch.tensor([2.0 ** -23, 2.0 ** -23, 2.0 ** -22, 2.0 ** -149], dtype=torch.float64))


def _pivoted_one_pass32(x, pre_bias, weight, bias, groups, eps, silu):
    """The scheme of the kernels in numpy: float32 sums of (v - K) and (v - K)^2 with K the slab's first element (the variance does not
    see the shift, and the sums stay of the size of the deviations), combined in float64; then ((v - mean) * (weight * rstd) + bias)
    in float32."""
    f = np.float32
    v = x.numpy()
    N, C = v.shape[:2]
    cs = (1, C) + (1,) * (v.ndim - 2)
    if pre_bias is not None:
        v = v + pre_bias.numpy().reshape(cs)
    s = v.reshape(N, groups, -1)
    K = s[..., :1]
    d = s - K
    n = s.shape[-1]
    m1 = d.sum(-1, keepdims=True, dtype=f).astype(np.float64) / n
    m2 = (d * d).sum(-1, keepdims=True, dtype=f).astype(np.float64) / n
    mean = (K.astype(np.float64) + m1).astype(f)
    rstd = (1.0 / np.sqrt(np.maximum(m2 - m1 * m1, 0.0) + eps)).astype(f)
    sc = (weight.numpy().reshape(N * 0 + 1, groups, -1, 1) * rstd[..., None]).astype(f)          # [N, G, Cg, 1]
    y = (s.reshape(N, groups, C // groups, -1) - mean[..., None]) * sc + bias.numpy().reshape(1, groups, -1, 1)
    y = y.astype(f).reshape(v.shape)
    if silu:
        y = (y / (f(1) + np.exp(-y))).astype(f)
    return torch.from_numpy(y)


@pytest.mark.parametrize("shape,content", CASES, ids=IDS)
def test_a_correct_float32_implementation_is_inside_the_bounds(shape, content):
    """torch's float32 GroupNorm on the host against the rules of the device tests: itself in float32, and rounded ONCE to bfloat16 /
    float16. And the kernels' scheme replayed in numpy float32 (_pivoted_one_pass32) -- another summation order than torch's -- is
    inside the float32 rule as well, which is what the 2 x margin is for."""
    c = _case(shape, content)
    for silu in (False, True):
        for pb in (None, c["pre_bias"]):
            ref = T.truth(c["x"], pb, c["weight"], c["bias"], c["groups"], T.EPS, silu)
            t32 = T.torch32(c["x"], pb, c["weight"], c["bias"], c["groups"], T.EPS, silu)
            assert bool(torch.isfinite(t32).all())
            e32 = float((t32.double() - ref).abs().max())
            err, bnd, ratio = T.worst(t32, ref, e32, torch.float32)
            assert err <= bnd
            y = _pivoted_one_pass32(c["x"], pb, c["weight"], c["bias"], c["groups"], T.EPS, silu)
            err, bnd, ratio = T.worst(y, ref, e32, torch.float32)
            print(f"{content[0]} silu={int(silu)} pb={int(pb is not None)} pivoted one-pass float32: error {err:.3e} bound {bnd:.3e} ratio {ratio:.2f}")
            assert err <= bnd, (silu, pb is not None, err, bnd)
            for dt in (torch.bfloat16, torch.float16):
                # 16-bit activations: the input is rounded to the type first, the truth and the yardstick see its exact upcast
                x16 = c["x"].to(dt)
                ref16 = T.truth(x16, pb, c["weight"], c["bias"], c["groups"], T.EPS, silu)
                t16 = T.torch32(x16, pb, c["weight"], c["bias"], c["groups"], T.EPS, silu)
                e16 = float((t16.double() - ref16).abs().max())
                err, bnd, ratio = T.worst(t16.to(dt), ref16, e16, dt)
                assert err <= bnd, (dt, silu, pb is not None, err, bnd)
