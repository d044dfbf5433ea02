"""The backbone's kernels between the convolutions (csrc/f3dg_groupnorm.hip: GroupNorm (+ SiLU) in two layouts and three activation
types, with and without the folded convolution bias; the residual join) against float64 (tests/backbone_truth.py), at the conditioning,
shapes and edges where such kernels go wrong.

Bounds. E32 is the max abs error of torch's float32 `silu(group_norm(x32 + pre_bias))` ON THE DEVICE against the float64 truth of the same
case (x32: the exact upcast of a 16-bit input); floor = 2e-6 max(1, max|ref|).
  float32:          max|y - ref| <= max(2 E32, floor)
  bfloat16/float16: |y - ref| <= max(2 E32, floor) + spacing_T(max(|y|, |ref|)) / 2 for every element
i.e. the float32 stage within the suite's margin for another sound summation order, plus ONE rounding of the result where the element
lies. Every case prints error, bound and ratio before it asserts."""
import ctypes as C

import numpy as np
import pytest
import torch

import backbone_truth as T
from f3dgaus_amd import _lib
from f3dgaus_amd import gaussian_predictor as gp

pytestmark = pytest.mark.gpu

DTYPES = (torch.float32, torch.bfloat16, torch.float16)
NAME = {torch.float32: "fp32", torch.bfloat16: "bf16", torch.float16: "fp16"}
PN = {torch.float32: 4, torch.bfloat16: 8, torch.float16: 8}
SWEEP = [("nchw", s) for s in T.NCHW_SHAPES] + [("nhwc", s) for s in T.NHWC_SHAPES + (T.NHWC_LONG_RUN,)]


def _sid(s):
    return "x".join(map(str, s))


def _module(c, dev, groups=None):
    gn = gp.GroupNorm(c["weight"].numel(), eps=T.EPS) if groups is None else gp.GroupNorm(c["weight"].numel(), num_groups=groups, eps=T.EPS)
    gn = gn.to(dev)
    with torch.no_grad():
        gn.weight.copy_(c["weight"]); gn.bias.copy_(c["bias"])
    assert gn.num_groups == c["groups"]
    return gn


def _layout(x, layout):
    return x.contiguous(memory_format=torch.channels_last) if layout == "nhwc" else x.contiguous()


def _check_gn(label, gn, x, pb, silu, expect_nhwc=None):
    """One call of the module on x (any layout / type) against the truth; returns the output."""
    with torch.no_grad():
        y = gn(x, silu=silu, pre_bias=pb)
        ref = T.truth(x, pb, gn.weight, gn.bias, gn.num_groups, gn.eps, silu)
        e32 = float((T.torch32(x, pb, gn.weight, gn.bias, gn.num_groups, gn.eps, silu).double() - ref).abs().max())
    assert y.dtype == x.dtype and y.shape == x.shape
    if expect_nhwc is not None:                      # the layout of the result tells which kernel ran
        assert gp._is_nhwc(y) == expect_nhwc, label
    assert bool(torch.isfinite(y).all()), label
    err, bnd, ratio = T.worst(y, ref, e32, x.dtype)
    print(f"{label}: error {err:.3e}  bound {bnd:.3e}  ratio {ratio:.2f}  (E32 {e32:.3e})")
    assert err <= bnd, (label, err, bnd)
    return y


# ------------------------------------------------------------------------------------------------ (a) conditioning sweep
@pytest.mark.parametrize("content", T.contents(), ids=lambda c: c[0])
@pytest.mark.parametrize("layout,shape", SWEEP, ids=["%s-%s" % (l, _sid(s)) for l, s in SWEEP])
def test_group_norm_conditioning_sweep(gpu_device, layout, shape, content):
    """|mean| / std of the (sample, group) slabs from 0.5 to 100, near-constant and constant slabs; both layouts, three activation types,
    SiLU off / on, with and without pre_bias, through gaussian_predictor.GroupNorm."""
    label, ratio, kind = content
    c = T.make_case(shape, ratio, 11, kind)
    gn = _module(c, gpu_device)
    pb = c["pre_bias"].to(gpu_device)
    x32 = _layout(c["x"].to(gpu_device), layout)
    for dt in DTYPES:
        x = x32.to(dt)
        assert gp._is_nhwc(x) == (layout == "nhwc")
        for silu in (False, True):
            for p in (None, pb):
                _check_gn(f"{layout} {_sid(shape)} {label} {NAME[dt]} silu={int(silu)} pb={int(p is not None)}", gn, x, p, silu,
                          expect_nhwc=layout == "nhwc")


# ------------------------------------------------------------------------------------------------ (b) isolation
@pytest.mark.parametrize("dt", (torch.float32, torch.bfloat16), ids=lambda d: NAME[d])
@pytest.mark.parametrize("layout", ("nchw", "nhwc"))
def test_group_norm_non_finite_value_stays_in_its_slab(gpu_device, layout, dt):
    """One NaN, then one +Inf, in a single (sample, group): every other slab equals the clean run to the bit, the poisoned slab is
    non-finite throughout."""
    shape, n, g = (2, 128, 20, 13), 1, 5
    c = T.make_case(shape, 10.0, 5)
    gn = _module(c, gpu_device)
    pb = c["pre_bias"].to(gpu_device)
    cg = shape[1] // c["groups"]
    x = _layout(c["x"].to(gpu_device).to(dt), layout)
    with torch.no_grad():
        clean = gn(x, silu=True, pre_bias=pb)
        for bad in (float("nan"), float("inf")):
            xb = x.clone()
            xb[n, g * cg + 1, 7, 4] = bad
            assert gp._is_nhwc(xb) == (layout == "nhwc")
            y = gn(xb, silu=True, pre_bias=pb)
            slab = torch.zeros(shape, dtype=torch.bool, device=gpu_device)
            slab[n, g * cg:(g + 1) * cg] = True
            assert not bool(torch.isfinite(y[slab]).any()), bad
            assert bool(torch.isfinite(y[~slab]).all()) and torch.equal(y[~slab], clean[~slab]), bad


# ------------------------------------------------------------------------------------------------ (c) determinism
@pytest.mark.parametrize("shape", ((1, 128, 64, 64), (1, 16, 192, 192), T.NHWC_LONG_RUN), ids=_sid)
def test_channels_last_group_norm_is_bit_identical_run_to_run(gpu_device, shape):
    c = T.make_case(shape, 10.0, 6)
    gn = _module(c, gpu_device)
    pb = c["pre_bias"].to(gpu_device)
    for dt in DTYPES:
        x = _layout(c["x"].to(gpu_device), "nhwc").to(dt)
        with torch.no_grad():
            a, b = gn(x, silu=True, pre_bias=pb), gn(x, silu=True, pre_bias=pb)
        assert gp._is_nhwc(a) and torch.equal(a, b), NAME[dt]


# ------------------------------------------------------------------------------------------------ (d) residual join
def _int_join_case(shape, dev, dt):
    """Small integers and distinct per-channel integer biases, scale 0.5: with a and b even in [-8, 8], bias_a[c] = 8 c and
    bias_b[c] = -3 c - 1, every intermediate of ((a + bias_a) + (b + bias_b)) * 0.5 is exact in float32, float16 and bfloat16 with both
    biases, the first only, or none (C <= 40: a + 8 c and a + 8 c + b are multiples of 2 below 512, b - 3 c - 1 and the sum with both
    biases, a + b + 5 c - 1, are below 256 in magnitude; the halves of the latter are odd multiples of 0.5 for every other channel)."""
    N, Cc, H, W = shape
    assert Cc <= 40
    i = torch.arange(N * H * W * Cc, device=dev, dtype=torch.int64)
    a = (((i * 5) % 9) - 4) * 2
    b = (((i * 7) % 9) - 4) * 2
    a = a.reshape(N, H, W, Cc).permute(0, 3, 1, 2).to(dt)           # values laid out along the channels-last order; layout set by the caller
    b = b.reshape(N, H, W, Cc).permute(0, 3, 1, 2).to(dt)
    ch = torch.arange(Cc, device=dev, dtype=torch.float32)
    return a, b, 8 * ch, -3 * ch - 1


def _join_exact(dev, shape, dt, layout, combos=((True, True), (True, False), (False, False))):
    a, b, ba, bb = _int_join_case(shape, dev, dt)
    a, b = _layout(a, layout), _layout(b, layout)
    assert gp._is_nhwc(a) == (layout == "nhwc")
    for use_a, use_b in combos:
        pa, pbb = (ba if use_a else None), (bb if use_b else None)
        tb = lambda t, bias: t if bias is None else t + bias.to(t.dtype).reshape(1, -1, 1, 1)
        want = (tb(a, pa) + tb(b, pbb)) * 0.5
        assert torch.equal(want.double(), T.join_truth(a, pa, b, pbb, 0.5))             # exact in the type, as claimed
        buf = a.clone()
        with torch.no_grad():
            got = gp.residual_join(buf, pa, b, pbb, 0.5)
        assert got.data_ptr() == buf.data_ptr(), "the kernel writes into a's storage"     # (the torch fall-back returns a new tensor)
        assert got.dtype == dt and torch.equal(got, want), (shape, NAME[dt], layout, use_a, use_b,
                                                            int((got != want).sum()), float((got.double() - want.double()).abs().max()))


JOIN_SMALL = [("nchw", (2, 6, 3, 3), (torch.float32,)),                        # packets straddle channels and samples
              ("nchw", (2, 12, 3, 3), (torch.bfloat16, torch.float16)),
              ("nchw", (2, 8, 4, 6), DTYPES),                                    # packets inside a channel
              ("nhwc", (3, 24, 5, 7), DTYPES),                                   # 6 / 3 packets per pixel
              ("nhwc", (1, 40, 6, 6), (torch.bfloat16, torch.float16))]          # 5 packets per pixel


@pytest.mark.parametrize("layout,shape,dtypes", JOIN_SMALL, ids=["%s-%s" % (l, _sid(s)) for l, s, _ in JOIN_SMALL])
def test_residual_join_is_exact_on_integers(gpu_device, layout, shape, dtypes):
    for dt in dtypes:
        assert shape[0] * shape[1] * shape[2] * shape[3] % PN[dt] == 0
        _join_exact(gpu_device, shape, dt, layout)


@pytest.mark.parametrize("shape,dt", (((3, 24, 484, 484), torch.float32), ((6, 24, 484, 484), torch.bfloat16)), ids=("fp32", "bf16"))
def test_residual_join_looping_threads_keep_their_channels(gpu_device, shape, dt):
    """Just above 16383 x 256 packets the grid is capped and threads take a second packet one grid stride on; channels-last, their bias
    values are loaded once, so the stride must be a whole number of pixels. All three bias combinations."""
    n_packets = shape[0] * shape[1] * shape[2] * shape[3] // PN[dt]
    assert 16383 * 256 < n_packets < 16383 * 256 * 1.01
    _join_exact(gpu_device, shape, dt, "nhwc")


@pytest.mark.parametrize("layout", ("nchw", "nhwc"))
def test_residual_join_random_data_within_one_rounding(gpu_device, layout):
    """Random data on (2, 64, 16, 16). Operands and biases are positive and the scale is 0.5, so that the bound -- 2 float32 ulps of |ref|
    for the float32 stage -- follows from the arithmetic: the three float32 additions err by at most half an ulp each of a value no
    larger than the sum, the multiplication by 0.5 is exact, 1.5 ulps of |ref| in all; a 16-bit result adds half its spacing."""
    g = torch.Generator().manual_seed(9)
    shape = (2, 64, 16, 16)
    a32, b32 = torch.rand(shape, generator=g) * 1.5 + 0.5, torch.rand(shape, generator=g) * 1.5 + 0.5
    ba, bb = torch.rand(64, generator=g).to(gpu_device), torch.rand(64, generator=g).to(gpu_device)
    for dt in DTYPES:
        a, b = _layout(a32.to(gpu_device).to(dt), layout), _layout(b32.to(gpu_device).to(dt), layout)
        ref = T.join_truth(a, ba, b, bb, 0.5)
        buf = a.clone()
        with torch.no_grad():
            got = gp.residual_join(buf, ba, b, bb, 0.5)
        assert got.data_ptr() == buf.data_ptr() and got.dtype == dt
        err = (got.double() - ref).abs()
        bnd = 2 * T.ulp32(ref)
        if dt != torch.float32:
            bnd = bnd + 0.5 * T.spacing(torch.maximum(got.double().abs(), ref.abs()), dt)
        r = err / bnd
        i = int(r.argmax())
        print(f"join {layout} {NAME[dt]}: error {float(err.flatten()[i]):.3e}  bound {float(bnd.flatten()[i]):.3e}  ratio {float(r.flatten()[i]):.2f}")
        assert bool((err <= bnd).all()), (layout, NAME[dt], float(r.max()))


# ------------------------------------------------------------------------------------------------ (e) refusals through the C ABI
def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _off(t, nbytes=0):
    return C.c_void_p(t.data_ptr() + nbytes)


def _all_nan(t):
    torch.cuda.synchronize()
    return bool(torch.isnan(t.float()).all())


@pytest.mark.parametrize("dt", DTYPES, ids=lambda d: NAME[d])
def test_c_abi_refuses_what_the_kernels_cannot_take_and_writes_nothing(gpu_device, dt):
    L = _lib.lib()
    kd = gp._KERNEL_DTYPE[dt]
    pn, dev = PN[dt], gpu_device
    big = 1032 * 16 + 64
    x = torch.ones(big, device=dev).to(dt)
    b2 = torch.ones(big, device=dev).to(dt)
    y = torch.full((big,), float("nan"), device=dev).to(dt)
    w, b, pb = (torch.ones(1040, device=dev) for _ in range(3))
    mom_bytes = L.f3dg_group_norm_nhwc_scratch_bytes(4, 4096, 32) + 8
    mom = torch.zeros(mom_bytes // 8, dtype=torch.float64, device=dev)

    def nchw(N, Cc, HW, groups, xo=0, yo=0):
        return L.f3dg_group_norm_silu_forward(_stream(), kd, 0, N, Cc, HW, groups, _off(x, xo), _off(pb), _off(w), _off(b), 1e-6, 1, _off(y, yo), None, None, 0)

    def nhwc(N, Cc, HW, groups, xo=0, yo=0):
        return L.f3dg_group_norm_silu_forward(_stream(), kd, 1, N, Cc, HW, groups, _off(x, xo), _off(pb), _off(w), _off(b), 1e-6, 1, _off(y, yo), None,
                                              _off(mom), mom_bytes)

    def jn(N, Cc, HW, cl, ao=0, bo=0, yo=0):
        return L.f3dg_residual_join_forward(_stream(), kd, cl, N, Cc, HW, _off(x, ao), _off(pb), _off(b2, bo), _off(pb), 0.5, _off(y, yo))

    bad = _lib.ERR_BAD_ARG
    # a pointer 4 bytes off the 16-byte grid
    assert nchw(2, 64, 16, 16, xo=4) == bad and nchw(2, 64, 16, 16, yo=4) == bad
    assert nhwc(2, 64, 16, 16, xo=4) == bad and nhwc(2, 64, 16, 16, yo=4) == bad
    for cl in (0, 1):
        assert jn(2, 64, 16, cl, ao=4) == bad and jn(2, 64, 16, cl, bo=4) == bad and jn(2, 64, 16, cl, yo=4) == bad
    # channels that do not divide into the groups
    assert nchw(2, 64, 16, 24) == bad and nhwc(2, 64, 16, 24) == bad
    # channels-last: whole 16-byte packets per pixel, at most 1024 channels
    assert nhwc(2, pn * 5 + pn // 2, 16, 1) == bad and nhwc(1, 1032, 16, 24) == bad
    assert jn(2, pn * 5 + pn // 2, 16, 1) == bad
    # a join whose element count is not a whole number of packets
    assert jn(1, 3, pn + 1, 0) == bad and jn(3, 1, 3, 0) == bad
    assert _all_nan(y)
    # an empty batch is no error and no work
    assert nchw(0, 64, 16, 16) == 0 and nhwc(0, 64, 16, 16) == 0 and jn(0, 64, 16, 0) == 0 and jn(0, 64, 16, 1) == 0
    assert _all_nan(y)
    # (and the same calls with what was wrong put right do write)
    assert nchw(2, 64, 16, 16) == 0 and not _all_nan(y[:2 * 64 * 16]) and _all_nan(y[2 * 64 * 16:])


def test_python_wrappers_serve_the_shapes_the_kernels_refuse(gpu_device):
    """The same situations through gaussian_predictor: another kernel or the torch operators take over, within the bounds of the sweep."""
    dev = gpu_device
    # a dense view that starts 4 bytes into its allocation, both layouts
    c = T.make_case((2, 64, 8, 8), 10.0, 21)
    gn = _module(c, dev)
    pb = c["pre_bias"].to(dev)
    flat = torch.zeros(c["x"].numel() + 1, device=dev)
    flat[1:] = c["x"].flatten().to(dev)
    xv = flat[1:].reshape(c["x"].shape)
    assert xv.data_ptr() % 16 == 4 and xv.is_contiguous()
    _check_gn("wrapper, NCHW view at +4 bytes", gn, xv, pb, True)
    flat[1:] = c["x"].permute(0, 2, 3, 1).flatten().to(dev)
    xv = flat[1:].reshape(2, 8, 8, 64).permute(0, 3, 1, 2)
    assert xv.data_ptr() % 16 == 4 and gp._is_nhwc(xv)
    _check_gn("wrapper, channels-last view at +4 bytes", gn, xv, pb, True)
    # channels-last with channels that are no whole number of packets (bfloat16: 36 = 4.5 packets), and with 1032 channels
    c = T.make_case((2, 36, 7, 5), 10.0, 22)
    _check_gn("wrapper, channels-last C=36 bf16", _module(c, dev), _layout(c["x"].to(dev).bfloat16(), "nhwc"), c["pre_bias"].to(dev), True)
    c = T.make_case((2, 6, 5, 5), 10.0, 23)
    _check_gn("wrapper, channels-last C=6 fp32", _module(c, dev), _layout(c["x"].to(dev), "nhwc"), c["pre_bias"].to(dev), True)
    c = T.make_case((1, 1032, 3, 3), 10.0, 24, groups=24)
    _check_gn("wrapper, channels-last C=1032 fp32", _module(c, dev, groups=24), _layout(c["x"].to(dev), "nhwc"), c["pre_bias"].to(dev), True)
    # an empty batch
    with torch.no_grad():
        assert gn(torch.zeros(0, 64, 8, 8, device=dev), silu=True).shape == (0, 64, 8, 8)
    # a join whose element count is no whole number of packets, and one at a misaligned address: the torch expression
    g = torch.Generator().manual_seed(3)
    a, b = torch.randn(1, 3, 3, 3, generator=g).to(dev), torch.randn(1, 3, 3, 3, generator=g).to(dev)
    ba, bb = torch.randn(3, generator=g).to(dev), torch.randn(3, generator=g).to(dev)
    want = ((a + ba.reshape(1, -1, 1, 1)) + (b + bb.reshape(1, -1, 1, 1))) * 0.5
    with torch.no_grad():
        assert torch.equal(gp.residual_join(a.clone(), ba, b, bb, 0.5), want)
        flat = torch.zeros(2 * 8 * 4 * 4 + 1, device=dev)
        av = flat[1:].reshape(2, 8, 4, 4)
        av.copy_(torch.randn(2, 8, 4, 4, generator=g))
        b8 = torch.randn(2, 8, 4, 4, generator=g).to(dev)
        ba8, bb8 = torch.randn(8, generator=g).to(dev), torch.randn(8, generator=g).to(dev)
        want = ((av + ba8.reshape(1, -1, 1, 1)) + (b8 + bb8.reshape(1, -1, 1, 1))) * 0.5
        assert torch.equal(gp.residual_join(av.clone(), ba8, b8, bb8, 0.5), want)          # (a clone is aligned: the kernel; same float32 operations)
        assert torch.equal(gp.residual_join(av, ba8, b8, bb8, 0.5), want)


# ------------------------------------------------------------------------------------------------ (f) other ranks
@pytest.mark.parametrize("shape", ((2, 64, 50), (2, 64, 3, 4, 5)), ids=_sid)
def test_group_norm_other_ranks_run_the_fused_kernel(gpu_device, shape, monkeypatch):
    """[N, C, L] and a 5-D input: the NCHW kernel with HW = the product of the trailing dimensions (50: the scalar path in bfloat16, 60:
    packets in float32), not the torch operators -- which the module cannot reach here."""
    import types

    def no_torch(*a, **k):
        raise AssertionError("GroupNorm took the torch operators")
    monkeypatch.setattr(gp, "F", types.SimpleNamespace(group_norm=no_torch, silu=no_torch))
    c = T.make_case(shape, 10.0, 31)
    gn = _module(c, gpu_device)
    pb = c["pre_bias"].to(gpu_device)
    for dt in (torch.float32, torch.bfloat16):
        _check_gn(f"rank {len(shape)} {_sid(shape)} {NAME[dt]}", gn, c["x"].to(gpu_device).to(dt), pb, True)


# ------------------------------------------------------------------------------------------------ (g) reported, not asserted
def test_report_conditioning_of_a_backbone_pass(gpu_device):
    """How far into the sweep a real pass goes: the largest |mean| / std over all (sample, group) slabs of every GroupNorm call of one
    pass of the formula-weight SongUNet on the songunet.npz input. A figure for the reader (profiles/backbone_kernels.md), no bound."""
    import os
    from f3dgaus_amd import cameras
    from helpers_weights import formula_state_dict
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "songunet.npz"))
    pred = gp.GaussianSplatPredictor_gtunet(cameras.default_cfg()).eval()
    sd = pred.state_dict()
    keep = {k: v for k, v in sd.items() if k in ("ray_dirs", "sh_to_v_transform", "v_to_sh_transform") or k.endswith("resample_filter")}
    pred.load_state_dict(formula_state_dict({k: tuple(v.shape) for k, v in sd.items()}, keep=keep))
    pred = pred.to(gpu_device)
    seen = []

    def hook(name):
        def fn(mod, args, kwargs):
            x = args[0].double()
            pb = kwargs.get("pre_bias")
            if pb is not None:
                x = x + pb.double().reshape(1, -1, *([1] * (x.dim() - 2)))
            s = x.reshape(x.shape[0], mod.num_groups, -1)
            r = s.mean(-1).abs() / s.std(-1, unbiased=False)
            seen.append((float(r.max()), float(r.median()), name, tuple(args[0].shape)))
        return fn

    handles = [m.register_forward_pre_hook(hook(n), with_kwargs=True) for n, m in pred.named_modules() if isinstance(m, gp.GroupNorm)]
    with torch.no_grad():
        pred.network_with_offset(torch.from_numpy(g["x"]).to(gpu_device), N_views_xa=1)
    for h in handles:
        h.remove()
    top = max(seen)
    med = float(np.median([s[1] for s in seen]))
    print(f"GroupNorm calls in one backbone pass: {len(seen)}; largest |mean|/std of a (sample, group) slab {top[0]:.2f} at {top[2]} "
          f"{top[3]}; median over the calls of the per-call median {med:.2f}; calls with a slab above 10: {sum(s[0] > 10 for s in seen)}")
    assert len(seen) > 0 and all(np.isfinite(s[0]) for s in seen)
