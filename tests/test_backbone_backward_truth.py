"""The gradient truth of the backbone's GroupNorm (+ SiLU) backward (tests/backbone_backward_truth.py), without a GPU:
  * autograd of ``T.truth`` in float64 IS the backward formulas of include/f3dg.h (written out in numpy);
  * a float32 restatement of those formulas with float64 sums stays inside the bound the device sweep uses -- max(2 E32, floor), E32 the
    error of torch's float32 autograd on the same case -- on every shape of the sweep, so the rule asks nothing a sound kernel cannot give;
  * the new entry points refuse on the host what the forward refuses, and size their scratch as the header says."""
import ctypes as C

import pytest
import torch

import backbone_backward_truth as G
import backbone_truth as T

SHAPES = T.NCHW_SHAPES + T.NHWC_SHAPES
NORMAL = [c for c in T.contents() if c[2] == "normal"]


def _sid(s):
    return "x".join(map(str, s))


def _variants(c):
    for silu in (False, True):
        for pb in (None, c["pre_bias"]):
            yield silu, pb


@pytest.mark.parametrize("shape", ((2, 64, 8, 8), (2, 36, 7, 5), (2, 384, 20, 13)), ids=_sid)
def test_autograd_truth_is_the_written_out_formulas(shape):
    c = T.make_case(shape, 10.0, 11)
    gy = G.cotangent(shape, 12)
    for silu, pb in _variants(c):
        ref = G.grad_truth(c["x"], pb, c["weight"], c["bias"], c["groups"], T.EPS, silu, gy)
        got = G.grad_formulas(c["x"], pb, c["weight"], c["bias"], c["groups"], T.EPS, silu, gy)
        assert set(ref) == set(got) and ("dpre_bias" in ref) == (pb is not None)
        for k in ref:
            scale = max(1.0, float(ref[k].abs().max()))
            err = float((got[k].reshape(ref[k].shape) - ref[k]).abs().max())
            assert err <= 1e-11 * scale, (k, silu, pb is not None, err)


@pytest.mark.parametrize("shape", SHAPES, ids=_sid)
def test_float32_restatement_stays_inside_the_device_bound(shape):
    """Every gradient of the restatement within T.bound32(E32, truth) on the four normal contents, SiLU off / on, with / without pre_bias."""
    worst = 0.0
    for label, ratio, kind in NORMAL:
        c = T.make_case(shape, ratio, 11, kind)
        gy = G.cotangent(shape, 12)
        for silu, pb in _variants(c):
            args = (c["x"], pb, c["weight"], c["bias"], c["groups"], T.EPS, silu, gy)
            ref, yard, got = G.grad_truth(*args), G.grad_torch32(*args), G.grad_restated32(*args)
            for name, err, bnd, r in G.compare(got, ref, yard):
                worst = max(worst, r)
                assert err <= bnd, (label, silu, pb is not None, name, err, bnd)
    print(f"{_sid(shape)}: worst ratio of the float32 restatement to the bound {worst:.2f}")


def test_backward_entry_points_refuse_on_the_host_and_size_their_scratch(f3d):
    from f3dgaus_amd import _lib
    L = _lib.lib()
    # the scratch arithmetic
    for N, Cc, HW, groups in ((2, 64, 64, 16), (8, 128, 65536, 32), (1, 16, 36864, 4), (2, 384, 260, 32), (1, 1024, 81, 32), (3, 36, 35, 9)):
        for nhwc in (0, 1):
            assert L.f3dg_group_norm_silu_backward_scratch_bytes(N, Cc, HW, groups, nhwc) == G.gn_backward_scratch_bytes(N, Cc, HW, groups, nhwc)
            assert L.f3dg_residual_join_backward_scratch_bytes(N, Cc, HW, nhwc) == G.join_backward_scratch_bytes(N, Cc, HW, nhwc)
    assert L.f3dg_group_norm_silu_backward_scratch_bytes(0, 64, 64, 16, 0) == 0 and L.f3dg_residual_join_backward_scratch_bytes(0, 64, 64, 1) == 0
    # refusals happen before any HIP call: host memory stands in for the device pointers
    buf = (C.c_char * 4096)()
    base = (C.addressof(buf) + 15) & ~15
    p = lambda off=0: C.c_void_p(base + off)
    bad, ws = _lib.ERR_BAD_ARG, _lib.ERR_WORKSPACE
    big = 1 << 30

    def bwd(N, Cc, HW, groups, nhwc, x=p(), gy=p(), dx=p(), stats=p(), scratch=p(), nbytes=big, w=p()):
        return L.f3dg_group_norm_silu_backward(None, N, Cc, HW, groups, nhwc, x, p(), w, p(), stats, 1, gy, dx, p(), p(), p(), scratch, nbytes)

    for nhwc in (0, 1):
        assert bwd(2, 64, 16, 24, nhwc) == bad                                         # groups that do not divide C
        assert bwd(2, 64, 16, 16, nhwc, x=p(4)) == bad and bwd(2, 64, 16, 16, nhwc, gy=p(4)) == bad and bwd(2, 64, 16, 16, nhwc, dx=p(4)) == bad
        assert bwd(2, 64, 16, 16, nhwc, x=None) == bad and bwd(2, 64, 16, 16, nhwc, gy=None) == bad and bwd(2, 64, 16, 16, nhwc, stats=None) == bad
        assert bwd(2, 64, 16, 16, nhwc, w=None) == bad and bwd(2, 64, 16, 16, nhwc, scratch=None) == bad
        assert bwd(-1, 64, 16, 16, nhwc) == bad and bwd(2, 0, 16, 16, nhwc) == bad and bwd(2, 64, 0, 16, nhwc) == bad
        need = L.f3dg_group_norm_silu_backward_scratch_bytes(2, 64, 16, 16, nhwc)
        assert bwd(2, 64, 16, 16, nhwc, nbytes=need - 1) == ws and bwd(2, 64, 16, 16, nhwc, nbytes=0) == ws
        assert bwd(0, 64, 16, 16, nhwc, nbytes=0) == 0                                 # an empty batch: no error, no work
    assert bwd(2, 22, 16, 1, 1) == bad and bwd(1, 1032, 16, 24, 1) == bad              # channels-last: whole packets, at most 1024 channels

    def stats_fwd(N, Cc, HW, groups, nhwc, x=p(), y=p(), stats=p(), nbytes=big, dtype=0, scratch=p()):
        return L.f3dg_group_norm_silu_forward(None, dtype, nhwc, N, Cc, HW, groups, x, p(), p(), p(), 1e-6, 1, y, stats, scratch, nbytes)

    for nhwc in (0, 1):
        assert stats_fwd(2, 64, 16, 24, nhwc) == bad and stats_fwd(2, 64, 16, 16, nhwc, x=p(4)) == bad and stats_fwd(2, 64, 16, 16, nhwc, y=p(4)) == bad
        assert stats_fwd(2, 64, 16, 16, nhwc, stats=p(4)) == bad             # (stats = NULL is the forward that keeps none: no refusal)
        assert stats_fwd(0, 64, 16, 16, nhwc) == 0
    assert stats_fwd(2, 64, 16, 16, 1, nbytes=8) == ws and stats_fwd(2, 22, 16, 1, 1) == bad
    # the one forward entry: a dtype it does not know, statistics of a 16-bit call, and per dtype what the forward refused before
    need = L.f3dg_group_norm_nhwc_scratch_bytes(2, 16, 16)
    assert need > 0
    for nhwc in (0, 1):
        assert stats_fwd(2, 64, 16, 16, nhwc, dtype=-1) == bad and stats_fwd(2, 64, 16, 16, nhwc, dtype=3) == bad
        assert stats_fwd(2, 64, 16, 16, nhwc, dtype=-1, stats=None) == bad and stats_fwd(2, 64, 16, 16, nhwc, dtype=3, stats=None) == bad
        assert stats_fwd(2, 64, 16, 16, nhwc, dtype=1) == bad and stats_fwd(2, 64, 16, 16, nhwc, dtype=2) == bad
        for dtype in (0, 1, 2):
            assert stats_fwd(2, 64, 16, 24, nhwc, dtype=dtype, stats=None) == bad and stats_fwd(2, 64, 16, 16, nhwc, dtype=dtype, stats=None, x=None) == bad
            assert stats_fwd(2, 64, 16, 16, nhwc, dtype=dtype, stats=None, x=p(4)) == bad and stats_fwd(2, 64, 16, 16, nhwc, dtype=dtype, stats=None, y=p(4)) == bad
            assert stats_fwd(0, 64, 16, 16, nhwc, dtype=dtype, stats=None) == 0
    for dtype in (0, 1, 2):
        assert stats_fwd(2, 64, 16, 16, 1, dtype=dtype, stats=None, nbytes=need - 1) == ws
        assert stats_fwd(2, 64, 16, 16, 1, dtype=dtype, stats=None, scratch=None) == bad
        assert stats_fwd(0, 64, 16, 16, 0, dtype=dtype, stats=None, scratch=None, nbytes=0) == 0
    assert stats_fwd(2, 36, 16, 9, 1, dtype=1, stats=None) == bad and stats_fwd(1, 1032, 16, 24, 1, stats=None) == bad    # 4.5 packets of 8; above 1024 channels

    def jf(N, Cc, HW, nhwc, dtype=0, a=p(), b=p(), y=p()):
        return L.f3dg_residual_join_forward(None, dtype, nhwc, N, Cc, HW, a, p(), b, p(), 0.5, y)

    for nhwc in (0, 1):
        assert jf(2, 64, 16, nhwc, dtype=3) == bad and jf(2, 64, 16, nhwc, dtype=-1) == bad
        for dtype in (0, 1, 2):
            assert jf(2, 64, 16, nhwc, dtype, a=p(4)) == bad and jf(2, 64, 16, nhwc, dtype, b=p(4)) == bad and jf(2, 64, 16, nhwc, dtype, y=p(4)) == bad
            assert jf(2, 64, 16, nhwc, dtype, a=None) == bad and jf(-1, 64, 16, nhwc, dtype) == bad and jf(2, 0, 16, nhwc, dtype) == bad
            assert jf(0, 64, 16, nhwc, dtype) == 0
    assert jf(1, 3, 5, 0) == bad and jf(3, 1, 3, 0) == bad and jf(2, 22, 16, 1) == bad and jf(2, 36, 16, 1, dtype=1) == bad      # no whole number of packets

    def jb(N, Cc, HW, nhwc, gy=p(), g=p(), gb=p(), scratch=p(), nbytes=big):
        return L.f3dg_residual_join_backward(None, N, Cc, HW, nhwc, gy, 0.5, g, gb, scratch, nbytes)

    for nhwc in (0, 1):
        assert jb(2, 64, 16, nhwc, gy=p(4)) == bad and jb(2, 64, 16, nhwc, g=p(4)) == bad and jb(2, 64, 16, nhwc, gy=None) == bad
        assert jb(2, 64, 16, nhwc, scratch=None) == bad
        assert jb(2, 64, 16, nhwc, nbytes=L.f3dg_residual_join_backward_scratch_bytes(2, 64, 16, nhwc) - 1) == ws
        assert jb(0, 64, 16, nhwc) == 0
    assert jb(1, 3, 5, 0) == bad and jb(3, 1, 3, 0) == bad and jb(2, 22, 16, 1) == bad      # no whole number of packets


def test_switch_and_cfg_key_on_the_host(f3d):
    """``backbone_autograd`` is read and validated, ``set_fused_autograd`` flips every GroupNorm and UNetBlock and nothing else, and on the
    host the switch changes nothing: a block with it on gives the same output and gradients as with it off, to the bit."""
    import copy
    from f3dgaus_amd import cameras
    from f3dgaus_amd import gaussian_predictor as gp
    cfg = cameras.default_cfg(32)
    pred = gp.GaussianSplatPredictor_gtunet(cfg)
    flags = lambda m: [x.fused_autograd for x in m.modules() if isinstance(x, (gp.GroupNorm, gp.UNetBlock))]
    assert pred.backbone_autograd == "torch" and len(flags(pred)) > 100 and not any(flags(pred))
    assert gp.set_fused_autograd(pred) is pred and all(flags(pred))
    assert not any(flags(gp.set_fused_autograd(pred, False)))
    del pred
    cfg["model"]["backbone_autograd"] = "hip"
    with pytest.raises(ValueError, match="backbone_autograd"):
        gp.GaussianSplatPredictor_gtunet(cfg)
    torch.manual_seed(2)
    blk = gp.UNetBlock(16, 32, dropout=0.0)
    on = gp.set_fused_autograd(copy.deepcopy(blk))
    x = torch.randn(2, 16, 8, 8)
    outs = []
    for m in (blk, on):
        xl = x.clone().requires_grad_()
        y = m(xl)
        y.sum().backward()
        outs.append([y.detach(), xl.grad] + [p.grad for p in m.parameters()])
    assert all(torch.equal(a, b) for a, b in zip(*outs))
