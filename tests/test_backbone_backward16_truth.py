"""The 16-bit (bfloat16 / float16) backward of the backbone's GroupNorm (+ SiLU) and residual join, without a GPU:
  * the three typed entry points (f3dg_group_norm_silu_forward_stats, f3dg_group_norm_silu_backward_dtype,
    f3dg_residual_join_backward_dtype) refuse on the host what include/f3dg.h says they refuse, in every dtype;
  * ``cfg['model']['backbone_train_dtype']`` is read and validated;
  * the bar of the device test (tests/test_backbone_backward16_gpu.py) is met by the reference arithmetic alone: the float32 restatement
    of the backward formulas on inputs rounded to the type, its ``dx`` rounded ONCE to the type, stays inside ``T.worst`` -- bound32 plus
    half the type's spacing -- and its float32 parameter gradients inside bound32."""
import ctypes as C

import pytest
import torch

import backbone_backward_truth as G
import backbone_truth as T

HALF = (torch.bfloat16, torch.float16)
HALF_IDS = ("bf16", "fp16")
# the NCHW shapes and the small channels-last shapes of the device sweep
SHAPES = ((2, 64, 8, 8), (2, 36, 7, 5), (1, 128, 48, 48), (1, 8, 40, 40), (1, 1024, 9, 9), (2, 384, 20, 13))
NORMAL = [c for c in T.contents() if c[2] == "normal"]


def _sid(s):
    return "x".join(map(str, s))


def test_typed_entry_points_refuse_on_the_host(f3d):
    from f3dgaus_amd import _lib
    L = _lib.lib()
    buf = (C.c_char * 4096)()
    base = (C.addressof(buf) + 15) & ~15
    p = lambda off=0: C.c_void_p(base + off)
    bad, ws = _lib.ERR_BAD_ARG, _lib.ERR_WORKSPACE
    big = 1 << 30

    def bwd(dtype, N, Cc, HW, groups, nhwc, x=p(), gy=p(), dx=p(), stats=p(), scratch=p(), nbytes=big, w=p(), b=p()):
        return L.f3dg_group_norm_silu_backward_dtype(None, dtype, N, Cc, HW, groups, nhwc, x, p(), w, b, stats, 1, gy, dx, p(), p(), p(), scratch, nbytes)

    def fwd(dtype, N, Cc, HW, groups, nhwc, x=p(), y=p(), stats=p(), scratch=p(), nbytes=big, w=p(), b=p()):
        return L.f3dg_group_norm_silu_forward_stats(None, dtype, nhwc, N, Cc, HW, groups, x, p(), w, b, 1e-6, 1, y, stats, scratch, nbytes)

    def jb(dtype, N, Cc, HW, nhwc, gy=p(), g=p(), gb=p(), scratch=p(), nbytes=big):
        return L.f3dg_residual_join_backward_dtype(None, dtype, N, Cc, HW, nhwc, gy, 0.5, g, gb, scratch, nbytes)

    for nhwc in (0, 1):
        for dtype in (-1, 3):
            assert bwd(dtype, 2, 64, 16, 16, nhwc) == bad and fwd(dtype, 2, 64, 16, 16, nhwc) == bad and jb(dtype, 2, 64, 16, nhwc) == bad
            assert bwd(dtype, 0, 64, 16, 16, nhwc) == bad and fwd(dtype, 0, 64, 16, 16, nhwc) == bad and jb(dtype, 0, 64, 16, nhwc) == bad
        for dtype in (0, 1, 2):
            # the backward
            assert bwd(dtype, 2, 64, 16, 24, nhwc) == bad                                      # groups that do not divide C
            for k in ("x", "gy", "dx"):
                assert bwd(dtype, 2, 64, 16, 16, nhwc, **{k: p(4)}) == bad and bwd(dtype, 2, 64, 16, 16, nhwc, **{k: p(8)}) == bad
            assert bwd(dtype, 2, 64, 16, 16, nhwc, stats=p(4)) == bad and bwd(dtype, 2, 64, 16, 16, nhwc, scratch=p(4)) == bad
            for k in ("x", "gy", "stats", "w", "b", "scratch"):
                assert bwd(dtype, 2, 64, 16, 16, nhwc, **{k: None}) == bad, k
            assert bwd(dtype, 2, 64, 16, 16, nhwc, dx=None, nbytes=0) == ws                     # (grad_x is optional: no refusal for it)
            assert bwd(dtype, -1, 64, 16, 16, nhwc) == bad and bwd(dtype, 2, 0, 16, 16, nhwc) == bad and bwd(dtype, 2, 64, 0, 16, nhwc) == bad
            need = L.f3dg_group_norm_silu_backward_scratch_bytes(2, 64, 16, 16, nhwc)          # no dtype among its arguments
            assert need == G.gn_backward_scratch_bytes(2, 64, 16, 16, nhwc)
            assert bwd(dtype, 2, 64, 16, 16, nhwc, nbytes=need - 1) == ws and bwd(dtype, 2, 64, 16, 16, nhwc, nbytes=0) == ws
            assert bwd(dtype, 0, 64, 16, 16, nhwc, nbytes=0) == 0                              # an empty batch: no error, no work
            # the forward that keeps its statistics
            assert fwd(dtype, 2, 64, 16, 24, nhwc) == bad
            for k in ("x", "y"):
                assert fwd(dtype, 2, 64, 16, 16, nhwc, **{k: p(4)}) == bad and fwd(dtype, 2, 64, 16, 16, nhwc, **{k: None}) == bad
            assert fwd(dtype, 2, 64, 16, 16, nhwc, stats=p(4)) == bad and fwd(dtype, 2, 64, 16, 16, nhwc, stats=None) == bad
            assert fwd(dtype, 0, 64, 16, 16, nhwc, stats=None) == bad                          # stats is required, whatever else
            assert fwd(dtype, 2, 64, 16, 16, nhwc, w=None) == bad and fwd(dtype, 2, 64, 16, 16, nhwc, b=None) == bad
            assert fwd(dtype, -1, 64, 16, 16, nhwc) == bad and fwd(dtype, 2, 0, 16, 16, nhwc) == bad and fwd(dtype, 2, 64, 0, 16, nhwc) == bad
            assert fwd(dtype, 0, 64, 16, 16, nhwc, nbytes=0) == 0
            # the join
            assert jb(dtype, 2, 64, 16, nhwc, gy=p(4)) == bad and jb(dtype, 2, 64, 16, nhwc, g=p(4)) == bad
            assert jb(dtype, 2, 64, 16, nhwc, gy=None) == bad and jb(dtype, 2, 64, 16, nhwc, g=None) == bad
            assert jb(dtype, 2, 64, 16, nhwc, scratch=None) == bad and jb(dtype, 2, 64, 16, nhwc, scratch=p(4)) == bad
            assert jb(dtype, -1, 64, 16, nhwc) == bad and jb(dtype, 2, 0, 16, nhwc) == bad and jb(dtype, 2, 64, 0, nhwc) == bad
            need = L.f3dg_residual_join_backward_scratch_bytes(2, 64, 16, nhwc)
            assert need == G.join_backward_scratch_bytes(2, 64, 16, nhwc)
            assert jb(dtype, 2, 64, 16, nhwc, nbytes=need - 1) == ws and jb(dtype, 2, 64, 16, nhwc, nbytes=0) == ws
            assert jb(dtype, 0, 64, 16, nhwc) == 0
    for dtype in (0, 1, 2):
        pn = 4 if dtype == 0 else 8
        # channels-last: whole packets per pixel, at most 1024 channels, a scratch for the forward
        assert bwd(dtype, 2, 22, 16, 1, 1) == bad and fwd(dtype, 2, 22, 16, 1, 1) == bad and jb(dtype, 2, 22, 16, 1) == bad
        assert bwd(dtype, 1, 1032, 16, 24, 1) == bad and fwd(dtype, 1, 1032, 16, 24, 1) == bad and jb(dtype, 1, 1032, 16, 1) == bad
        if pn == 8:      # 4.5 packets of 8 (only refusals are tried here: a call that passes would launch on these host pointers)
            assert bwd(dtype, 2, 36, 16, 9, 1) == bad and fwd(dtype, 2, 36, 16, 9, 1) == bad and jb(dtype, 2, 36, 16, 1) == bad
            assert jb(dtype, 1, 3, 4, 0) == bad                                                # 12 values: one and a half packets of 8
        assert fwd(dtype, 2, 64, 16, 16, 1, nbytes=L.f3dg_group_norm_nhwc_scratch_bytes(2, 16, 16) - 1) == ws
        assert fwd(dtype, 2, 64, 16, 16, 1, scratch=None) == bad
        # the join: no whole number of packets
        assert jb(dtype, 1, 3, 5, 0) == bad and jb(dtype, 3, 1, 3, 0) == bad


def test_backbone_train_dtype_is_read_and_validated(f3d):
    from f3dgaus_amd import cameras
    from f3dgaus_amd import gaussian_predictor as gp
    cfg = cameras.default_cfg(32)
    assert gp.GaussianSplatPredictor_gtunet(cfg).backbone_train_dtype == "fp32"
    cfg["model"]["backbone_train_dtype"] = "fp8"
    with pytest.raises(ValueError, match="backbone_train_dtype"):
        gp.GaussianSplatPredictor_gtunet(cfg)
    for half in ("bf16", "fp16"):
        cfg["model"]["backbone_train_dtype"] = half
        cfg["model"]["backbone_autograd"] = "torch"
        with pytest.raises(ValueError, match="backbone_train_dtype.*backbone_autograd"):
            gp.GaussianSplatPredictor_gtunet(cfg)
        cfg["model"].pop("backbone_autograd")                    # (the default route is torch's)
        with pytest.raises(ValueError, match="backbone_train_dtype.*backbone_autograd"):
            gp.GaussianSplatPredictor_gtunet(cfg)
        cfg["model"]["backbone_autograd"] = "fused"
        pred = gp.GaussianSplatPredictor_gtunet(cfg)
        assert pred.backbone_train_dtype == half and pred.backbone_dtype == "fp32"      # the inference option keeps its own key
    cfg["model"]["backbone_train_dtype"] = "fp32"
    cfg["model"]["backbone_autograd"] = "torch"
    assert gp.GaussianSplatPredictor_gtunet(cfg).backbone_train_dtype == "fp32"


@pytest.mark.parametrize("dtype", HALF, ids=HALF_IDS)
@pytest.mark.parametrize("shape", SHAPES, ids=_sid)
def test_reference_arithmetic_meets_the_device_bar(shape, dtype):
    """x and grad_y rounded to the type and upcast exactly; truth G.grad_truth, yardstick G.grad_torch32, candidate G.grad_restated32 with
    its dx rounded once to the type: the dx ratio of T.worst and the parameter-gradient ratios of G.compare stay <= 1 on the four normal
    contents, SiLU off / on, with / without pre_bias. (dx is a half-spacing bound: elements near a rounding midpoint approach 1.)"""
    worst_dx = worst_par = 0.0
    for label, ratio, kind in NORMAL:
        c = T.make_case(shape, ratio, 11, kind)
        x = c["x"].to(dtype).float()
        gy = G.cotangent(shape, 12).to(dtype).float()
        for silu in (False, True):
            for pb in (None, c["pre_bias"]):
                args = (x, pb, c["weight"], c["bias"], c["groups"], T.EPS, silu, gy)
                ref, yard, got = G.grad_truth(*args), G.grad_torch32(*args), G.grad_restated32(*args)
                dx = got["dx"].float().to(dtype)                 # ONE rounding, to nearest even
                e32 = float((yard["dx"].double() - ref["dx"]).abs().max())
                err, bnd, r = T.worst(dx, ref["dx"], e32, dtype)
                worst_dx = max(worst_dx, r)
                assert r <= 1.0, (label, silu, pb is not None, "dx", err, bnd)
                for name, err, bnd, r in G.compare(got, ref, yard):
                    if name == "dx":
                        continue
                    worst_par = max(worst_par, r)
                    assert err <= bnd, (label, silu, pb is not None, name, err, bnd)
    print(f"{_sid(shape)} {dtype}: worst ratio to the bound, dx {worst_dx:.3f}, parameter gradients {worst_par:.2f}")
