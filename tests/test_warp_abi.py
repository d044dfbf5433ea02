"""The forward warp and the masked L1 at the boundary, without a device: the symbols exist and are bound, the workspace arithmetic, every
documented argument check of the C ABI (all of them return before any HIP call), and the Python wrappers' refusals."""
import ctypes as C
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("f3dg_forward_warp_workspace_bytes", "f3dg_forward_warp", "f3dg_masked_l1_partials_bytes", "f3dg_masked_l1_forward",
         "f3dg_masked_l1_backward")
CFG = {"model": {"fov": 13.164}}


def test_symbols_are_declared_exported_and_bound(f3d):
    from f3dgaus_amd import _lib
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "f3dg.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(f3dg_\w+)\s*\(", txt))
    L = C.CDLL(_lib.LIB_PATH)
    for n in NAMES:
        assert n in declared and n in _lib.SIGNATURES and hasattr(L, n), n
        assert getattr(_lib.lib(), n).argtypes == _lib.SIGNATURES[n][1]
    data = open(_lib.LIB_PATH, "rb").read()
    for kernel in (b"warp_zbuffer_kernel", b"warp_splat_kernel", b"warp_resolve_kernel", b"warp_erode_kernel", b"masked_l1_fwd_kernel",
                   b"masked_l1_bwd_kernel"):
        assert kernel in data, kernel
    import f3dgaus_amd.warp as w                      # through the alias finder
    assert w.__spec__.name == "f3d-gaus_amd.warp"
    assert set(w.__all__) == {"forward_warp", "relative_transforms"} and f3d.forward_warp is w.forward_warp
    assert {"warping_sums", "warping_loss"} <= set(f3d.losses.__all__)


def test_workspace_arithmetic(f3d):
    L = f3d._lib.lib()
    ws = L.f3dg_forward_warp_workspace_bytes
    base = ws(8, 4, 3, 256, 256)
    px = 8 * 4 * 256 * 256
    assert base == px * (8 * (3 + 2) + 4 + 4)        # accumulators [pair][C + 2][H W] u64, the z-buffer, the mask before erosion
    assert base < ws(9, 4, 3, 256, 256) and base < ws(8, 5, 3, 256, 256) and base < ws(8, 4, 4, 256, 256)
    assert base < ws(8, 4, 3, 257, 256) and base < ws(8, 4, 3, 256, 257)
    for bad in ((0, 4, 3, 8, 8), (8, 0, 3, 8, 8), (8, 4, 0, 8, 8), (8, 4, 3, 0, 8), (8, 4, 3, 8, 0), (-1, 4, 3, 8, 8), (8, 4, 3, -8, 8),
                (8, 4, 17, 8, 8), (1, 1, 3, 4096, 2049), (1 << 30, 4, 3, 8, 8)):
        assert ws(*bad) == 0, bad
    assert ws(1, 1, 16, 4096, 2048) == (1 << 23) * (8 * 18 + 8)
    pb = L.f3dg_masked_l1_partials_bytes
    assert pb(2, 3, 37, 19) == 2 * 2 * 2 * 2 * 4 and pb(2, 3, 32, 16) == 2 * 2 * 4          # a slot of two floats per 32 x 16 tile
    assert pb(3, 3, 37, 19) > pb(2, 3, 37, 19) and pb(2, 3, 65, 19) > pb(2, 3, 37, 19) and pb(2, 3, 37, 33) > pb(2, 3, 37, 19)
    for bad in ((0, 3, 8, 8), (2, 0, 8, 8), (2, 3, 0, 8), (2, 3, 8, 0), (2, 3, -1, 8), (1, 3, 1 << 15, 1 << 15)):
        assert pb(*bad) == 0, bad


def test_argument_checks_return_before_any_launch(f3d):
    from f3dgaus_amd import _lib
    L = _lib.lib()
    buf = (C.c_char * 4096)()
    p = C.cast(buf, C.c_void_p)
    odd = C.c_void_p(p.value + 4)
    good = dict(stream=None, n_src=1, n_views=1, C=3, H=2, W=2, image=p, depth=p, valid=None, rel=p, fx=10.0, fy=10.0, z_near=0.01, tol=0.05,
                floor=1 / 16, thr=0.9, erode=0, ws=p, ws_bytes=1 << 40, warped=p, mask=p, wdepth=None, weight=None)
    call = lambda **kw: L.f3dg_forward_warp(*{**good, **kw}.values())
    nan, inf = float("nan"), float("inf")
    bad_arg = [dict(image=None), dict(depth=None), dict(rel=None), dict(ws=None), dict(warped=None), dict(mask=None), dict(ws=odd),
               dict(n_src=0), dict(n_views=0), dict(C=0), dict(H=0), dict(W=-3), dict(fx=0.0), dict(fy=-1.0), dict(fx=nan), dict(fy=inf),
               dict(z_near=-0.1), dict(z_near=nan), dict(z_near=inf), dict(tol=-1e-3), dict(tol=nan), dict(floor=-0.1), dict(floor=1.5),
               dict(floor=nan), dict(thr=nan), dict(erode=-1), dict(erode=2), dict(erode=4), dict(erode=17)]
    for kw in bad_arg:
        assert call(**kw) == _lib.ERR_BAD_ARG, kw
    for kw in (dict(C=17), dict(H=4096, W=2049), dict(n_src=1 << 30, n_views=4)):
        assert call(**kw) == _lib.ERR_UNSUPPORTED, kw
    need = L.f3dg_forward_warp_workspace_bytes(1, 1, 3, 2, 2)
    assert need == 4 * (8 * 5 + 8)
    assert call(ws_bytes=need - 1) == _lib.ERR_WORKSPACE and call(ws_bytes=0) == _lib.ERR_WORKSPACE
    # the masked L1
    fwd = lambda **kw: L.f3dg_masked_l1_forward(*{**dict(s=None, F=1, C=3, H=2, W=2, a=p, b=p, m=p, part=p, nbytes=1 << 20, sums=p), **kw}.values())
    bwd = lambda **kw: L.f3dg_masked_l1_backward(*{**dict(s=None, F=1, C=3, H=2, W=2, a=p, b=p, m=p, fw=p, out=p), **kw}.values())
    for kw in (dict(F=0), dict(C=0), dict(H=0), dict(W=-1), dict(a=None), dict(b=None), dict(m=None)):
        assert fwd(**kw) == _lib.ERR_BAD_ARG and bwd(**kw) == _lib.ERR_BAD_ARG, kw
    assert fwd(part=None) == _lib.ERR_BAD_ARG and fwd(sums=None) == _lib.ERR_BAD_ARG
    assert bwd(fw=None) == _lib.ERR_BAD_ARG and bwd(out=None) == _lib.ERR_BAD_ARG
    assert fwd(nbytes=7) == _lib.ERR_WORKSPACE
    assert fwd(H=1 << 15, W=1 << 15) == _lib.ERR_UNSUPPORTED and bwd(H=1 << 15, W=1 << 15) == _lib.ERR_UNSUPPORTED


def test_python_wrappers_refuse_without_a_device(f3d):
    from f3dgaus_amd import losses, warp
    B, V, Cn, H, W = 2, 3, 3, 4, 5
    img, dep = torch.rand(B, Cn, H, W), torch.full((B, H, W), 7.0)
    src, dst = torch.eye(4).repeat(B, 1, 1), torch.eye(4).repeat(B, V, 1, 1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        warp.forward_warp(img, dep, src, dst, CFG)
    with pytest.raises(TypeError, match="float32"):
        warp.forward_warp(img.double(), dep, src, dst, CFG)
    with pytest.raises(TypeError, match="`depth` must be float32"):
        warp.forward_warp(img, dep.double(), src, dst, CFG)
    with pytest.raises(TypeError, match="`valid` must be float32"):
        warp.forward_warp(img, dep, src, dst, CFG, valid=torch.ones(B, H, W, dtype=torch.int32))
    with pytest.raises(TypeError, match="`src_world_view` must be float32"):
        warp.forward_warp(img, dep, src.double(), dst, CFG)
    with pytest.raises(ValueError, match=r"\[B, C, H, W\]"):
        warp.forward_warp(img[0], dep, src, dst, CFG)
    with pytest.raises(ValueError, match="`depth` is"):
        warp.forward_warp(img, dep[:, :3], src, dst, CFG)
    with pytest.raises(ValueError, match="`src_world_view` is"):
        warp.forward_warp(img, dep, src[:1], dst, CFG)
    with pytest.raises(ValueError, match="at most 16 channels"):
        warp.forward_warp(torch.rand(B, 17, H, W), dep, src, dst, CFG)
    for name, args in (("image", (img.clone().requires_grad_(), dep, src, dst)), ("depth", (img, dep.clone().requires_grad_(), src, dst)),
                       ("src_world_view", (img, dep, src.clone().requires_grad_(), dst)), ("dst_world_views", (img, dep, src, dst.clone().requires_grad_()))):
        with pytest.raises(NotImplementedError, match=f"no gradient for `{name}`"):
            warp.forward_warp(*args, CFG)
    # relative_transforms is plain torch: on the CPU it is the float64 product, [V,4,4] shared or [B,V,4,4]
    import warp_truth as T
    f = T.make_fixture(2, 4, 3, 5)
    rel = warp.relative_transforms(f["src_world_view"], f["dst_world_views"])
    assert rel.dtype == torch.float32 and rel.shape == (2, 4, 4, 4) and rel.is_contiguous()
    assert float((rel - T.relative(f["src_world_view"], f["dst_world_views"])).abs().max()) <= 2.0 ** -22
    shared = warp.relative_transforms(f["src_world_view"], f["dst_world_views"][0])
    assert torch.equal(shared[0], rel[0]) and shared.shape == (2, 4, 4, 4)
    with pytest.raises(ValueError, match="dst_world_views"):
        warp.relative_transforms(f["src_world_view"], f["dst_world_views"][:1])
    # the loss
    r, w, m = torch.rand(B, V, Cn, H, W), torch.rand(B, V, Cn, H, W), torch.ones(B, V, 1, H, W)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        losses.warping_loss(r, w, m)
    with pytest.raises(ValueError, match="differ in shape"):
        losses.warping_sums(r, w[:, :2], m)
    with pytest.raises(ValueError, match="`mask` is"):
        losses.warping_sums(r, w, m[:, :, :, :2])
    with pytest.raises(TypeError, match="float32"):
        losses.warping_sums(r.double(), w.double(), m)
    with pytest.raises(TypeError, match="`mask` must be"):
        losses.warping_sums(r, w, m.double())
    with pytest.raises(NotImplementedError, match="no gradient for `warped`"):
        losses.warping_loss(r, w.clone().requires_grad_(), m)
    with pytest.raises(NotImplementedError, match="no gradient for `mask`"):
        losses.warping_loss(r, w, m.clone().requires_grad_())
    with pytest.raises(ValueError, match="reduction"):
        losses.warping_loss(r, w, m, reduction="sum")
