"""CPU checks of the geometry losses' truth (tests/geometry_loss_truth.py) and of everything the feature decides without a GPU: the
float64 restatement's gradient against central finite differences, term 0 against ``epilogue_torch``'s maps, the argument checks of the
C ABI (they run before any HIP call) and the errors of ``f3dgaus_amd.losses`` on host tensors."""
import ctypes as C

import pytest
import torch

import epilogue_truth as E
import geometry_loss_truth as T


def test_float64_gradient_agrees_with_central_differences():
    """5 x 6 frame, all five terms, alpha weight on: every one of the 270 raster elements, step 1e-6. The terms are piecewise smooth and
    the fixture has no tie within the step, so the central difference is good to ~1e-9 of the gradient's scale."""
    f = T.make_fixture(1, 5, 6, seed=3)
    g = T.grads(f, torch.float64, alpha_weight=True)[0]
    fw = f["frame_weights"][0].double()

    r0 = f["raster"][0].double()

    def loss(r):            # (the alpha weight is data: held at the unperturbed alpha)
        t = T.terms_torch(r, f["world_view"][0], 6, 5, f["FoVx"], f["FoVy"], r0[7], f["depth_target"][0], f["normal_target"][0],
                          f["alpha_target"][0], f["mask"][0])
        return float((t.sum((1, 2)) * fw).sum())

    assert float((r0[6] - f["depth_target"][0].double()).abs().min()) > 1e-5 and float((r0[7] - f["alpha_target"][0].double()).abs().min()) > 1e-5
    h = 1e-6
    fd = torch.zeros_like(r0)
    for i in range(r0.numel()):
        rp, rm = r0.clone(), r0.clone()
        rp.view(-1)[i] += h
        rm.view(-1)[i] -= h
        fd.view(-1)[i] = (loss(rp) - loss(rm)) / (2 * h)
    scale = float(g.abs().max())
    err = float((g - fd).abs().max()) / scale
    print(f"max|g| {scale:.3e}  max|g - fd| / max|g| {err:.3e}")
    assert err < 1e-7
    assert float(g[:3].abs().max()) == 0.0 and float(g[3:7].abs().amax((1, 2)).min()) > 0.0
    # the alpha weight is data: channel 7 sees the alpha term alone
    assert torch.equal(g[7], fw[4] * torch.sign(r0[7] - f["alpha_target"][0].double()))
    assert torch.equal(g[8], torch.full_like(g[8], float(fw[1])))


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_term0_is_one_minus_the_dot_of_the_epilogue_maps(dtype):
    f = T.make_fixture(2, 7, 9)
    for v in range(2):
        r = f["raster"][v].to(dtype)
        nw, dn = E.epilogue_torch(r, f["world_view"][v], 9, 7, f["FoVx"], f["FoVy"])
        want = 1 - (nw * dn).sum(0)
        assert torch.equal(T.terms_torch(r, f["world_view"][v], 9, 7, f["FoVx"], f["FoVy"])[0], want)
        assert torch.equal(T.terms_torch(r, f["world_view"][v], 9, 7, f["FoVx"], f["FoVy"], alpha_weight=True)[0], r[7] * want)
        assert torch.equal(want[0], torch.ones(9, dtype=dtype)) and float((want[1:-1, 1:-1] - 1).abs().min()) > 0      # D = 0 on the border


def test_float32_restatement_is_well_inside_both_rules():
    """The fixtures at the GPU tests' shapes, on the CPU: the float32 restatement's own sums pass the sum rule with room to spare, and
    E_ref of both gradient groups is small, so 4 E_ref means something."""
    for shape in ((2, 19, 37), (1, 3, 5)):
        f = T.make_fixture(*shape)
        t32, t64 = T.per_pixel(f, torch.float32, True), T.per_pixel(f, torch.float64, True)
        s64, bound = T.sum_bounds(t32, t64)
        err = (t32.sum((2, 3)).double() - s64).abs()
        print(shape, "float32 sum error / bound, worst:", float((err / bound).max()))
        assert bool((err <= bound).all())
        g32, g64 = T.grads(f, torch.float32, True), T.grads(f, torch.float64, True)
        for name, sl in E.GROUPS.items():
            e = float((g32[:, sl].double() - g64[:, sl]).abs().max()) / float(g64[:, sl].abs().max())
            print(shape, name, "E_ref", e)
            assert 0 < e < 1e-5


def test_abi_argument_checks_need_no_gpu(f3d):
    from f3dgaus_amd import _lib
    L = _lib.lib()
    assert L.f3dg_geometry_loss_partials_bytes(3, 33, 17) == 3 * 2 * 2 * 5 * 4           # 32 x 16 tiles, five floats per tile
    assert L.f3dg_geometry_loss_partials_bytes(1, 32, 16) == 20
    for bad in ((0, 8, 8), (-1, 8, 8), (1, 0, 8), (1, 8, -3)):
        assert L.f3dg_geometry_loss_partials_bytes(*bad) == 0, bad
    buf = (C.c_char * 1024)()
    one = C.cast(buf, C.c_void_p)
    fwd = lambda F=1, H=8, W=8, raster=one, wv=one, flags=0, partials=one, nbytes=1024, sums=one: L.f3dg_geometry_loss_forward(
        None, F, H, W, raster, wv, 100.0, 100.0, flags, None, None, None, None, partials, nbytes, sums)
    bwd = lambda F=1, H=8, W=8, raster=one, wv=one, flags=0, fw=one, out=one: L.f3dg_geometry_loss_backward(
        None, F, H, W, raster, wv, 100.0, 100.0, flags, None, None, None, None, fw, out)
    for kw in (dict(raster=None), dict(wv=None), dict(sums=None), dict(partials=None), dict(F=0), dict(H=0), dict(W=-1), dict(flags=2),
               dict(flags=-1)):
        assert fwd(**kw) == _lib.ERR_BAD_ARG, kw
    assert fwd(nbytes=19) == _lib.ERR_WORKSPACE and fwd(H=17, W=33, nbytes=79) == _lib.ERR_WORKSPACE
    for kw in (dict(raster=None), dict(wv=None), dict(fw=None), dict(out=None), dict(F=0), dict(H=-2), dict(W=0), dict(flags=4)):
        assert bwd(**kw) == _lib.ERR_BAD_ARG, kw
    assert _lib.GEOM_ALPHA_WEIGHT == 1


def test_python_errors_on_host_tensors(f3d):
    from f3dgaus_amd import losses
    for name in ("geometry_sums", "geometry_loss", "normal_consistency", "distortion_loss", "depth_loss"):
        assert name in losses.__all__ and callable(getattr(losses, name))
    cfg = {"model": {"fov": 50.0}}
    r, wv = torch.zeros(2, 9, 6, 8), torch.eye(4).repeat(2, 1, 1)
    with pytest.raises(RuntimeError, match="HIP device"):                      # no CPU fallback
        losses.geometry_sums(r, wv, cfg)
    with pytest.raises(RuntimeError, match="HIP device"):
        losses.distortion_loss(r)
    with pytest.raises(TypeError, match="float32"):
        losses.geometry_sums(r.double(), wv, cfg)
    with pytest.raises(TypeError, match="depth_target"):
        losses.geometry_sums(r, wv, cfg, depth_target=torch.zeros(2, 6, 8, dtype=torch.float64))
    with pytest.raises(TypeError, match="world_views"):
        losses.geometry_sums(r, wv.double(), cfg)
    with pytest.raises(ValueError, match="9, H, W"):
        losses.geometry_sums(torch.zeros(2, 8, 6, 8), wv, cfg)
    with pytest.raises(ValueError, match="normal_target"):
        losses.geometry_sums(r, wv, cfg, normal_target=torch.zeros(2, 1, 6, 8))
    with pytest.raises(ValueError, match="mask"):
        losses.geometry_sums(r, wv, cfg, mask=torch.zeros(3, 6, 8))
    with pytest.raises(ValueError, match="cameras"):
        losses.geometry_sums(torch.zeros(3, 9, 6, 8), wv, cfg)
    for name in ("depth_target", "normal_target", "alpha_target", "mask"):
        t = torch.zeros(2, 3 if name == "normal_target" else 1, 6, 8, requires_grad=True)
        with pytest.raises(NotImplementedError, match=name):
            losses.geometry_sums(r, wv, cfg, **{name: t})
    with pytest.raises(NotImplementedError, match="cameras"):
        losses.geometry_sums(r, wv.clone().requires_grad_(), cfg)
    with pytest.raises(ValueError, match="w_depth = 0.5 needs `depth_target`"):
        losses.geometry_loss(r, wv, cfg, w_depth=0.5)
    with pytest.raises(ValueError, match="alpha_target"):
        losses.geometry_loss(r, wv, cfg, w_alpha=1.0, depth_target=torch.zeros(2, 6, 8))
    with pytest.raises(ValueError, match="reduction"):
        losses.geometry_loss(r, wv, cfg, w_distortion=1.0, reduction="sum")
