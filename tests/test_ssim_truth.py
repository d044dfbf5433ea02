"""CPU tests of the fused image loss: the float64 helper every GPU comparison uses (tests/ssim_truth.py) is pinned to the reference's own
float64 results recorded in tests/golden/ssim/*.npz, and the host-side checks of the C ABI and of f3dgaus_amd.losses -- which run
before any HIP call -- are exercised without a device."""
import ctypes as C

import numpy as np
import pytest
import torch

import ssim_truth as T


@pytest.mark.parametrize("name", T.cases() + [T.case_name(T.PADDING_SHAPE, "padding")])
def test_helper_reproduces_the_reference_float64(name):
    z = T.load(name)
    t = T.truth(z["img1"], z["img2"], dL_dmap=z["dL_dmap"])
    e_map = float(np.abs(t["map"] - z["map64"]).max())
    e_mean = abs(t["mean"] - float(z["mean64"]))
    e_grad = float(np.abs(t["grad_mean"] - z["grad64"]).max())
    print(f"{name}: map {e_map:.2e} mean {e_mean:.2e} grad {e_grad:.2e}")
    assert z["map64"].dtype == np.float64 and z["grad64"].dtype == np.float64 and z["map32"].dtype == np.float32
    assert e_map <= 1e-10 and e_mean <= 1e-10 and e_grad <= 1e-10
    # the per-plane means (the reference evaluated every plane alone) and the size of the gradient for the recorded random cotangent
    hw = z["img1"].shape[-1] * z["img1"].shape[-2]
    assert float(np.abs(t["sums"][:, 0] / hw - z["plane_mean64"]).max()) <= 1e-10
    assert abs(float(np.abs(t["grad"]).max()) - float(z["grad_dl_max64"])) <= 1e-10
    assert z["dL_dmap"].dtype == np.float32 and z["dL_dmap"].shape == z["img1"].shape and float(z["grad_dl_err32"]) > 0


def test_taps_are_the_recorded_window():
    g = T.taps().numpy()
    assert g.dtype == np.float32 and g.shape == (11,)
    for name in T.cases():
        assert np.array_equal(T.load(name)["window"], g), name
    assert len(set(g.tolist())) == 6 and np.array_equal(g, g[::-1])


def test_truth_cotangent_forms_agree():
    """A full dL/dm plane of 1 / n is the mean; per-plane weights on the sums of m are the same thing."""
    z = T.load("random_2x3x7x5")
    a, b = z["img1"], z["img2"]
    n = a.size
    by_map = T.truth(a, b, dL_dmap=np.full(a.shape, 1.0 / n))
    w = np.zeros((6, 3))
    w[:, 0] = 1.0 / n
    by_weights = T.truth(a, b, plane_weights=w)
    assert np.abs(by_map["grad"] - by_map["grad_mean"]).max() <= 1e-15
    assert np.abs(by_weights["grad"] - by_map["grad_mean"]).max() <= 1e-15


def test_fixture_shapes_of_the_reference_results():
    """psnr is [N, 1], ssim(size_average=False) is [N], the losses are scalars -- the shapes f3dgaus_amd.losses returns."""
    for shape in T.SHAPES:
        z = T.load(T.case_name(shape, "random"))
        assert z["psnr32"].shape == (shape[0], 1) and z["ssim_n32"].shape == (shape[0],)
        assert z["l1_32"].shape == () and z["l2_32"].shape == () and z["mean32"].shape == ()
        assert z["img1"].shape == shape and z["map64"].shape == shape and z["grad32"].shape == shape


# ---- host-side argument checks of the C ABI: they run before any HIP call
def _abi():
    from f3dgaus_amd import _lib
    return _lib, _lib.lib()


def test_partials_bytes(f3d):
    _lib, L = _abi()
    f = L.f3dg_ssim_partials_bytes
    assert f(1, 1, 1) == 12                          # one tile, three float32 sums
    assert f(0, 64, 64) == 0 and f(-3, 64, 64) == 0 and f(3, 0, 64) == 0 and f(3, 64, -1) == 0
    base = f(3, 64, 64)
    assert base >= 3 * 3 * 4
    for n in (3, 4, 96, 384):                          # monotone in each argument
        assert f(n, 64, 64) <= f(n + 1, 64, 64)
    for s in (1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 255, 256):
        assert f(3, s, 64) <= f(3, s + 1, 64) and f(3, 64, s) <= f(3, 64, s + 1)
    assert f(384, 256, 256) > f(96, 256, 256) > f(96, 128, 256)


def test_forward_argument_checks(f3d):
    _lib, L = _abi()
    buf = (C.c_char * 4096)()
    p = C.cast(buf, C.c_void_p)
    need = L.f3dg_ssim_partials_bytes(2, 40, 20)

    def rc(n=2, W=40, H=20, img1=p, img2=p, out=(p, p, p, p), partials=p, nbytes=need, sums=p):
        return L.f3dg_ssim_forward(None, n, W, H, img1, img2, *out, partials, nbytes, sums)
    assert rc(img1=None) == _lib.ERR_BAD_ARG and rc(img2=None) == _lib.ERR_BAD_ARG
    assert rc(n=0) == _lib.ERR_BAD_ARG and rc(W=0) == _lib.ERR_BAD_ARG and rc(H=-2) == _lib.ERR_BAD_ARG
    assert rc(partials=None) == _lib.ERR_BAD_ARG                       # plane_sums without partials
    assert rc(nbytes=need - 1) == _lib.ERR_WORKSPACE and rc(nbytes=0) == _lib.ERR_WORKSPACE
    assert rc(partials=None, sums=None, nbytes=0, out=(None,) * 4) == _lib.OK      # nothing asked for: nothing launched


def test_backward_argument_checks(f3d):
    _lib, L = _abi()
    buf = (C.c_char * 4096)()
    p = C.cast(buf, C.c_void_p)
    names = ("img1", "img2", "dL_dmap", "plane_weights", "dm_dmu1", "dm_dsigma1_sq", "dm_dsigma12", "dL_dimg1")

    def rc(n=2, W=40, H=20, **kw):
        a = {k: p for k in names}
        a.update(kw)
        return L.f3dg_ssim_backward(None, n, W, H, *[a[k] for k in names])
    for k in ("img1", "img2", "dm_dmu1", "dm_dsigma1_sq", "dm_dsigma12", "dL_dimg1"):
        assert rc(**{k: None}) == _lib.ERR_BAD_ARG, k
    assert rc(dL_dmap=None, plane_weights=None) == _lib.ERR_BAD_ARG     # neither gradient form
    assert rc(n=0) == _lib.ERR_BAD_ARG and rc(W=-1) == _lib.ERR_BAD_ARG and rc(H=0) == _lib.ERR_BAD_ARG


# ---- the Python boundary on host tensors
def test_python_boundary_errors_on_cpu_tensors(f3d):
    from f3dgaus_amd import losses
    assert f3d.losses is losses
    a, b = torch.rand(2, 3, 8, 8), torch.rand(2, 3, 8, 8)
    fns = (losses.ssim, losses.ssim_map, losses.l1_loss, losses.l2_loss, losses.psnr, losses.photometric_loss, losses.image_metrics)
    for fn in fns:
        with pytest.raises(RuntimeError, match="HIP device"):          # no CPU fallback
            fn(a, b)
        with pytest.raises(ValueError, match="shape"):
            fn(a, b[:, :, :7])
        with pytest.raises(TypeError, match="float32"):
            fn(a.double(), b.double())
        with pytest.raises(NotImplementedError, match="img2"):
            fn(a, b.clone().requires_grad_())
        with pytest.raises(ValueError):
            fn(a[0, 0], b[0, 0])                                        # no channel dim
    with torch.no_grad():                                               # a target that requires grad is fine where no graph is built
        with pytest.raises(RuntimeError, match="HIP device"):
            losses.ssim(a, b.clone().requires_grad_())
    with pytest.raises(ValueError, match="window_size"):
        losses.ssim(a, b, window_size=7)
    with pytest.raises(ValueError, match="reduction"):
        losses.photometric_loss(a, b, reduction="sum")
