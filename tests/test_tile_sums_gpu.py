"""GPU tests that pin the ORDER of the per-frame loss sums (csrc/f3dg_tile_sums.h): the sums f3dg_ssim_forward,
f3dg_geometry_loss_forward and f3dg_masked_l1_forward write are the bits of the numpy float32 restatement tests/tile_sums_truth.py,
through the C ABI and through f3dgaus_amd.losses. The other GPU tests hold the sums to float64 inside a rounding bound, which a
reordered sum passes too; tests/test_tile_sums_truth.py shows that these inputs tell the orders apart.

Pinned are the columns whose per-pixel term float32 numpy reproduces to the bit: both of the masked L1 (m |a - b|, m), 1 and 2 of SSIM
(|a - b|, (a - b)^2), 1, 2 and 4 of the geometry terms (distortion, m |d - target|, |alpha - target|). SSIM's column 0 and the
geometry columns 0 and 3 go through divides and square roots and stay with their float64 bars.

Shapes: 2 frames (SSIM: planes) of 120 x 260 -- 72 tiles a frame, so lanes 0..7 of the second stage take a second slot; right tiles
4 pixels wide; bottom tiles 8 high, every thread's second row outside the image -- and (1, 3, 5), one nearly empty tile."""
import ctypes as C

import pytest
import torch

from f3dgaus_amd import _lib, losses
import epilogue_truth as E
import tile_sums_truth as T

pytestmark = pytest.mark.gpu
CFG = {"model": {"fov": E.FOV_DEG}}


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _nan(dev, *shape):
    return torch.full(shape, float("nan"), device=dev)


def _pinned(got, sums, label):
    """The kernel's columns against the restatement's, to the bit."""
    got = got.cpu()
    for col, want in sorted(sums.items()):
        print(f"{label} col {col}: kernel {got[:, col].tolist()}  restated {want.tolist()}")
        assert torch.equal(got[:, col], torch.from_numpy(want)), (label, col)


def _ssim_raw(a, b):
    """f3dg_ssim_forward with the sums alone (no map, no derivative planes); partials and sums start as NaN."""
    n, H, W = a.shape
    L = _lib.lib()
    nbytes = L.f3dg_ssim_partials_bytes(n, W, H)
    partials, sums = _nan(a.device, nbytes // 4), _nan(a.device, n, 3)
    rc = L.f3dg_ssim_forward(_stream(), n, W, H, _lib.ptr(a), _lib.ptr(b), None, None, None, None, _lib.ptr(partials), nbytes, _lib.ptr(sums))
    assert rc == _lib.OK, rc
    torch.cuda.synchronize()
    return sums


@pytest.mark.parametrize("shape", T.SHAPES)
def test_ssim_sums_are_the_restatement(gpu_device, shape):
    (a, b), _, sums = T.case("ssim", shape)
    a, b = torch.from_numpy(a).to(gpu_device), torch.from_numpy(b).to(gpu_device)
    got = _ssim_raw(a, b)
    _pinned(got, sums, f"ssim {shape} C ABI")
    # losses: l1_loss / l2_loss are (the sum of the plane sums) / n -- two planes at most here, and one float32 addition has no order;
    # the same two torch operations on the restated plane sums, on the same device
    for fn, col in ((losses.l1_loss, 1), (losses.l2_loss, 2)):
        want = torch.from_numpy(sums[col]).to(gpu_device).sum() / float(a.numel())
        assert torch.equal(fn(a.unsqueeze(1), b.unsqueeze(1)), want), (fn.__name__, shape)
    if shape[0] > 1:
        assert torch.equal(_ssim_raw(a[1:].contiguous(), b[1:].contiguous())[0], got[1])


def _geometry_dev(f, dev, frames=slice(None)):
    pick = lambda t: t[frames].to(dev).contiguous()
    return dict(raster=pick(f["raster"]), wv=pick(f["world_view"]), depth_target=pick(f["depth_target"]), normal_target=pick(f["normal_target"]),
                alpha_target=pick(f["alpha_target"]), mask=pick(f["mask"]))


def _geometry_raw(f, d):
    F, _, H, W = d["raster"].shape
    fx, fy = E.focal(f)
    L = _lib.lib()
    nbytes = L.f3dg_geometry_loss_partials_bytes(F, W, H)
    partials, sums = _nan(d["raster"].device, nbytes // 4), _nan(d["raster"].device, F, 5)
    rc = L.f3dg_geometry_loss_forward(_stream(), F, H, W, _lib.ptr(d["raster"]), _lib.ptr(d["wv"]), float(fx), float(fy), 1, _lib.ptr(d["depth_target"]),
                                      _lib.ptr(d["normal_target"]), _lib.ptr(d["alpha_target"]), _lib.ptr(d["mask"]), _lib.ptr(partials), nbytes,
                                      _lib.ptr(sums))
    assert rc == _lib.OK, rc
    torch.cuda.synchronize()
    return sums


@pytest.mark.parametrize("shape", T.SHAPES)
def test_geometry_sums_are_the_restatement(gpu_device, shape):
    f, _, sums = T.case("geometry", shape)
    d = _geometry_dev(f, gpu_device)
    got = _geometry_raw(f, d)
    assert bool(torch.isfinite(got).all())
    _pinned(got, sums, f"geometry {shape} C ABI")
    api = losses.geometry_sums(d["raster"], d["wv"].reshape(-1, 4, 4), CFG, alpha_weight=True, depth_target=d["depth_target"],
                               normal_target=d["normal_target"], alpha_target=d["alpha_target"], mask=d["mask"])
    assert torch.equal(api, got)
    if shape[0] > 1:
        assert torch.equal(_geometry_raw(f, _geometry_dev(f, gpu_device, slice(1, 2)))[0], got[1])


def _masked_l1_raw(a, b, m):
    F, Cn, H, W = a.shape
    L = _lib.lib()
    nbytes = L.f3dg_masked_l1_partials_bytes(F, Cn, W, H)
    partials, sums = _nan(a.device, nbytes // 4), _nan(a.device, F, 2)
    rc = L.f3dg_masked_l1_forward(_stream(), F, Cn, H, W, _lib.ptr(a), _lib.ptr(b), _lib.ptr(m), _lib.ptr(partials), nbytes, _lib.ptr(sums))
    assert rc == _lib.OK, rc
    torch.cuda.synchronize()
    return sums


@pytest.mark.parametrize("shape", T.SHAPES)
def test_masked_l1_sums_are_the_restatement(gpu_device, shape):
    inputs, _, sums = T.case("masked_l1", shape)
    a, b, m = (torch.from_numpy(x).to(gpu_device) for x in inputs)
    got = _masked_l1_raw(a, b, m)
    _pinned(got, sums, f"masked L1 {shape} C ABI")
    assert torch.equal(losses.warping_sums(a, b, m), got)
    if shape[0] > 1:
        assert torch.equal(_masked_l1_raw(a[1:].contiguous(), b[1:].contiguous(), m[1:].contiguous())[0], got[1])
