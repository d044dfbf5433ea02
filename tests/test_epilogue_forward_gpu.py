"""The render epilogue's forward kernels (epilogue_kernel<true> behind f3dg_render_epilogue_view and the Python wrappers,
epilogue_kernel<false> behind f3dg_render_epilogue) against float64 on their own inputs, element by element (truth,
scales, condition number and cases: tests/epilogue_truth.py, proven on the host by tests/test_epilogue_forward_truth.py).

    K = |x - truth| / (2^-24 A);  per group, pooled over the ordinary cases: the kernel's median, p99 and max of K each <= 4 x the float32
    restatement's on the same inputs; every case alone: max K <= 4 x the restatement's pooled max.

Every output starts as a NaN sentinel bit pattern, so a skipped element shows; every figure is printed before it is asserted."""
import ctypes as C
import math

import pytest
import torch

import f3dgaus_amd as f3d
from f3dgaus_amd import _lib
from f3dgaus_amd.gaussian_renderer import _epilogue
import epilogue_truth as T
import forward_bars as FB

pytestmark = pytest.mark.gpu
CASES = tuple(T.forward_cases())
POOLED = tuple(n for n in CASES if T.forward_cases()[n]["pooled"])
SENTINEL = 0x7FC0BEEF


def _bits(t):
    return t.contiguous().view(torch.int32)


def _sentinel(V, H, W, dev):
    t = torch.empty(V, 3, H, W, dtype=torch.float32, device=dev)
    t.view(torch.int32).fill_(SENTINEL)
    return t


def _raw(case, dev, given_c2w=False, want_normal=True, want_depth_normal=True, raster=None):
    """f3dg_render_epilogue_view (or, ``given_c2w``, f3dg_render_epilogue on the case's float32 c2w) through ctypes into
    sentinel-filled outputs; a map that is not wanted goes in as NULL and comes back as None."""
    ras = (case["raster"] if raster is None else raster).to(dev).contiguous()
    V, _, H, W = ras.shape
    assert (H, W) == (case["H"], case["W"]) and ras.dtype == torch.float32
    mat = (case["c2w"] if given_c2w else case["world_view"]).to(dev).contiguous()
    assert mat.numel() == 16 * V and mat.dtype == torch.float32
    fx, fy = case["W"] / (2 * math.tan(case["FoVx"] / 2.)), case["H"] / (2 * math.tan(case["FoVy"] / 2.))
    nw = _sentinel(V, H, W, dev) if want_normal else None
    dn = _sentinel(V, H, W, dev) if want_depth_normal else None
    fn = _lib.lib().f3dg_render_epilogue if given_c2w else _lib.lib().f3dg_render_epilogue_view
    rc = fn(C.c_void_p(torch.cuda.current_stream().cuda_stream), V, H, W, _lib.ptr(ras), _lib.ptr(mat), float(fx), float(fy), _lib.ptr(nw), _lib.ptr(dn))
    assert rc == _lib.OK, rc
    torch.cuda.synchronize()
    return nw, dn


@pytest.mark.parametrize("given_c2w", [False, True], ids=["from_view", "c2w_given"])
def test_every_element_against_float64(gpu_device, given_c2w):
    """All cases through one entry point: the bars per group, borders and exact-zero pixels exactly 0, zero normals exactly 0."""
    k_ker, k_ref, bad = {}, {}, []
    for name in CASES:
        tr, ks_ref, bad_ref, _ = T.case_truth(name, given_c2w)
        assert not bad_ref, bad_ref
        nw, dn = (t.cpu() for t in _raw(T.forward_cases()[name], gpu_device, given_c2w))
        assert not bool((_bits(nw) == SENTINEL).any()) and not bool((_bits(dn) == SENTINEL).any()), (name, "an element was not written")
        assert float(dn[:, :, 0].abs().max()) == 0 and float(dn[:, :, -1].abs().max()) == 0, name
        assert float(dn[:, :, :, 0].abs().max()) == 0 and float(dn[:, :, :, -1].abs().max()) == 0, name
        k_ker[name], b = T.forward_K(nw, dn, tr, name)
        k_ref[name] = ks_ref
        bad += b
    label = "epilogue (c2w given)" if given_c2w else "epilogue (from view)"
    broken = FB.hold_to_bars(k_ker, k_ref, POOLED, label)
    print("rules:", bad, "\nbars:", broken)
    assert not bad and not broken, (bad, broken)


def test_null_outputs_wrappers_and_out_reuse(gpu_device):
    """With one output NULL the other is bit-identical to the two-output run, through both entry points; the Python wrapper, its out=
    reuse and depth_to_normal return the raw call's bits."""
    dev = gpu_device
    case = T.forward_cases()["17x33_fov"]
    for given in (False, True):
        nw, dn = _raw(case, dev, given)
        only_n, none_d = _raw(case, dev, given, want_depth_normal=False)
        none_n, only_d = _raw(case, dev, given, want_normal=False)
        assert none_d is None and none_n is None
        assert torch.equal(_bits(only_n), _bits(nw)) and torch.equal(_bits(only_d), _bits(dn)), given
    nw, dn = _raw(case, dev)
    args = (case["raster"].to(dev), case["world_view"].to(dev), case["W"], case["H"], case["FoVx"], case["FoVy"])
    w_nw, w_dn = _epilogue(*args)
    assert torch.equal(_bits(w_nw), _bits(nw)) and torch.equal(_bits(w_dn), _bits(dn))
    r_nw, r_dn = _sentinel(2, 17, 33, dev), _sentinel(2, 17, 33, dev)
    got = _epilogue(*args, out=(r_nw, r_dn))
    assert got[0] is r_nw and got[1] is r_dn and torch.equal(_bits(r_nw), _bits(nw)) and torch.equal(_bits(r_dn), _bits(dn))
    lean_nw, lean_dn = _epilogue(*args, want_normal=False)
    assert lean_nw is None and torch.equal(_bits(lean_dn), _bits(dn))
    r_dn2 = _sentinel(2, 17, 33, dev)
    assert _epilogue(*args, out=(None, r_dn2))[0] is None and torch.equal(_bits(r_dn2), _bits(dn))
    one = f3d.depth_to_normal(case["world_view"][1].to(dev), case["W"], case["H"], case["FoVx"], case["FoVy"], case["raster"][1, 6:7].to(dev))
    assert one.shape == (17, 33, 3) and torch.equal(_bits(one.permute(2, 0, 1)), _bits(dn[1]))


def test_a_nan_depth_reaches_its_axial_neighbours_only(gpu_device):
    """A NaN depth at one pixel: the depth normals of its axial neighbours that are interior pixels become NaN; every other depth
    normal, its own included, and every normal_world are bit-identical to the clean run. At an interior pixel, next to the border
    and in a corner."""
    case = T.forward_cases()["20x35"]
    V, _, H, W = case["raster"].shape
    for given in (False, True):
        nw0, dn0 = _raw(case, gpu_device, given)
        for v, y, x in ((1, 9, 17), (0, 1, 1), (2, 0, 0), (2, H - 1, 20)):
            ras = case["raster"].clone()
            ras[v, 6, y, x] = float("nan")
            nw, dn = _raw(case, gpu_device, given, raster=ras)
            assert torch.equal(_bits(nw), _bits(nw0)), (v, y, x, "a NaN depth reached normal_world")
            hit = torch.zeros(V, 3, H, W, dtype=torch.bool)
            for yy, xx in ((y - 1, x), (y + 1, x), (y, x - 1), (y, x + 1)):
                if 1 <= yy < H - 1 and 1 <= xx < W - 1:
                    hit[v, :, yy, xx] = True
            same = (_bits(dn) == _bits(dn0)).cpu()
            assert bool(same[~hit].all()), (v, y, x, "a NaN depth reached a pixel that does not read it")
            assert bool(torch.isnan(dn.cpu()[hit]).all()), (v, y, x, "a NaN depth did not arrive")
            assert int(hit.sum()) == 3 * {(9, 17): 4, (1, 1): 2, (0, 0): 0, (H - 1, 20): 1}[(y, x)]


def test_two_runs_are_bit_identical(gpu_device):
    for name in ("20x35", "background", "degenerate"):
        for given in (False, True):
            a, b = _raw(T.forward_cases()[name], gpu_device, given), _raw(T.forward_cases()[name], gpu_device, given)
            assert torch.equal(_bits(a[0]), _bits(b[0])) and torch.equal(_bits(a[1]), _bits(b[1])), (name, given)


def test_wrong_shapes_are_refused_on_the_device_and_a_valid_call_follows(gpu_device):
    """The wrappers raise before any launch (the checks themselves: tests/test_epilogue_forward_truth.py); a valid call right after
    gives the raw call's result."""
    dev = gpu_device
    case = T.forward_cases()["17x33_fov"]
    ras, wv = case["raster"].to(dev), case["world_view"].to(dev)
    fov = (case["FoVx"], case["FoVy"])
    with pytest.raises(ValueError, match="raster must be"):
        _epilogue(ras, wv, 17, 33, *fov)                                    # width and height exchanged
    with pytest.raises(ValueError, match="raster must be"):
        _epilogue(ras[:, :8], wv, 33, 17, *fov)
    with pytest.raises(ValueError, match="float32"):
        _epilogue(ras.half(), wv, 33, 17, *fov)
    with pytest.raises(ValueError, match="world_view"):
        _epilogue(ras, wv[:1], 33, 17, *fov)
    with pytest.raises(ValueError, match="out depth_normal"):
        _epilogue(ras, wv, 33, 17, *fov, out=(torch.empty(2, 3, 17, 33, device=dev), torch.empty(2, 3, 17, 32, device=dev)))
    with pytest.raises(RuntimeError, match="is on"):
        _epilogue(ras, wv, 33, 17, *fov, out=(torch.empty(2, 3, 17, 33), None))
    with pytest.raises(RuntimeError, match="HIP device"):
        _epilogue(ras.cpu(), wv, 33, 17, *fov)
    with pytest.raises(ValueError, match="depth must be"):
        f3d.depth_to_normal(wv[0], 32, 17, *fov, ras[0, 6:7])              # a depth map wider than the launch it would get
    with pytest.raises(ValueError, match="depth must be"):
        f3d.depth_to_normal(wv[0], 33, 18, *fov, ras[0, 6:7])
    nw, dn = _epilogue(ras, wv, 33, 17, *fov)
    raw = _raw(case, dev)
    assert torch.equal(_bits(nw), _bits(raw[0])) and torch.equal(_bits(dn), _bits(raw[1]))
