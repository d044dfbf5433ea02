"""The render epilogue's backward kernel (f3dg_render_epilogue_backward) against the float64 autograd of the torch restatement of the
reference's lines (tests/epilogue_truth.py), by the tolerance rule stated there, and its structural promises: it ADDS into channels
3..5 and 6 of dL_dpix and touches no other channel, a NULL cotangent is a zero cotangent, two runs are bit-identical.

Shapes: V = 3 at 20 x 35 (700 pixels: two full workgroups and a partial one, odd width), 3 x 3 (a single interior pixel),
2 x 5 (no interior pixel: the depth channel gets exactly nothing)."""
import ctypes as C

import pytest
import torch

import f3dgaus_amd as f3d
from f3dgaus_amd import _lib
from f3dgaus_amd.gaussian_renderer import _epilogue_autograd
import epilogue_truth as T

gpu = pytest.mark.gpu
SHAPES = [(3, 20, 35), (1, 3, 3), (1, 2, 5)]
_CACHE = {}


def _case(shape):
    """(fixture, g32, g64) of a shape: computed once, never modified."""
    if shape not in _CACHE:
        f = T.make_fixture(*shape)
        _CACHE[shape] = (f, T.restatement_grads(f, torch.float32), T.restatement_grads(f, torch.float64))
    return _CACHE[shape]


def _kernel(f, dev, g_normal="fixture", g_depth="fixture", dpix=None):
    """dL_dpix after the call (a clone of ``dpix``, zeros by default)."""
    V, _, H, W = f["raster"].shape
    fx, fy = T.focal(f)
    gn = f["g_normal"].to(dev).contiguous() if isinstance(g_normal, str) else g_normal
    gd = f["g_depth_normal"].to(dev).contiguous() if isinstance(g_depth, str) else g_depth
    out = torch.zeros(V, 9, H, W, device=dev) if dpix is None else dpix.to(dev).clone().contiguous()
    ras, wv = f["raster"].to(dev).contiguous(), f["world_view"].to(dev).contiguous()
    rc = _lib.lib().f3dg_render_epilogue_backward(C.c_void_p(torch.cuda.current_stream().cuda_stream), V, H, W, _lib.ptr(ras), _lib.ptr(wv),
                                                  float(fx), float(fy), _lib.ptr(gn), _lib.ptr(gd), _lib.ptr(out))
    assert rc == _lib.OK, rc
    torch.cuda.synchronize()
    return out


def test_restatement_is_the_renderers_float32_formulation(f3d):
    """The truth's float32 forward is, to the bit, ``gaussian_renderer._epilogue_autograd`` (the reference's lines in torch ops) on the host."""
    f = T.make_fixture(2, 20, 35)
    for v in range(2):
        a = T.epilogue_torch(f["raster"][v], f["world_view"][v], 35, 20, f["FoVx"], f["FoVy"])
        b = _epilogue_autograd(f["raster"][v], f["world_view"][v], 35, 20, f["FoVx"], f["FoVy"])
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
        assert float(a[1][:, 1:-1, 1:-1].abs().max()) > 0 and float(a[1][:, 0].abs().max()) == 0.0


def test_fixture_is_well_conditioned_on_the_host():
    """E_ref of the fixture at the tests' shapes, on the CPU: float32 autograd of the restatement within 1e-5 of the float64 one, so the
    4 * E_ref bound means something (no division by a vanishing norm or cross product anywhere in the frame)."""
    for shape in SHAPES:
        f, g32, g64 = _case(shape)
        for name, sl in T.GROUPS.items():
            m = float(g64[:, sl].abs().max())
            if name == "depth" and shape[1] < 3:
                assert m == 0.0
                continue
            e = float((g32[:, sl].double() - g64[:, sl]).abs().max()) / m
            print(f"{shape} {name}: max|g64| {m:.3e}  E_ref {e:.3e}")
            assert 0 < e < 1e-5, (shape, name, e)


@gpu
@pytest.mark.parametrize("shape", SHAPES)
def test_kernel_against_the_float64_restatement(gpu_device, shape):
    f, g32, g64 = _case(shape)
    got = _kernel(f, gpu_device)
    assert bool(torch.isfinite(got).all())
    T.check_groups(got, g32, g64, label=f"epilogue bwd {shape}")
    for c in (0, 1, 2, 7, 8):
        assert float(got[:, c].abs().max()) == 0.0, c
    if shape[1] < 3:
        assert float(got[:, 6].abs().max()) == 0.0
    else:       # border pixels are no centres, but they do receive from their interior neighbours
        assert float(got[:, 6, 0, 1:-1].abs().max()) > 0 and float(got[:, 6, 1:-1, 0].abs().max()) > 0
        for y, x in ((0, 0), (0, -1), (-1, 0), (-1, -1)):       # a corner has no interior axial neighbour
            assert float(got[:, 6, y, x].abs().max()) == 0.0


@gpu
def test_kernel_adds_and_leaves_the_other_channels_alone(gpu_device):
    f, _, _ = _case(SHAPES[0])
    V, _, H, W = f["raster"].shape
    base = torch.randn(V, 9, H, W, generator=torch.Generator().manual_seed(3)).to(gpu_device)
    fresh = _kernel(f, gpu_device)
    added = _kernel(f, gpu_device, dpix=base)
    for c in (0, 1, 2, 7, 8):
        assert torch.equal(added[:, c], base[:, c]), c
    assert torch.equal(added[:, 3:7], base[:, 3:7] + fresh[:, 3:7])      # one float32 addition per element
    assert not torch.equal(added[:, 3:7], base[:, 3:7])


@gpu
def test_null_cotangent_is_a_zero_cotangent(gpu_device):
    f, _, _ = _case(SHAPES[0])
    zero = torch.zeros_like(f["g_normal"]).to(gpu_device)
    both = _kernel(f, gpu_device)
    only_n, only_d = _kernel(f, gpu_device, g_depth=None), _kernel(f, gpu_device, g_normal=None)
    assert torch.equal(only_n, _kernel(f, gpu_device, g_depth=zero)) and torch.equal(only_d, _kernel(f, gpu_device, g_normal=zero))
    assert torch.equal(only_n[:, 3:6], both[:, 3:6]) and float(only_n[:, 6].abs().max()) == 0.0
    assert torch.equal(only_d[:, 6], both[:, 6]) and float(only_d[:, 3:6].abs().max()) == 0.0
    base = torch.randn(both.shape, generator=torch.Generator().manual_seed(4)).to(gpu_device)
    assert torch.equal(_kernel(f, gpu_device, g_normal=None, g_depth=None, dpix=base), base)       # nothing to add: nothing touched


@gpu
def test_bit_reproducible(gpu_device):
    f, _, _ = _case(SHAPES[0])
    assert torch.equal(_kernel(f, gpu_device), _kernel(f, gpu_device))


@gpu
def test_clamped_normal_and_constant_depth_patch(gpu_device):
    """A pixel whose accumulated normal is exactly 0: F.normalize's clamp_min(1e-12) is active and torch hands the cotangent on as
    g / 1e-12 -- compared on its own, relative to its own maximum, with the normal group's bound over the ordinary pixels. An interior
    pixel on a constant-depth patch of a frontal camera: its cross product is finite (the rays differ), so the ordinary rule holds."""
    f0, _, _ = _case(SHAPES[0])
    f = dict(f0)
    f["raster"] = f0["raster"].clone()
    f["world_view"] = f0["world_view"].clone()
    zv, zy, zx = 1, 7, 12
    f["raster"][zv, 3:6, zy, zx] = 0.0
    f["world_view"][2] = torch.eye(4)                   # frontal: camera frame = world frame
    f["raster"][2, 6, 9:14, 20:25] = 2.0                # constant depth around the interior pixel (11, 22)
    g32, g64 = T.restatement_grads(f, torch.float32), T.restatement_grads(f, torch.float64)
    got = _kernel(f, gpu_device)
    assert bool(torch.isfinite(got).all())
    keep = torch.ones_like(g64, dtype=torch.bool)
    keep[zv, 3:6, zy, zx] = False
    # the ordinary pixels: the clamped pixel's 1e12-scaled values are taken out of all three arrays
    mask = lambda t: torch.where(keep, t.double().cpu(), torch.zeros((), dtype=torch.float64))
    fig = T.check_groups(mask(got), mask(g32), mask(g64), label="clamp/others")
    # (as for the splat head's degenerate quaternions: three values are too few for a stable worst case of their own, so the bound is
    # 4 * max(E_ref of that pixel, E_ref of the normal group over the ordinary pixels))
    t64, t32, tk = g64[zv, 3:6, zy, zx], g32[zv, 3:6, zy, zx].double(), got[zv, 3:6, zy, zx].double().cpu()
    m = float(t64.abs().max())
    e_pix, err = float((t32 - t64).abs().max()) / m, float((tk - t64).abs().max()) / m
    print(f"clamp/zero normal: max|g64| {m:.3e}  E_ref(pixel) {e_pix:.3e}  E_ref(group) {fig['normal'][0]:.3e}  kernel {err:.3e}")
    assert m > 1e10 and err <= 4 * max(e_pix, fig["normal"][0]), (m, err)
    assert float(g64[2, 6, 10:13, 21:24].abs().max()) > 0 and float(g64[2, 6].abs().max()) < 1e6     # finite cross product on the patch
