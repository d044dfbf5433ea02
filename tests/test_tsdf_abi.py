"""The TSDF entries' host side (no GPU): every refusal of include/f3dg.h is found before any HIP call, the workspace arithmetic, the
symbols and the capacity constant."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN, INF = float("nan"), float("inf")


@pytest.fixture(scope="module")
def env(f3d):
    from f3dgaus_amd import _lib
    buf = (C.c_char * 4096)()
    one = C.c_void_p((C.addressof(buf) + 255) & ~255)          # a 256-byte aligned non-NULL pointer nothing dereferences
    return _lib, _lib.lib(), one, (C.c_float * 3)(0.0, 0.0, 0.0)


def _integrate(L, one, origin0, **kw):
    a = dict(nx=8, ny=8, nz=8, origin=origin0, voxel=0.1, trunc=0.4, z_near=0.05, n_views=2, H=16, W=16, depth=one, color=one, alpha=one,
             alpha_min=0.5, world_view=one, fx=20.0, fy=20.0, tsdf=one, weight=one, color_out=one, color_weight=one)
    a.update(kw)
    return L.f3dg_tsdf_integrate(None, a["nx"], a["ny"], a["nz"], a["origin"], a["voxel"], a["trunc"], a["z_near"], a["n_views"], a["H"], a["W"],
                                 a["depth"], a["color"], a["alpha"], a["alpha_min"], a["world_view"], a["fx"], a["fy"], a["tsdf"], a["weight"],
                                 a["color_out"], a["color_weight"])


def test_symbols_are_bound_and_the_capacity_matches_the_header(env):
    _lib, L, _, _ = env
    for name in ("f3dg_tsdf_integrate", "f3dg_tsdf_cells_workspace_bytes", "f3dg_tsdf_cells_count", "f3dg_tsdf_cells_emit", "f3dg_tsdf_vertices"):
        assert name in _lib.SIGNATURES and hasattr(L, name)
    text = open(os.path.join(ROOT, "include", "f3dg.h")).read()
    assert int(re.search(r"#define F3DG_TSDF_MAX_VIEWS\s+(\d+)", text).group(1)) == _lib.TSDF_MAX_VIEWS == 128


def test_integrate_refusals(env):
    _lib, L, one, origin = env
    bad = _lib.ERR_BAD_ARG
    for name in ("origin", "depth", "world_view", "tsdf", "weight"):
        assert _integrate(L, one, origin, **{name: None}) == bad, name
    assert _integrate(L, one, origin, color_out=None) == bad and _integrate(L, one, origin, color_weight=None) == bad    # a colour needs both
    for name in ("nx", "ny", "nz", "n_views", "H", "W"):
        for v in (0, -3):
            assert _integrate(L, one, origin, **{name: v}) == bad, (name, v)
    for name in ("voxel", "trunc", "fx", "fy"):
        for v in (0.0, -1.0, NAN, INF):
            assert _integrate(L, one, origin, **{name: v}) == bad, (name, v)
    for v in (-0.1, NAN, INF):
        assert _integrate(L, one, origin, z_near=v) == bad, v
    assert _integrate(L, one, origin, alpha_min=NAN) == bad
    for v in (NAN, INF, -INF):
        assert _integrate(L, one, origin, origin=(C.c_float * 3)(0.0, v, 0.0)) == bad, v
    # 2^31 voxels and beyond, and images of 2^31 pixels, are unsupported
    assert _integrate(L, one, origin, nx=2048, ny=1024, nz=1024) == _lib.ERR_UNSUPPORTED
    assert _integrate(L, one, origin, nx=1 << 16, ny=1 << 16, nz=4) == _lib.ERR_UNSUPPORTED
    assert _integrate(L, one, origin, H=1 << 16, W=1 << 15) == _lib.ERR_UNSUPPORTED


def test_cells_refusals_and_workspace_arithmetic(env):
    _lib, L, one, origin = env
    bad = _lib.ERR_BAD_ARG
    wsb = L.f3dg_tsdf_cells_workspace_bytes
    # header 256 B + one bit per cell (whole 64-bit words) + one count per 256 cells (whole groups of 16), each rounded to 256 B
    r256 = lambda b: (b + 255) // 256 * 256
    for nx, ny, nz in ((2, 2, 2), (37, 21, 19), (256, 256, 256), (3, 2, 1000)):
        cells = (nx - 1) * (ny - 1) * (nz - 1)
        blocks = (cells + 255) // 256
        assert wsb(nx, ny, nz) == 256 + r256((cells + 63) // 64 * 8) + r256((blocks + 15) // 16 * 16 * 4), (nx, ny, nz)
    assert wsb(1, 8, 8) == 0 and wsb(8, 1, 8) == 0 and wsb(8, 8, 1) == 0 and wsb(0, 8, 8) == 0 and wsb(-2, 8, 8) == 0      # a dimension below 2
    assert wsb(2048, 1024, 1024) == 0
    n = C.c_longlong(-7)
    count = lambda **kw: L.f3dg_tsdf_cells_count(None, kw.get("nx", 8), kw.get("ny", 8), kw.get("nz", 8), kw.get("min_weight", 1.0), kw.get("tsdf", one),
                                                kw.get("weight", one), kw.get("ws", one), kw.get("bytes", 1 << 20), kw.get("out", C.byref(n)))
    for name in ("tsdf", "weight", "ws", "out"):
        assert count(**{name: None}) == bad, name
    assert count(min_weight=NAN) == bad
    for name in ("nx", "ny", "nz"):
        for v in (1, 0, -1):
            assert count(**{name: v}) == bad, (name, v)
    assert count(nx=2048, ny=1024, nz=1024) == _lib.ERR_UNSUPPORTED
    assert count(bytes=wsb(8, 8, 8) - 1) == _lib.ERR_WORKSPACE
    assert count(ws=C.c_void_p(one.value + 4)) == bad                      # off the 16-byte grid
    assert n.value == -7                                                    # a refused call writes nothing
    emit = lambda **kw: L.f3dg_tsdf_cells_emit(None, kw.get("nx", 8), kw.get("ny", 8), kw.get("nz", 8), kw.get("ws", one), kw.get("bytes", 1 << 20),
                                              kw.get("n", 5), kw.get("tets", one))
    assert emit(ws=None) == bad and emit(tets=None) == bad and emit(n=0) == bad and emit(n=-1) == bad
    assert emit(nx=1) == bad and emit(nz=0) == bad
    assert emit(bytes=wsb(8, 8, 8) - 1) == _lib.ERR_WORKSPACE
    assert emit(tets=C.c_void_p(one.value + 8)) == bad
    assert emit(nx=2048, ny=1024, nz=1024) == _lib.ERR_UNSUPPORTED


def test_vertices_refusals(env):
    _lib, L, one, origin = env
    bad = _lib.ERR_BAD_ARG
    call = lambda **kw: L.f3dg_tsdf_vertices(None, kw.get("nx", 8), kw.get("ny", 8), kw.get("nz", 8), kw.get("origin", origin), kw.get("voxel", 0.1),
                                            kw.get("E", 10), kw.get("interp_v", one), kw.get("tsdf", one), kw.get("color", one),
                                            kw.get("color_weight", one), kw.get("vertices", one), kw.get("vertex_colors", one))
    for name in ("origin", "interp_v", "tsdf", "vertices"):
        assert call(**{name: None}) == bad, name
    assert call(color=None) == bad and call(color_weight=None) == bad      # vertex colours need the volume's colour
    assert call(E=0) == bad and call(E=-4) == bad
    for v in (0.0, -1.0, NAN, INF):
        assert call(voxel=v) == bad, v
    assert call(origin=(C.c_float * 3)(NAN, 0.0, 0.0)) == bad
    for name in ("nx", "ny", "nz"):
        assert call(**{name: 0}) == bad, name
    assert call(nx=2048, ny=1024, nz=1024) == _lib.ERR_UNSUPPORTED


def test_python_api_refuses_host_tensors_without_a_gpu(f3d):
    import torch
    with pytest.raises(RuntimeError, match="HIP device"):
        f3d.tsdf.TSDFVolume((0, 0, 0), 0.1, (8, 8, 8), device="cpu")
    assert f3d.TSDFVolume is f3d.tsdf.TSDFVolume and callable(f3d.mesh.extract_mesh_tsdf) and f3d.extract_mesh_tsdf is f3d.mesh.extract_mesh_tsdf
    with pytest.raises(RuntimeError, match="HIP device"):
        f3d.mesh.extract_mesh_tsdf({"xyz": torch.zeros(1, 4, 3)}, 0, torch.eye(4)[None], None, None, None, {"model": {"fov": 10.0}})
