"""The mesh rasteriser's host side (no GPU): the symbols, the workspace arithmetic, every refusal of include/f3dg.h found before any HIP
call with nothing written to h_counts, and the Python entries' refusal of host tensors and of vertices that require grad."""
import ctypes as C
import inspect
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("f3dg_mesh_raster_workspace_bytes", "f3dg_mesh_raster")
BIG = 1 << 31


@pytest.fixture(scope="module")
def env(f3d):
    from f3dgaus_amd import _lib
    buf = (C.c_char * 16384)()
    one = C.c_void_p((C.addressof(buf) + 255) & ~255)          # 256-byte aligned non-NULL pointers nothing dereferences
    return _lib, _lib.lib(), [C.c_void_p(one.value + 1024 * k) for k in range(10)], buf


def test_symbols_are_declared_exported_and_bound(env):
    _lib, L, _, _ = env
    text = open(os.path.join(ROOT, "include", "f3dg.h")).read()
    raw = C.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert re.search(r"\b(int|size_t)\s+%s\(" % name, text), name
        assert name in _lib.SIGNATURES and hasattr(L, name)
        assert getattr(raw, name) is not None, name
    sig = _lib.SIGNATURES["f3dg_mesh_raster"][1]
    assert len(sig) == 23 and sig[-1] is C.POINTER(C.c_longlong)
    assert sig[10:12] == [C.c_double, C.c_double] and sig[14] is C.c_double       # fx, fy and z_near travel as doubles
    for name, value in (("NONE", 0), ("BACK", 1), ("FRONT", 2)):
        assert re.search(r"#define F3DG_RASTER_CULL_%s %d\b" % (name, value), text)
    assert _lib.RASTER_CULL == {"none": 0, "back": 1, "front": 2}


def test_workspace_bytes(env):
    _, L, _, _ = env
    wb = L.f3dg_mesh_raster_workspace_bytes
    r256 = lambda b: (b + 255) // 256 * 256
    for V, F, H, W in ((1, 0, 1, 1), (1, 1, 1, 1), (3, 320, 29, 33), (8, 1_000_003, 256, 256), (1, 5, 16384, 16384), (32, 67_108_863, 512, 512),
                       (BIG - 1, 1, 1, 1), (1, BIG - 1, 7, 5)):
        # a header of 256 B + one 64-bit key per pixel + one 32-bit queue slot per (view, face) pair
        assert wb(V, F, H, W) == 256 + r256(8 * V * H * W) + r256(4 * V * F), (V, F, H, W)
    sizes = (1, 2, 17, 1000, 4097)
    for a, b in zip(sizes, sizes[1:]):                             # positive and monotone in every size
        assert 0 < wb(a, 9, 8, 8) <= wb(b, 9, 8, 8) and 0 < wb(2, a, 8, 8) <= wb(2, b, 8, 8)
        assert 0 < wb(2, 9, a, 8) <= wb(2, 9, b, 8) and 0 < wb(2, 9, 8, a) <= wb(2, 9, 8, b)
    for V, F, H, W in ((0, 5, 8, 8), (-1, 5, 8, 8), (1, -1, 8, 8), (1, 5, 0, 8), (1, 5, 8, 0), (1, 5, 8, -3), (1, 5, 16385, 8), (1, 5, 8, 16385),
                       (1, BIG, 8, 8), (BIG, 1, 1, 1), (8, 5, 16384, 16384), (2, 1 << 30, 8, 8), (1 << 40, 1, 1, 1), (1, 1 << 62, 1, 1)):
        assert wb(V, F, H, W) == 0, (V, F, H, W)


def test_refusals_write_nothing(env):
    _lib, L, p, _ = env
    bad, uns = _lib.ERR_BAD_ARG, _lib.ERR_UNSUPPORTED
    h = (C.c_longlong * 7)(*([-7] * 7))
    need = L.f3dg_mesh_raster_workspace_bytes(3, 50, 29, 33)

    def call(**kw):
        a = dict(ws=p[0], bytes=1 << 30, N=100, F=50, v=p[1], faces=p[2], is32=0, V=3, wv=p[3], fx=28.0, fy=25.0, H=29, W=33, z_near=0.01,
                 cull=0, C=6, attrs=p[4], face_id=p[5], depth=p[6], bary=p[7], out=p[8], h=h)
        a.update(kw)
        return L.f3dg_mesh_raster(None, a["ws"], a["bytes"], a["N"], a["F"], a["v"], a["faces"], a["is32"], a["V"], a["wv"], a["fx"], a["fy"],
                                  a["H"], a["W"], a["z_near"], a["cull"], a["C"], a["attrs"], a["face_id"], a["depth"], a["bary"], a["out"], a["h"])
    for name in ("ws", "v", "faces", "wv", "face_id", "depth", "bary", "h", "attrs", "out"):
        assert call(**{name: None}) == bad, name
    assert call(C=0) == bad and call(C=9) == bad and call(C=-1) == bad and call(C=3, attrs=None, out=None) == bad
    assert call(N=0) == bad and call(N=-4) == bad and call(F=-1) == bad and call(V=0) == bad and call(H=0) == bad and call(W=-2) == bad
    for name in ("fx", "fy", "z_near"):
        for value in (0.0, -1.0, float("nan"), float("inf")):
            assert call(**{name: value}) == bad, (name, value)
    assert call(cull=3) == bad and call(cull=-1) == bad
    assert call(ws=C.c_void_p(p[0].value + 8)) == bad                                # off the 16-byte grid
    assert call(N=BIG) == uns and call(F=BIG) == uns and call(H=16385) == uns and call(W=16385) == uns
    assert call(V=8, H=16384, W=16384) == uns and call(V=64, F=1 << 25) == uns
    assert call(bytes=need - 1) == _lib.ERR_WORKSPACE and call(bytes=0) == _lib.ERR_WORKSPACE
    assert list(h) == [-7] * 7                                                       # a refused call writes nothing


def test_python_entries_refuse_host_tensors_and_gradients(f3d):
    import torch
    assert f3d.render_mesh is f3d.mesh.render_mesh and f3d.mesh_depth_agreement is f3d.mesh.mesh_depth_agreement
    assert f3d.interpolate_vertex_attributes is f3d.mesh.interpolate_vertex_attributes
    faces, v, wv = torch.tensor([[0, 1, 2]]), torch.rand(3, 3), torch.eye(4)[None]
    with pytest.raises(RuntimeError, match="HIP device"):
        f3d.mesh.render_mesh(v, faces, wv, 50.0, 32)
    with pytest.raises(NotImplementedError, match="produces no gradient for `vertices`"):
        f3d.mesh.render_mesh(v.clone().requires_grad_(), faces, wv, 50.0, 32)
    with pytest.raises(RuntimeError, match="HIP device"):
        f3d.mesh.interpolate_vertex_attributes(v, faces, torch.zeros(1, 4, 4, dtype=torch.int32), torch.zeros(1, 3, 4, 4))
    with pytest.raises(RuntimeError, match="HIP device"):
        f3d.mesh.mesh_depth_agreement(*(torch.zeros(1, 4, 4) for _ in range(4)))
    p = inspect.signature(f3d.mesh.render_mesh).parameters
    assert [k for k in p][:5] == ["vertices", "faces", "world_views", "fov", "resolution"]
    assert all(p[k].kind is inspect.Parameter.KEYWORD_ONLY for k in ("vertex_colors", "vertex_normals", "cull", "z_near"))
    assert (p["vertex_colors"].default, p["vertex_normals"].default, p["cull"].default, p["z_near"].default) == (None, None, "none", 0.01)
    assert inspect.signature(f3d.mesh.mesh_depth_agreement).parameters["alpha_min"].default == 0.5
