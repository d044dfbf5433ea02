"""The mesh clean-up entries' host side (no GPU): the symbols, the workspace arithmetic, every refusal of include/f3dg.h found before any HIP
call with nothing written to h_counts, and the Python entries' refusal of host tensors."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("f3dg_mesh_components_workspace_bytes", "f3dg_mesh_components", "f3dg_mesh_compact_workspace_bytes", "f3dg_mesh_compact_count",
         "f3dg_mesh_compact_emit")
BIG = 1 << 31


@pytest.fixture(scope="module")
def env(f3d):
    from f3dgaus_amd import _lib
    buf = (C.c_char * 4096)()
    one = C.c_void_p((C.addressof(buf) + 255) & ~255)          # a 256-byte aligned non-NULL pointer nothing dereferences
    return _lib, _lib.lib(), one, buf


def test_symbols_are_declared_exported_and_bound(env):
    _lib, L, _, _ = env
    text = open(os.path.join(ROOT, "include", "f3dg.h")).read()
    raw = C.CDLL(_lib.LIB_PATH)                                 # exported: the dynamic loader finds the symbol
    for name in NAMES:
        assert re.search(r"\b(int|size_t)\s+%s\(" % name, text), name
        assert name in _lib.SIGNATURES and hasattr(L, name)
        assert getattr(raw, name) is not None, name
    assert _lib.SIGNATURES["f3dg_mesh_components"][1][-1] is C.POINTER(C.c_longlong)


def test_workspace_arithmetic(env):
    _, L, _, _ = env
    r256 = lambda b: (b + 255) // 256 * 256
    up = lambda a, b: (a + b - 1) // b
    cc, mc = L.f3dg_mesh_components_workspace_bytes, L.f3dg_mesh_compact_workspace_bytes
    for N, F in ((1, 0), (3, 1), (64, 64), (65, 257), (4101, 4099), (1 << 20, 2_000_001), (BIG - 1, BIG - 1)):
        # components: header 256 B + one 32-bit parent per vertex
        assert cc(N, F) == 256 + r256(4 * N), (N, F)
        # compaction: header 256 B + one bit per face and per vertex (whole 64-bit words) + one count per 256 faces and per 256 vertices
        # (whole groups of 16), each rounded to 256 B
        want = 256 + r256(up(F, 64) * 8) + r256(up(N, 64) * 8) + r256(up(up(F, 256), 16) * 16 * 4) + r256(up(up(N, 256), 16) * 16 * 4)
        assert mc(N, F) == want, (N, F)
    for N, F in ((0, 5), (-1, 5), (5, -1), (BIG, 5), (5, BIG), (1 << 40, 1)):
        assert cc(N, F) == 0 and mc(N, F) == 0, (N, F)


def _sentinel():
    return (C.c_longlong * 4)(-7, -7, -7, -7)


def test_components_refusals(env):
    _lib, L, one, _ = env
    bad = _lib.ERR_BAD_ARG
    h = _sentinel()

    def call(**kw):
        a = dict(ws=one, bytes=1 << 20, N=100, F=50, faces=one, is32=0, fc=one, cf=one, h=h)
        a.update(kw)
        return L.f3dg_mesh_components(None, a["ws"], a["bytes"], a["N"], a["F"], a["faces"], a["is32"], a["fc"], a["cf"], a["h"])
    for name in ("ws", "faces", "fc", "cf", "h"):
        assert call(**{name: None}) == bad, name
    assert call(N=0) == bad and call(N=-4) == bad and call(F=-1) == bad
    assert call(ws=C.c_void_p(one.value + 8)) == bad                      # off the 16-byte grid
    assert call(N=BIG) == _lib.ERR_UNSUPPORTED and call(F=BIG) == _lib.ERR_UNSUPPORTED and call(N=1 << 40, F=1 << 33) == _lib.ERR_UNSUPPORTED
    assert call(bytes=L.f3dg_mesh_components_workspace_bytes(100, 50) - 1) == _lib.ERR_WORKSPACE
    assert call(bytes=0) == _lib.ERR_WORKSPACE
    assert list(h) == [-7] * 4                                            # a refused call writes nothing


def test_compact_refusals(env):
    _lib, L, one, _ = env
    bad = _lib.ERR_BAD_ARG
    h = _sentinel()
    need = L.f3dg_mesh_compact_workspace_bytes(100, 50)

    def count(**kw):
        a = dict(ws=one, bytes=1 << 20, N=100, F=50, faces=one, is32=1, fc=one, keep=one, h=h)
        a.update(kw)
        return L.f3dg_mesh_compact_count(None, a["ws"], a["bytes"], a["N"], a["F"], a["faces"], a["is32"], a["fc"], a["keep"], a["h"])
    for name in ("ws", "faces", "fc", "keep", "h"):
        assert count(**{name: None}) == bad, name
    assert count(N=0) == bad and count(N=-4) == bad and count(F=-1) == bad
    assert count(ws=C.c_void_p(one.value + 4)) == bad
    assert count(N=BIG) == _lib.ERR_UNSUPPORTED and count(F=BIG) == _lib.ERR_UNSUPPORTED
    assert count(bytes=need - 1) == _lib.ERR_WORKSPACE
    assert list(h) == [-7] * 4

    def emit(**kw):
        a = dict(ws=one, bytes=1 << 20, N=100, F=50, faces=one, is32=0, fc=one, keep=one, nf=5, nv=9, out=one, ids=one)
        a.update(kw)
        return L.f3dg_mesh_compact_emit(None, a["ws"], a["bytes"], a["N"], a["F"], a["faces"], a["is32"], a["fc"], a["keep"], a["nf"], a["nv"],
                                        a["out"], a["ids"])
    for name in ("ws", "faces", "fc", "keep", "out", "ids"):
        assert emit(**{name: None}) == bad, name
    assert emit(nf=0) == bad and emit(nf=-2) == bad and emit(nv=0) == bad
    assert emit(N=0) == bad and emit(F=-1) == bad and emit(F=0) == bad    # F == 0: nothing was counted
    assert emit(ws=C.c_void_p(one.value + 8)) == bad and emit(out=C.c_void_p(one.value + 4)) == bad and emit(ids=C.c_void_p(one.value + 4)) == bad
    assert emit(N=BIG) == _lib.ERR_UNSUPPORTED and emit(F=BIG) == _lib.ERR_UNSUPPORTED
    assert emit(bytes=need - 1) == _lib.ERR_WORKSPACE


def test_python_entries_refuse_host_tensors(f3d):
    import torch
    assert f3d.mesh_components is f3d.mesh.mesh_components and f3d.clean_mesh is f3d.mesh.clean_mesh
    faces = torch.tensor([[0, 1, 2]])
    with pytest.raises(RuntimeError, match="HIP device"):
        f3d.mesh.mesh_components(faces, 3)
    with pytest.raises(RuntimeError, match="HIP device"):
        f3d.mesh.clean_mesh(torch.zeros(3, 3), faces, keep_largest=1)
    import inspect
    for fn in (f3d.mesh.extract_mesh_tsdf, f3d.mesh.extract_mesh):
        p = inspect.signature(fn).parameters
        assert p["min_component_faces"].default is None and p["keep_largest"].default is None
