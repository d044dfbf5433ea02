"""The smoothing entries' host side (no GPU): the symbols, the workspace arithmetic, every refusal of include/f3dg.h found before any HIP
call with nothing written to h_counts, and the Python entries' refusal of host tensors and of inputs that require grad."""
import ctypes as C
import inspect
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("f3dg_mesh_adjacency_workspace_bytes", "f3dg_mesh_adjacency", "f3dg_mesh_smooth", "f3dg_mesh_vertex_normals")
BIG = 1 << 31
F_MAX = (BIG - 1) // 6          # 6 F < 2^31: nbr_start is int32


@pytest.fixture(scope="module")
def env(f3d):
    from f3dgaus_amd import _lib
    buf = (C.c_char * 8192)()
    one = C.c_void_p((C.addressof(buf) + 255) & ~255)          # 256-byte aligned non-NULL pointers nothing dereferences
    two, three = C.c_void_p(one.value + 1024), C.c_void_p(one.value + 2048)
    return _lib, _lib.lib(), (one, two, three), buf


def test_symbols_are_declared_exported_and_bound(env):
    _lib, L, _, _ = env
    text = open(os.path.join(ROOT, "include", "f3dg.h")).read()
    raw = C.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert re.search(r"\b(int|size_t)\s+%s\(" % name, text), name
        assert name in _lib.SIGNATURES and hasattr(L, name)
        assert getattr(raw, name) is not None, name
    assert _lib.SIGNATURES["f3dg_mesh_adjacency"][1][-1] is C.POINTER(C.c_longlong)
    assert _lib.SIGNATURES["f3dg_mesh_smooth"][1][6:9] == [C.c_float, C.c_float, C.c_int]


def test_workspace_bytes(env):
    _, L, _, _ = env
    wb = L.f3dg_mesh_adjacency_workspace_bytes
    r256 = lambda b: (b + 255) // 256 * 256
    up = lambda a, b: (a + b - 1) // b
    for N, F in ((1, 0), (3, 1), (64, 64), (65, 257), (4101, 4099), (1 << 20, 2_000_001), (BIG - 1, F_MAX)):
        # header 256 B + two 32-bit arrays of N + 1 entries in whole groups of 16 + the queue of the long rows + 6 entries of 8 B per face
        per_vertex = r256(up(N + 1, 16) * 16 * 4)
        assert wb(N, F) == 256 + 2 * per_vertex + r256(min(N, 6 * F // 33 + 1) * 4) + r256(48 * F), (N, F)
    sizes = (1, 2, 17, 1000, 4097, 1 << 20)
    for a, b in zip(sizes, sizes[1:]):                                            # positive and monotone in N and in F
        for fixed in (0, 5, 100_000):
            assert 0 < wb(a, fixed) <= wb(b, fixed) and 0 < wb(fixed + 1, a) <= wb(fixed + 1, b)
    assert wb(1, 1000) < wb(100_000, 1000) and wb(1000, 1) < wb(1000, 100_000)
    for N, F in ((0, 5), (-1, 5), (5, -1), (BIG, 5), (5, BIG), (1 << 40, 1), (5, F_MAX + 1)):
        assert wb(N, F) == 0, (N, F)


def _sentinel():
    return (C.c_longlong * 4)(-7, -7, -7, -7)


def test_adjacency_and_normals_refusals(env):
    _lib, L, (one, two, three), _ = env
    bad = _lib.ERR_BAD_ARG
    h = _sentinel()
    need = L.f3dg_mesh_adjacency_workspace_bytes(100, 50)

    def adj(**kw):
        a = dict(ws=one, bytes=1 << 20, N=100, F=50, faces=one, is32=0, start=one, nbr=one, bnd=one, h=h)
        a.update(kw)
        return L.f3dg_mesh_adjacency(None, a["ws"], a["bytes"], a["N"], a["F"], a["faces"], a["is32"], a["start"], a["nbr"], a["bnd"], a["h"])
    for name in ("ws", "faces", "start", "nbr", "bnd", "h"):
        assert adj(**{name: None}) == bad, name
    assert adj(N=0) == bad and adj(N=-4) == bad and adj(F=-1) == bad
    assert adj(ws=C.c_void_p(one.value + 8)) == bad                               # off the 16-byte grid
    assert adj(N=BIG) == _lib.ERR_UNSUPPORTED and adj(F=BIG) == _lib.ERR_UNSUPPORTED and adj(F=F_MAX + 1) == _lib.ERR_UNSUPPORTED
    assert adj(bytes=need - 1) == _lib.ERR_WORKSPACE and adj(bytes=0) == _lib.ERR_WORKSPACE
    assert list(h) == [-7] * 4                                                    # a refused call writes nothing

    def nrm(**kw):
        a = dict(ws=one, bytes=1 << 20, N=100, F=50, faces=one, is32=1, v=two, n=three)
        a.update(kw)
        return L.f3dg_mesh_vertex_normals(None, a["ws"], a["bytes"], a["N"], a["F"], a["faces"], a["is32"], a["v"], a["n"])
    for name in ("ws", "faces", "v", "n"):
        assert nrm(**{name: None}) == bad, name
    assert nrm(N=0) == bad and nrm(F=-1) == bad and nrm(ws=C.c_void_p(one.value + 4)) == bad
    assert nrm(N=BIG) == _lib.ERR_UNSUPPORTED and nrm(F=BIG) == _lib.ERR_UNSUPPORTED
    assert nrm(bytes=need - 1) == _lib.ERR_WORKSPACE


def test_smooth_refusals(env):
    _lib, L, (one, two, three), _ = env
    bad = _lib.ERR_BAD_ARG

    def smooth(**kw):
        a = dict(N=100, start=one, nbr=one, pinned=None, vin=one, lam=0.5, mu=-0.53, it=10, scratch=two, out=three)
        a.update(kw)
        return L.f3dg_mesh_smooth(None, a["N"], a["start"], a["nbr"], a["pinned"], a["vin"], a["lam"], a["mu"], a["it"], a["scratch"], a["out"])
    for name in ("start", "vin", "out", "scratch"):
        assert smooth(**{name: None}) == bad, name
    assert smooth(N=0) == bad and smooth(N=-3) == bad and smooth(N=BIG) == _lib.ERR_UNSUPPORTED
    assert smooth(it=-1) == bad
    for lam in (0.0, -0.5, 1.0000001, float("nan"), float("inf")):
        assert smooth(lam=lam) == bad, lam
    for mu in (0.3, -0.5, -0.2, float("nan")):                                    # mu must be 0 or below -lambda
        assert smooth(mu=mu) == bad, mu
    assert smooth(lam=1.0, mu=-1.0) == bad
    assert smooth(out=one) == bad and smooth(scratch=one) == bad and smooth(scratch=three) == bad       # no two arrays alias


def test_python_entries_refuse_host_tensors_and_gradients(f3d):
    import torch
    assert f3d.mesh_adjacency is f3d.mesh.mesh_adjacency and f3d.smooth_mesh is f3d.mesh.smooth_mesh
    assert f3d.vertex_normals is f3d.mesh.vertex_normals
    faces, v = torch.tensor([[0, 1, 2]]), torch.rand(3, 3)
    with pytest.raises(RuntimeError, match="HIP device"):
        f3d.mesh.mesh_adjacency(faces, 3)
    with pytest.raises(RuntimeError, match="HIP device"):
        f3d.mesh.smooth_mesh(v, faces)
    with pytest.raises(RuntimeError, match="HIP device"):
        f3d.mesh.vertex_normals(v, faces)
    g = v.clone().requires_grad_()
    with pytest.raises(NotImplementedError, match="produces no gradient for `vertices`"):
        f3d.mesh.smooth_mesh(g, faces)
    with pytest.raises(NotImplementedError, match="produces no gradient for `vertices`"):
        f3d.mesh.vertex_normals(g, faces)
    p = inspect.signature(f3d.mesh.smooth_mesh).parameters
    assert (p["iterations"].default, p["lam"].default, p["mu"].default, p["pin_boundary"].default) == (10, 0.5, -0.53, True)
    assert p["pinned"].default is None and p["adjacency"].default is None
    for fn in (f3d.mesh.extract_mesh_tsdf, f3d.mesh.extract_mesh):
        p = inspect.signature(fn).parameters
        assert p["smooth_iterations"].default is None and p["vertex_normals"].default is False
        assert (p["smooth_lambda"].default, p["smooth_mu"].default) == (0.5, -0.53)
    assert inspect.signature(f3d.ply.save_mesh_ply).parameters["vertex_normals"].default is None
    assert inspect.signature(f3d.ply.read_mesh_ply).parameters["with_normals"].default is False
