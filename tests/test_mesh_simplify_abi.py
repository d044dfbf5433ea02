"""The simplification entries' host side (no GPU): the symbols, the workspace arithmetic, every refusal of include/f3dg.h found before any
HIP call with nothing written to h_counts, the Python entry's refusals and defaults, and the new keywords of both mesh routes."""
import ctypes as C
import inspect
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("f3dg_mesh_simplify_workspace_bytes", "f3dg_mesh_simplify_count", "f3dg_mesh_simplify_emit")
BIG = 1 << 31
F_ADJ = (BIG - 1) // 6          # 6 F < 2^31: what the adjacency rows of the quadric placement allow


@pytest.fixture(scope="module")
def env(f3d):
    from f3dgaus_amd import _lib
    buf = (C.c_char * 16384)()
    base = (C.addressof(buf) + 255) & ~255
    p = [C.c_void_p(base + 1024 * i) for i in range(12)]        # 256-byte aligned non-NULL pointers nothing dereferences
    return _lib, _lib.lib(), p, buf


def test_symbols_are_declared_exported_and_bound(env):
    _lib, L, _, _ = env
    text = open(os.path.join(ROOT, "include", "f3dg.h")).read()
    raw = C.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert re.search(r"\b(int|size_t)\s+%s\(" % name, text), name
        assert name in _lib.SIGNATURES and hasattr(L, name)
        assert getattr(raw, name) is not None, name
    assert _lib.SIGNATURES["f3dg_mesh_simplify_count"][1][-3:] == [C.POINTER(C.c_double), C.c_double, C.POINTER(C.c_longlong)]
    defs = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define F3DG_SIMPLIFY_(\w+)\s+(\d+)", text)}
    assert {k.upper(): v for k, v in _lib.SIMPLIFY_PLACEMENT.items()} == {k: defs[k] for k in ("ROOT", "MEAN", "QUADRIC")}
    assert defs["MAX_ATTRS"] == _lib.SIMPLIFY_MAX_ATTRS
    assert len(_lib.SIMPLIFY_COUNTS) == 7
    data = open(_lib.LIB_PATH, "rb").read()
    assert b"ms_place_kernel" in data and b"ms_face_flag_kernel" in data            # the library holds the kernels


def test_workspace_bytes(env):
    _, L, _, _ = env
    wb = L.f3dg_mesh_simplify_workspace_bytes
    r256 = lambda b: (b + 255) // 256 * 256
    up = lambda a, b: (a + b - 1) // b

    def table(items):                                                             # a power of two, at least 16 and at least twice the items
        c = 16
        while c < 2 * items:
            c *= 2
        return c

    def compact(n):                                                               # flag words of 64 items, one count per 256 in whole groups of 16
        return r256(up(n, 64) * 8), r256(up(up(n, 256), 16) * 16 * 4)
    for N, F in ((1, 0), (3, 1), (64, 64), (65, 257), (4101, 4099), (1 << 20, 2_000_001), (BIG - 1, BIG - 1)):
        (flag_f, count_f), (flag_v, count_v) = compact(F), compact(N)
        expect = (256 + r256(table(N) * 4) + r256(table(F) * 4)                   # header, vertex table, face table
                  + r256(N * 4)                                                   # root
                  + 2 * r256(up(N + 1, 16) * 16 * 4)                              # start, fill
                  + r256(N * 4) + r256((N // 33 + 1) * 4)                         # members, the queue of the long rows
                  + flag_f + flag_v + count_f + count_v)
        assert wb(N, F) == expect, (N, F)
    sizes = (1, 2, 17, 1000, 4097, 1 << 20)
    for a, b in zip(sizes, sizes[1:]):                                            # positive and monotone in N and in F
        for fixed in (0, 5, 100_000):
            assert 0 < wb(a, fixed) <= wb(b, fixed) and 0 < wb(fixed + 1, a) <= wb(fixed + 1, b)
    assert wb(1, 1000) < wb(100_000, 1000) and wb(1000, 1) < wb(1000, 100_000)
    for N, F in ((0, 5), (-1, 5), (5, -1), (BIG, 5), (5, BIG), (1 << 40, 1)):
        assert wb(N, F) == 0, (N, F)


def test_count_refusals(env):
    _lib, L, p, _ = env
    bad = _lib.ERR_BAD_ARG
    h = (C.c_longlong * 8)(*([-7] * 8))
    need = L.f3dg_mesh_simplify_workspace_bytes(100, 50)

    def count(**kw):
        a = dict(ws=p[0], bytes=1 << 20, N=100, F=50, v=p[1], faces=p[2], is32=0, origin=(C.c_double * 3)(0.0, 0.0, 0.0), cell=0.5, h=h)
        a.update(kw)
        return L.f3dg_mesh_simplify_count(None, a["ws"], a["bytes"], a["N"], a["F"], a["v"], a["faces"], a["is32"], a["origin"], a["cell"], a["h"])
    for name in ("ws", "v", "faces", "origin", "h"):
        assert count(**{name: None}) == bad, name
    assert count(N=0) == bad and count(N=-4) == bad and count(F=-1) == bad
    assert count(ws=C.c_void_p(p[0].value + 8)) == bad                            # off the 16-byte grid
    for cell in (0.0, -1.0, float("nan"), float("inf"), -float("inf")):
        assert count(cell=cell) == bad, cell
    for o in ((float("nan"), 0.0, 0.0), (0.0, float("inf"), 0.0), (0.0, 0.0, -float("inf"))):
        assert count(origin=(C.c_double * 3)(*o)) == bad, o
    assert count(N=BIG) == _lib.ERR_UNSUPPORTED and count(F=BIG) == _lib.ERR_UNSUPPORTED
    assert count(bytes=need - 1) == _lib.ERR_WORKSPACE and count(bytes=0) == _lib.ERR_WORKSPACE
    assert list(h) == [-7] * 8                                                    # a refused call writes nothing


def test_emit_refusals(env):
    _lib, L, p, _ = env
    bad = _lib.ERR_BAD_ARG
    need = L.f3dg_mesh_simplify_workspace_bytes(100, 50)
    need_adj = L.f3dg_mesh_adjacency_workspace_bytes(100, 50)
    Q = _lib.SIMPLIFY_PLACEMENT["quadric"]

    def emit(**kw):
        a = dict(ws=p[0], bytes=1 << 20, N=100, F=50, v=p[1], faces=p[2], is32=1, placement=Q, C=3, attrs=p[3], adj=p[4], adj_bytes=1 << 20,
                 n=10, f=12, vo=p[5], fo=p[6], ao=p[7], vmap=p[8], root=p[9], size=p[10])
        a.update(kw)
        return L.f3dg_mesh_simplify_emit(None, a["ws"], a["bytes"], a["N"], a["F"], a["v"], a["faces"], a["is32"], a["placement"], a["C"],
                                         a["attrs"], a["adj"], a["adj_bytes"], a["n"], a["f"], a["vo"], a["fo"], a["ao"], a["vmap"], a["root"],
                                         a["size"])
    for name in ("ws", "v", "faces", "attrs", "adj", "vo", "fo", "ao", "vmap", "root", "size"):
        assert emit(**{name: None}) == bad, name
    assert emit(N=0) == bad and emit(F=-1) == bad and emit(F=0) == bad and emit(n=0) == bad and emit(f=0) == bad and emit(n=-1) == bad
    for placement in (-1, 3, 7):
        assert emit(placement=placement) == bad, placement
    assert emit(C=-1) == bad and emit(C=_lib.SIMPLIFY_MAX_ATTRS + 1) == bad
    assert emit(ws=C.c_void_p(p[0].value + 8)) == bad and emit(adj=C.c_void_p(p[4].value + 8)) == bad
    for name in ("fo", "vmap", "root", "size"):
        assert emit(**{name: C.c_void_p(p[6].value + 516)}) == bad, name          # an int64 output off the 8-byte grid
    # no output is another output, an input or a workspace
    outs = ("vo", "fo", "ao", "vmap", "root", "size")
    for i, a in enumerate(outs):
        for b in outs[:i]:
            assert emit(**{a: p[11], b: p[11]}) == bad, (a, b)
        for q in (p[0], p[1], p[2], p[3], p[4]):
            assert emit(**{a: q}) == bad, a
    assert emit(N=BIG) == _lib.ERR_UNSUPPORTED and emit(F=BIG) == _lib.ERR_UNSUPPORTED
    assert emit(F=F_ADJ + 1, bytes=1 << 40, adj_bytes=1 << 40) == _lib.ERR_UNSUPPORTED          # the rows of the quadric placement
    assert emit(bytes=need - 1) == _lib.ERR_WORKSPACE and emit(adj_bytes=need_adj - 1) == _lib.ERR_WORKSPACE
    # root and mean read no adjacency, and no attributes are needed with C = 0: the same refusals otherwise
    for placement in (_lib.SIMPLIFY_PLACEMENT["root"], _lib.SIMPLIFY_PLACEMENT["mean"]):
        assert emit(placement=placement, adj=None, adj_bytes=0, C=0, attrs=None, ao=None, bytes=need - 1) == _lib.ERR_WORKSPACE
        assert emit(placement=placement, adj=None, adj_bytes=0, vo=None) == bad
        assert emit(placement=placement, F=F_ADJ + 1, bytes=16) == _lib.ERR_WORKSPACE


def test_python_entry_refusals_and_defaults(f3d):
    import torch
    assert f3d.simplify_mesh is f3d.mesh.simplify_mesh
    faces, v = torch.tensor([[0, 1, 2]]), torch.rand(3, 3)
    with pytest.raises(RuntimeError, match="HIP device"):
        f3d.simplify_mesh(v, faces, 0.5)
    with pytest.raises(RuntimeError, match="HIP device"):
        f3d.simplify_mesh(v, faces, grid_resolution=8, placement="root", vertex_colors=torch.rand(3, 3))
    g = v.clone().requires_grad_()
    with pytest.raises(NotImplementedError, match="produces no gradient for `vertices`"):
        f3d.simplify_mesh(g, faces, 0.5)
    with pytest.raises(NotImplementedError, match="produces no gradient for `vertex_colors`"):
        f3d.simplify_mesh(v, faces, 0.5, vertex_colors=g)
    with pytest.raises(ValueError, match="exactly one of cell_size and grid_resolution"):
        f3d.simplify_mesh(v, faces)
    with pytest.raises(ValueError, match="exactly one of cell_size and grid_resolution"):
        f3d.simplify_mesh(v, faces, 0.5, grid_resolution=8)
    with pytest.raises(ValueError, match="placement"):
        f3d.simplify_mesh(v, faces, 0.5, placement="median")
    for cell in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="cell_size"):
            f3d.simplify_mesh(v, faces, cell)
    for res in (0, -3, 1 << 21):
        with pytest.raises(ValueError, match="grid_resolution"):
            f3d.simplify_mesh(v, faces, grid_resolution=res)
    for origin in ((0.0, 0.0), (0.0, float("nan"), 0.0)):
        with pytest.raises(ValueError, match="origin"):
            f3d.simplify_mesh(v, faces, 0.5, origin=origin)
    sig = inspect.signature(f3d.mesh.simplify_mesh)
    p = sig.parameters
    assert list(p) == ["vertices", "faces", "cell_size", "grid_resolution", "origin", "placement", "vertex_colors", "adjacency"]
    assert p["cell_size"].default is None and p["cell_size"].kind is inspect.Parameter.POSITIONAL_OR_KEYWORD
    for name in ("grid_resolution", "origin", "vertex_colors", "adjacency"):
        assert p[name].default is None and p[name].kind is inspect.Parameter.KEYWORD_ONLY, name
    assert p["placement"].default == "quadric" and p["placement"].kind is inspect.Parameter.KEYWORD_ONLY


def test_both_routes_take_the_keywords(f3d):
    for fn in (f3d.mesh.extract_mesh_tsdf, f3d.mesh.extract_mesh):
        p = inspect.signature(fn).parameters
        assert p["simplify_cell"].default is None and p["simplify_placement"].default == "quadric"
