"""The vertex colour baking's host side (no GPU): the symbols, the workspace function, every refusal of include/f3dg.h found before any
launch with nothing written to h_counts, and the Python entry's refusal of host tensors and of vertices or images that require grad."""
import ctypes as C
import inspect
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("f3dg_mesh_bake_workspace_bytes", "f3dg_mesh_bake_colors")
BIG = 1 << 31


@pytest.fixture(scope="module")
def env(f3d):
    from f3dgaus_amd import _lib
    buf = (C.c_char * 16384)()
    one = C.c_void_p((C.addressof(buf) + 255) & ~255)          # 256-byte aligned non-NULL pointers nothing dereferences
    return _lib, _lib.lib(), [C.c_void_p(one.value + 1024 * k) for k in range(13)], buf


def test_symbols_are_declared_exported_and_bound(env):
    _lib, L, _, _ = env
    text = open(os.path.join(ROOT, "include", "f3dg.h")).read()
    raw = C.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert re.search(r"\b(int|size_t)\s+%s\(" % name, text), name
        assert name in _lib.SIGNATURES and hasattr(L, name)
        assert getattr(raw, name) is not None, name
    assert text.index("f3dg_mesh_bake_colors / f3dg_mesh_bake_workspace_bytes") < text.index("#ifndef F3DG_H_INCLUDED")     # the symbol list at the top
    sig = _lib.SIGNATURES["f3dg_mesh_bake_colors"][1]
    assert len(sig) == 27 and sig[-1] is C.POINTER(C.c_longlong)
    assert [k for k, t in enumerate(sig) if t is C.c_double] == [8, 9, 12, 18, 19, 20]      # fx fy z_near alpha_min depth_tol cos_min
    assert [sig[k] for k in (3, 6, 10, 11)] == [C.c_longlong] * 4                           # N V H W
    assert _lib.SIGNATURES["f3dg_mesh_bake_workspace_bytes"] == (C.c_size_t, [C.c_longlong] * 4)
    for name, value in (("BLEND", 0), ("BEST", 1)):
        assert re.search(r"#define F3DG_BAKE_%s %d\b" % (name, value), text)
    assert _lib.BAKE_MODE == {"blend": 0, "best": 1}
    assert _lib.BAKE_COUNTS == ("near", "outside", "uncovered", "occluded", "grazing", "masked", "used", "vertices_seen")


def test_workspace_bytes(env):
    _, L, _, _ = env
    wb = L.f3dg_mesh_bake_workspace_bytes
    sizes = (1, 2, 17, 1000, 4097)
    for a, b in zip(sizes, sizes[1:]):                             # positive, a multiple of 16, and monotone in every size
        assert 0 < wb(a, 9, 8, 8) <= wb(b, 9, 8, 8) and 0 < wb(2, a, 8, 8) <= wb(2, b, 8, 8)
        assert 0 < wb(2, 9, a, 8) <= wb(2, 9, b, 8) and 0 < wb(2, 9, 8, a) <= wb(2, 9, 8, b)
    for V, N, H, W in ((1, 1, 1, 1), (3, 162, 29, 33), (130, 12, 4, 5), (128, 27_000, 256, 256), (1, 5, 16384, 16384), (BIG - 1, 1, 1, 1), (1, BIG - 1, 7, 5)):
        assert wb(V, N, H, W) > 0 and wb(V, N, H, W) % 16 == 0, (V, N, H, W)
    for V, N, H, W in ((0, 5, 8, 8), (-1, 5, 8, 8), (1, 0, 8, 8), (1, -1, 8, 8), (1, 5, 0, 8), (1, 5, 8, 0), (1, 5, 8, -3), (1, 5, 16385, 8), (1, 5, 8, 16385),
                       (1, BIG, 8, 8), (BIG, 1, 1, 1), (8, 5, 16384, 16384), (2, 1 << 30, 8, 8), (1 << 40, 1, 1, 1), (1, 1 << 62, 1, 1)):
        assert wb(V, N, H, W) == 0, (V, N, H, W)


def test_refusals_write_nothing(env):
    _lib, L, p, _ = env
    bad, uns = _lib.ERR_BAD_ARG, _lib.ERR_UNSUPPORTED
    h = (C.c_longlong * 8)(*([-7] * 8))
    need = L.f3dg_mesh_bake_workspace_bytes(3, 162, 29, 33)
    nan, inf = float("nan"), float("inf")

    def call(**kw):
        a = dict(ws=p[0], bytes=1 << 20, N=162, v=p[1], n=p[2], V=3, wv=p[3], fx=28.0, fy=25.0, H=29, W=33, z_near=0.01, C=3, images=p[4],
                 face_id=p[5], depth=p[6], alpha=p[7], alpha_min=0.5, depth_tol=0.05, cos_min=0.1, mode=0, colors=p[8], weight=p[9], n_used=p[10],
                 best_view=p[11], h=h)
        a.update(kw)
        return L.f3dg_mesh_bake_colors(None, a["ws"], a["bytes"], a["N"], a["v"], a["n"], a["V"], a["wv"], a["fx"], a["fy"], a["H"], a["W"],
                                       a["z_near"], a["C"], a["images"], a["face_id"], a["depth"], a["alpha"], a["alpha_min"], a["depth_tol"],
                                       a["cos_min"], a["mode"], a["colors"], a["weight"], a["n_used"], a["best_view"], a["h"])
    for name in ("ws", "v", "wv", "images", "face_id", "depth", "colors", "weight", "n_used", "best_view", "h"):      # everything but normals and alpha
        assert call(**{name: None}) == bad, name
    for name in ("N", "V", "H", "W"):
        assert call(**{name: 0}) == bad and call(**{name: -4}) == bad, name
    assert call(C=0) == bad and call(C=9) == bad and call(C=-1) == bad
    for name in ("fx", "fy", "z_near"):
        for value in (0.0, -1.0, nan, inf):
            assert call(**{name: value}) == bad, (name, value)
    for value in (-1e-300, -1.0, nan, inf):
        assert call(depth_tol=value) == bad, value
    for value in (-1e-300, 1.0000000000000002, 2.0, nan, inf, -inf):
        assert call(cos_min=value) == bad, value
    assert call(alpha_min=nan) == bad
    assert call(mode=2) == bad and call(mode=-1) == bad
    assert call(ws=C.c_void_p(p[0].value + 8)) == bad                                # off the 16-byte grid
    assert call(N=BIG) == uns and call(V=BIG) == uns and call(H=16385) == uns and call(W=16385) == uns
    assert call(V=8, H=16384, W=16384) == uns and call(V=64, N=1 << 25) == uns
    assert call(bytes=need - 1) == _lib.ERR_WORKSPACE and call(bytes=0) == _lib.ERR_WORKSPACE
    assert list(h) == [-7] * 8                                                       # a refused call writes nothing


def test_python_entry_refuses_host_tensors_and_gradients(f3d):
    import torch
    assert f3d.bake_vertex_colors is f3d.mesh.bake_vertex_colors
    faces, v, wv, images = torch.tensor([[0, 1, 2]]), torch.rand(3, 3), torch.eye(4)[None], torch.rand(1, 3, 8, 8)
    with pytest.raises(RuntimeError, match="HIP device"):
        f3d.bake_vertex_colors(v, faces, images, wv, 50.0)
    with pytest.raises(NotImplementedError, match="produces no gradient for `vertices`"):
        f3d.bake_vertex_colors(v.clone().requires_grad_(), faces, images, wv, 50.0)
    with pytest.raises(NotImplementedError, match="produces no gradient for `images`"):
        f3d.bake_vertex_colors(v, faces, images.clone().requires_grad_(), wv, 50.0)
    p = inspect.signature(f3d.mesh.bake_vertex_colors).parameters
    assert [k for k in p][:5] == ["vertices", "faces", "images", "world_views", "fov"]
    defaults = {"vertex_normals": None, "alpha": None, "alpha_min": 0.5, "depth_tol": None, "cos_min": 0.1, "mode": "blend", "cull": "none",
                "z_near": 0.01, "visibility": None}
    assert [k for k in p][5:] == list(defaults)
    assert all(p[k].kind is inspect.Parameter.KEYWORD_ONLY and p[k].default == d for k, d in defaults.items())
    for route in (f3d.mesh.extract_mesh, f3d.mesh.extract_mesh_tsdf):
        assert inspect.signature(route).parameters["color_from_views"].default is False
