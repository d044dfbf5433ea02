"""``f3dg_cycle_inputs_backward`` (the adjoint of the cycle aggregation's hand-off kernel) at the C ABI: declared in include/f3dg.h, bound in
``_lib``, exported by the library, and its argument checks -- which run before any HIP call, as the forward's do, so they are testable
without a GPU."""
import ctypes as C
import inspect
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "f3dg_cycle_inputs_backward"


def _header():
    return open(os.path.join(ROOT, "include", "f3dg.h")).read()


def test_header_declares_and_documents_the_entry():
    txt = _header()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    m = re.search(r"int\s+" + NAME + r"\s*\(([^)]*)\)\s*;", code)
    assert m, "include/f3dg.h does not declare " + NAME
    args = [" ".join(a.split()) for a in m.group(1).split(",")]
    assert args == ["void* stream", "int B", "int V", "int H", "int W", "const float* raster", "const float* g_xin", "const float* g_depth",
                    "float* d_raster"], args
    # the "what each entry point replaces" list at the top names it with the reference lines autograd differentiates there
    head = txt[:txt.index("#ifndef F3DG_H_INCLUDED")]
    assert NAME in head and "visualize.py:311, 331-333" in head[head.index(NAME):head.index(NAME) + 300]


def test_binding_and_export(f3d):
    from f3dgaus_amd import _lib
    assert NAME in _lib.SIGNATURES
    res, args = _lib.SIGNATURES[NAME]
    assert res is C.c_int and args == [C.c_void_p] + [C.c_int] * 4 + [C.c_void_p] * 4
    assert hasattr(C.CDLL(_lib.LIB_PATH), NAME)
    assert getattr(_lib.lib(), NAME).argtypes == args


def _aligned(n_bytes=256):
    buf = (C.c_char * (n_bytes + 16))()
    a = C.addressof(buf)
    a += (-a) % 16
    return buf, a


def test_refusals_and_the_empty_batch(f3d):
    from f3dgaus_amd import _lib
    fn = getattr(_lib.lib(), NAME)
    keep, a = _aligned()
    p = lambda off=0: C.c_void_p(a + off)
    ok = dict(B=2, V=3, H=4, W=6, raster=p(), g_xin=p(64), g_depth=p(128), d_raster=p(192))

    def call(**kw):
        d = dict(ok, **kw)
        return fn(None, d["B"], d["V"], d["H"], d["W"], d["raster"], d["g_xin"], d["g_depth"], d["d_raster"])

    bad = _lib.ERR_BAD_ARG
    assert call(raster=None) == bad and call(d_raster=None) == bad
    for name in ("V", "H", "W"):
        assert call(**{name: 0}) == bad and call(**{name: -1}) == bad, name
    assert call(B=-1) == bad
    assert call(H=3, W=7) == bad and call(H=1, W=2) == bad               # H * W = 21, 2: no multiple of 4
    for name in ("raster", "g_xin", "g_depth", "d_raster"):
        assert call(**{name: p(4)}) == bad and call(**{name: p(8)}) == bad, name      # 4- and 8-byte aligned only
    assert call(B=65536, V=1) == bad and call(B=256, V=256) == bad and call(B=1, V=65536) == bad       # B * V > 65,535 (grid.y)
    assert call(B=1 << 20, V=1 << 12) == bad                                # ... also where B * V leaves 32 bits
    # B == 0 is an empty batch: F3DG_OK at once, with or without the optional cotangents
    assert call(B=0) == _lib.OK and call(B=0, g_xin=None, g_depth=None) == _lib.OK
    assert call(B=0, raster=None) == bad                                    # (the required pointers are checked first, as in the forward)
    del keep


def test_python_surface_without_gpu(f3d):
    """The new keywords exist with the defaults that keep every existing call what it was."""
    from f3dgaus_amd import cycle, gaussian_predictor, unet_gs
    sig = inspect.signature(cycle.cycle_aggregate).parameters
    assert sig["differentiable"].default is False and sig["grad_through_renders"].default is True
    assert list(sig)[:9] == ["model", "images", "depth", "cfg", "rig", "num_views", "yaw_diff", "pitch_diff", "return_renders"]
    for f in (gaussian_predictor.GaussianSplatPredictor_gtunet.forward, unet_gs.Unet_GS_gtunet.forward):
        params = inspect.signature(f).parameters
        assert list(params)[-1] == "head" and params["head"].default is True
    assert f3d.splat_head_merge is gaussian_predictor.splat_head_merge
    assert list(inspect.signature(f3d.splat_head_merge).parameters) == ["net_outs", "depths", "ray_dirs", "view_to_worlds", "cam_quats",
                                                                       "squre_clip"]
    import torch
    z = torch.zeros(1, 23, 2, 2)
    with pytest.raises(RuntimeError, match="HIP device"):                   # no CPU fallback
        f3d.splat_head_merge([z], [torch.zeros(1, 1, 2, 2)], torch.zeros(1, 3, 2, 2), [torch.eye(4)[None]], [torch.zeros(1, 4)])
