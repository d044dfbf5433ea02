"""The contribution and Gaussian-compaction entries' host side (no GPU): the symbols, the workspace arithmetic, every refusal of
include/f3dg.h found before any HIP call with nothing written to h_kept, and the Python entries' refusals before any launch."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("f3dg_contribution", "f3dg_gaussian_compact_workspace_bytes", "f3dg_gaussian_compact_count", "f3dg_gaussian_compact_emit")
ID_MAX = (1 << 28) - 1


@pytest.fixture(scope="module")
def env(f3d):
    from f3dgaus_amd import _lib
    buf = (C.c_char * 4096)()
    one = C.c_void_p((C.addressof(buf) + 255) & ~255)          # a 256-byte aligned non-NULL pointer nothing dereferences
    return _lib, _lib.lib(), one, buf


def test_symbols_are_declared_exported_and_bound(env):
    _lib, L, _, _ = env
    text = open(os.path.join(ROOT, "include", "f3dg.h")).read()
    raw = C.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert re.search(r"\b(int|size_t)\s+%s\(" % name, text), name
        assert name in _lib.SIGNATURES and hasattr(L, name)
        assert getattr(raw, name) is not None, name
    assert re.search(r"#define\s+F3DG_CONTRIBUTION_BYTES\s+32\b", text) and re.search(r"#define\s+F3DG_COMPACT_MAX_ARRAYS\s+8\b", text)
    assert _lib.SIGNATURES["f3dg_gaussian_compact_count"][1][-1] is C.POINTER(C.c_longlong)
    assert _lib.SIGNATURES["f3dg_gaussian_compact_count"][1][8] is C.c_double
    assert b"contribution_kernel" in open(_lib.LIB_PATH, "rb").read()


def test_workspace_arithmetic(env):
    _, L, _, _ = env
    r256 = lambda b: (b + 255) // 256 * 256
    up = lambda a, b: (a + b - 1) // b
    gc = L.f3dg_gaussian_compact_workspace_bytes
    for P in (0, 1, 64, 65, 257, 4101, 589824, 2_000_001, ID_MAX):
        # header 256 B + one bit per Gaussian (whole 64-bit words) + one count per 256 Gaussians (whole groups of 16), each rounded to 256 B
        assert gc(P) == 256 + r256(up(P, 64) * 8) + r256(up(up(P, 256), 16) * 16 * 4), P
    for P in (-1, ID_MAX + 1, 1 << 40):
        assert gc(P) == 0, P


def test_contribution_refusals(env):
    _lib, L, one, _ = env
    bad = _lib.ERR_BAD_ARG
    need = L.f3dg_workspace_bytes(1000, 64, 64, 2, 50000)

    def call(**kw):
        a = dict(ws=one, bytes=need, cap=50000, V=2, P=1000, W=64, H=64, stats=one, fT=None)
        a.update(kw)
        return L.f3dg_contribution(None, a["ws"], a["bytes"], a["cap"], a["V"], a["P"], a["W"], a["H"], 0.5, 0.5, a["stats"], a["fT"])
    assert call(ws=None) == bad and call(stats=None) == bad
    assert call(P=-1) == bad and call(V=0) == bad and call(W=0) == bad and call(H=-3) == bad and call(cap=-1) == bad
    assert call(P=ID_MAX + 1, bytes=1 << 62) == bad
    assert call(stats=C.c_void_p(one.value + 16)) == bad                  # off the 32-byte grid
    assert call(V=8, W=16384, H=16384, bytes=1 << 62) == bad              # 2^31 pixels in one call: the record's limit
    assert call(bytes=need - 1) == _lib.ERR_WORKSPACE and call(bytes=0) == _lib.ERR_WORKSPACE


def test_compact_refusals(env):
    _lib, L, one, _ = env
    bad = _lib.ERR_BAD_ARG
    h = (C.c_longlong * 1)(-7)
    need = L.f3dg_gaussian_compact_workspace_bytes(1000)

    def count(**kw):
        a = dict(ws=one, bytes=1 << 20, P=1000, stats=one, keep=one, mt=1, mm=0.0, ms=0.0, h=h)
        a.update(kw)
        return L.f3dg_gaussian_compact_count(None, a["ws"], a["bytes"], a["P"], a["stats"], a["keep"], a["mt"], a["mm"], a["ms"], a["h"])
    assert count(ws=None) == bad and count(h=None) == bad
    assert count(stats=None, keep=None) == bad                            # nothing to go by
    assert count(P=-1) == bad and count(mt=-1) == bad and count(mm=float("nan")) == bad and count(ms=float("nan")) == bad
    assert count(ws=C.c_void_p(one.value + 4)) == bad and count(stats=C.c_void_p(one.value + 8)) == bad
    assert count(P=ID_MAX + 1) == _lib.ERR_UNSUPPORTED
    assert count(bytes=need - 1) == _lib.ERR_WORKSPACE
    assert list(h) == [-7]                                                # a refused call writes nothing

    srcs, dsts = (C.c_void_p * 9)(*[one.value] * 9), (C.c_void_p * 9)(*[one.value] * 9)
    rows = (C.c_int * 9)(*[3] * 9)

    def emit(**kw):
        a = dict(ws=one, bytes=1 << 20, P=1000, K=10, n=7, srcs=srcs, dsts=dsts, rows=rows, ids=one)
        a.update(kw)
        return L.f3dg_gaussian_compact_emit(None, a["ws"], a["bytes"], a["P"], a["K"], a["n"], a["srcs"], a["dsts"], a["rows"], a["ids"])
    assert emit(ws=None) == bad and emit(ids=None) == bad and emit(srcs=None) == bad and emit(dsts=None) == bad and emit(rows=None) == bad
    assert emit(n=9) == bad and emit(n=-1) == bad                         # more than F3DG_COMPACT_MAX_ARRAYS arrays
    assert emit(rows=(C.c_int * 9)(3, 0, 3, 3, 3, 3, 3, 3, 3)) == bad and emit(rows=(C.c_int * 9)(-2, *[3] * 8)) == bad      # a row width <= 0
    assert emit(srcs=(C.c_void_p * 9)(one.value, None, *[one.value] * 7)) == bad
    assert emit(K=0) == bad and emit(K=-4) == bad and emit(K=1001) == bad
    assert emit(P=-1) == bad and emit(P=0) == bad                         # P == 0: nothing was counted
    assert emit(ws=C.c_void_p(one.value + 8)) == bad and emit(ids=C.c_void_p(one.value + 2)) == bad
    assert emit(P=ID_MAX + 1, K=5) == _lib.ERR_UNSUPPORTED
    assert emit(bytes=need - 1) == _lib.ERR_WORKSPACE


def test_python_entries_refuse_before_any_launch(f3d):
    import torch
    assert f3d.prune_gaussians is f3d.contribution.prune_gaussians and f3d.gaussian_contribution is f3d.contribution.gaussian_contribution
    assert f3d.contribution_raw is f3d.contribution.contribution_raw
    pc = {"xyz": torch.zeros(1, 5, 3), "opacity": torch.zeros(1, 5, 1)}
    with pytest.raises(RuntimeError, match="stats=.*keep="):
        f3d.prune_gaussians(pc, 0)
    with pytest.raises(RuntimeError, match="HIP device"):
        f3d.prune_gaussians(pc, 0, keep=torch.ones(5, dtype=torch.bool))
    cfg = {"model": {"fov": 50.0, "training_resolution": 32, "max_sh_degree": 1}}
    with pytest.raises(RuntimeError, match="HIP device"):
        f3d.gaussian_contribution(pc, 0, torch.eye(4)[None], torch.eye(4)[None], torch.zeros(1, 3), torch.zeros(3), cfg)
    # the record's columns, on host memory: sum_fixed 3 * 2^31, blended 5 | stops 2 << 32, the bits of 0.25
    s = f3d.GaussianContribution(2, "cpu")
    s.raw[1] = torch.tensor([-2147483648, 1, 5, 2, 0x3E800000, 0, 0, 0], dtype=torch.int32)
    assert s.sum_fixed.tolist() == [0, 3 << 31] and s.sum_weight.tolist() == [0.0, 1.5]
    assert s.blended.tolist() == [0, 5] and s.stops.tolist() == [0, 2] and s.touched.tolist() == [0, 7]
    assert s.max_weight.tolist() == [0.0, 0.25] and s.sum_weight.dtype == torch.float64 and s.touched.dtype == torch.int64
