"""The depth sort of a compact view -- all keys that touch a tile within 2^24 of kbase = kmin & ~0xFFFF -- narrows its keys pass by
pass: pass 0 finds the views' key ranges (its histogram) and writes (key - kbase) >> 8 in 16 bits, pass 1 reads those and writes their
top 8 bits, pass 2 reads those and writes the order only. The narrow keys of a view lie at the start of the view's own slice of the
key array; a view that is not compact keeps 32-bit keys and four passes in the same launches. The digits are the ones of the 32-bit
keys, so the order -- and with it every list -- is the same element for element. The shapes here are the ones at which that can go
wrong. Every case holds the final list, the ranges and the count to the oracle's exactly (lists without tile culling), and the images
of the default, culled call to the plain transcription's (option reference_kernels) bit for bit, and asserts first, from the oracle,
that the scene has the property it is there for.

Several cases look through a camera whose view matrix is the identity: the sort key of a Gaussian is then the bit pattern of its z,
which the case sets.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import f3dgaus_amd as f3d
from f3dgaus_amd import _lib
from helpers import make_scene, run_hip, run_oracle

pytestmark = pytest.mark.gpu

SORT_CHUNK = 4096       # F3DG_SORT_CHUNK of f3dg_common.h: keys per workgroup of a pass


def _views(scene, idx):
    return dict(scene, **{k: scene[k][idx].contiguous() for k in ("viewmatrix", "projmatrix", "campos")})


def _joined(per):
    """The oracle's lists of several views joined the way a batched call lays them out: view after view, ranges as positions in the
    joined list, (0, 0) where empty."""
    pl, rg, total = [], [], 0
    for o in per:
        r = o["ranges"].astype(np.int64)
        rg.append(r + total * (r.sum(-1, keepdims=True) > 0))
        pl.append(np.array(o["point_list"], dtype=np.uint32))
        total += o["num_rendered"]
    return dict(per=per, point_list=np.concatenate(pl), ranges=np.stack(rg), num_rendered=total)


def _oracle_views(scene):
    return _joined([run_oracle(scene, v) for v in range(scene["viewmatrix"].shape[0])])


def _culled_bits(scene, device, reference):
    """Images of the default (tile-culled) call on the general launch sequence, in the reference's arithmetic: through the plain
    transcription of the compositing kernel (reference) or the default kernels."""
    L = _lib.lib()
    dev = lambda t: None if t is None else t.to(device)
    try:
        assert L.f3dg_set_option(b"reference_kernels", 1 if reference else 0) == 0
        out, _, _ = f3d.rasterize_views(
            dev(scene["means3D"]), dev(scene["opacities"]), dev(scene["viewmatrix"]), dev(scene["projmatrix"]), dev(scene["campos"]),
            dev(scene["bg"]), image_height=scene["H"], image_width=scene["W"], tanfovx=scene["tanfovx"], tanfovy=scene["tanfovy"],
            sh=dev(scene["shs"]), colors_precomp=dev(scene["colors_precomp"]), scales=dev(scene["scales"]), rotations=dev(scene["rotations"]),
            sh_degree=scene["sh_degree"], scale_modifier=scene["scale_modifier"], kernel_size=scene["kernel_size"], exact=True,
            small_path=False)
        if reference:
            assert b"render_fwd_kernel" in L.f3dg_debug_last_render_kernel(), L.f3dg_debug_last_render_kernel()
        return out.cpu().numpy().view(np.uint32)
    finally:
        L.f3dg_set_option(b"reference_kernels", 0)


def _check(scene, device, ora=None, max_rendered=None):
    ora = _oracle_views(scene) if ora is None else ora
    h = run_hip(scene, device, max_rendered=max_rendered)
    assert h["num_rendered"] == ora["num_rendered"]
    assert np.array_equal(h["point_list"], ora["point_list"])
    assert np.array_equal(h["ranges"].astype(np.int64), ora["ranges"])
    assert np.array_equal(_culled_bits(scene, device, True), _culled_bits(scene, device, False))
    return h, ora


def _keys(o):
    """Of one oracle view: the sort keys (depth bits) of the Gaussians that touch a tile, and their ids."""
    seen = np.flatnonzero(np.array(o["tiles_touched"]) > 0)
    return np.array(o["depths"], dtype=np.float32).view(np.uint32)[seen].astype(np.int64), seen


def _kbase(o):
    return int(_keys(o)[0].min()) & ~0xFFFF


def _compact(o):
    """gsort_compact of one oracle view: the keys of the Gaussians that touch a tile lie within 2^24 of kmin & ~0xFFFF."""
    k = _keys(o)[0]
    return len(k) > 0 and ((int(k.max()) - (int(k.min()) & ~0xFFFF)) >> 24) == 0


# ------------------------------------------------------------------------------------------------ P x V at 72 x 40
GRID_P = [1, 15, 16, 17, 255, 4095, 4096, 4097, 4111, 4112, 8193]


@functools.lru_cache(maxsize=None)
def _grid_scene(P):
    return make_scene(P=P, res=(72, 40), s0=0.05, seed=3, view=range(9))


@functools.lru_cache(maxsize=None)
def _grid_oracle(P, cam):
    return run_oracle(_grid_scene(P), cam)


def _grid_properties(P, per):
    """Every view that sees anything is compact (it reads 16- and 8-bit keys); from 15 Gaussians on every view sees something."""
    for o in per:
        assert _compact(o) == (o["num_rendered"] > 0)
    if P >= 15:
        assert all(o["num_rendered"] > 0 for o in per)


@pytest.mark.parametrize("V", [1, 3, 9])
@pytest.mark.parametrize("P", GRID_P)
def test_vector_edges_and_slice_alignments(P, V, gpu_device):
    """The histograms read 16-byte vectors of 8 (u16) and 16 (u8) keys, the first and the last of a chunk masked: P around 16 and
    around 4,096 + 16 puts the end of a view's keys, and of its first chunk, on either side of a vector's edge; a view's slice starts
    at byte 4 v P, at every alignment for odd P and v > 0; from 4,097 on there is a second chunk."""
    scene = _views(_grid_scene(P), list(range(V)))
    per = [_grid_oracle(P, v) for v in range(V)]
    _grid_properties(P, per)
    _check(scene, gpu_device, _joined(per))


# ------------------------------------------------------------------------------------------------ compact and not, in one call
def _mixed_compact_scene():
    scene = make_scene(P=1500, res=(72, 40), s0=0.05, seed=17, view=[0, 3, 5])
    scene["means3D"] = scene["means3D"].clone()
    scene["means3D"][:40, 2] = 1.5            # close to the canonical camera, on its axis: out of the side views' frusta
    scene["means3D"][:40, :2] *= 0.1
    return scene


def _mixed_compact_properties(ora):
    flags = [_compact(o) for o in ora["per"]]
    assert flags[0] is False and True in flags[1:], flags
    assert all(o["num_rendered"] > 0 for o in ora["per"])


def test_compact_and_wide_views_in_one_call(gpu_device):
    """A few Gaussians close to the first camera, which the others do not see: the first view keeps 32-bit keys and four passes while
    compact views of the same launches narrow theirs."""
    scene = _mixed_compact_scene()
    ora = _oracle_views(scene)
    _mixed_compact_properties(ora)
    _check(scene, gpu_device, ora)


# ------------------------------------------------------------------------------------------------ keys set by the case
def _key_scene(keys, seed, P_behind=0):
    """One view through a camera at the origin whose view matrix is the identity, Gaussian i at depth bits keys[i] (a float > 0.2),
    inside the frustum; P_behind more Gaussians follow, behind the near plane."""
    keys = np.asarray(keys, dtype=np.uint32)
    P = len(keys) + P_behind
    scene = make_scene(P=P, res=(72, 40), s0=0.05, seed=seed, view=[0])
    vm, pm = scene["viewmatrix"][0].double(), scene["projmatrix"][0].double()
    proj = torch.linalg.solve(vm, pm)                             # full_proj = world_view @ projection (row vectors)
    scene["viewmatrix"][0] = torch.eye(4)
    scene["projmatrix"][0] = proj.float()
    scene["campos"][0] = 0.0
    rng = np.random.default_rng(seed)
    z = np.concatenate([keys.view(np.float32), np.full(P_behind, -1.0, dtype=np.float32)])
    xy = rng.uniform(-0.6, 0.6, size=(P, 2)).astype(np.float32) * np.abs(z)[:, None] * np.array([scene["tanfovx"], scene["tanfovy"]], dtype=np.float32)
    scene["means3D"] = torch.from_numpy(np.concatenate([xy, z[:, None]], 1).astype(np.float32)).contiguous()
    return scene


def _key_oracle(scene, keys):
    """The oracle of a _key_scene, after asserting that the keys are what the case set and that every one of them touches a tile."""
    ora = _oracle_views(scene)
    o = ora["per"][0]
    k, seen = _keys(o)
    assert np.array_equal(seen, np.arange(len(keys))), (len(seen), len(keys))
    assert np.array_equal(k, np.asarray(keys, dtype=np.int64))
    return ora


def _spread_keys(lo, hi, n, seed):
    return np.random.default_rng(seed).integers(lo, hi, size=n, dtype=np.int64, endpoint=True)


@pytest.mark.parametrize("span", [0xFFFFFF, 0x1000000])
def test_edge_of_compactness(span, gpu_device):
    """kmax - kbase = 0xFFFFFF: the widest compact view, its farthest Gaussian in digit 255 of the last pass, where the Gaussians that
    touch no tile go. One more: not compact, four passes over 32-bit keys."""
    kbase = 0x40000000                                            # 2.0
    keys = np.concatenate([[kbase + 0x1234, kbase + span], _spread_keys(kbase + 0x1234, kbase + 0xFFFFFF, 598, seed=61)])
    scene = _key_scene(keys, seed=61)
    ora = _key_oracle(scene, keys)
    o = ora["per"][0]
    assert _kbase(o) == kbase and int(_keys(o)[0].max()) - kbase == span
    assert _compact(o) == (span == 0xFFFFFF)
    if span == 0xFFFFFF:
        assert ((keys[1] - kbase) >> 16) == 255
    _check(scene, gpu_device, ora)


def test_kmin_on_a_multiple_of_65536(gpu_device):
    """kmin's low 16 bits are 0: kbase = kmin, the nearest Gaussian's narrow keys are 0 in both widths."""
    kmin = 0x40400000                                             # 3.0
    keys = np.concatenate([[kmin], _spread_keys(kmin, kmin + 0x7FFFFF, 499, seed=67)])
    scene = _key_scene(keys, seed=67)
    ora = _key_oracle(scene, keys)
    o = ora["per"][0]
    assert int(_keys(o)[0].min()) & 0xFFFF == 0 and _kbase(o) == kmin and _compact(o)
    _check(scene, gpu_device, ora)


def test_culled_gaussians_beside_digit_255(gpu_device):
    """A compact view that also holds Gaussians behind the near plane (key ~0, narrow keys 0xFFFF and 0xFF), together with visible keys
    whose low 16 bits are 0xFFFF and visible keys in digit 255 of the last pass -- one of them 0x..FFFFFF, the largest 16-bit key a
    Gaussian that touches a tile can have, equal to the one of those that touch none."""
    kbase = 0x40000000
    special = [kbase + 0x10, kbase + 0xFFFFFF, kbase + 0xFF0000, kbase + 0xFF1234, kbase + 0x12FFFF, kbase + 0xFFFF, kbase + 0xFEFFFF]
    keys = np.concatenate([special, _spread_keys(kbase + 0x10, kbase + 0xFFFFFF, 693, seed=71)])
    scene = _key_scene(keys, seed=71, P_behind=300)
    ora = _key_oracle(scene, keys)                                # (the 300 behind the camera touch no tile: _key_oracle holds `seen` to the others)
    o = ora["per"][0]
    k = _keys(o)[0]
    assert _compact(o) and _kbase(o) == kbase and len(o["tiles_touched"]) == len(keys) + 300
    assert int(((k & 0xFFFF) == 0xFFFF).sum()) >= 4 and int((((k - kbase) >> 16) == 255).sum()) >= 3
    assert int(k.max()) - kbase == 0xFFFFFF
    _check(scene, gpu_device, ora)


def test_equal_depths_keep_id_order(gpu_device):
    """Runs of Gaussians at the same depth, to the bit: the sort is stable, the id decides -- in every pass, narrow or not."""
    kbase = 0x40000000
    distinct = _spread_keys(kbase + 1, kbase + 0x3FFFFF, 40, seed=73)
    keys = np.random.default_rng(73).choice(distinct, size=800)
    scene = _key_scene(keys, seed=73)
    ora = _key_oracle(scene, keys)
    o = ora["per"][0]
    assert _compact(o) and len(np.unique(_keys(o)[0])) <= 40 < 800
    _check(scene, gpu_device, ora)


# ------------------------------------------------------------------------------------------------ a view that sees nothing
def _turned_away_scene():
    scene = make_scene(P=700, res=(72, 40), s0=0.05, seed=5, view=[1, 2, 3])
    vm, pm = scene["viewmatrix"].double(), scene["projmatrix"].double()
    turn = torch.diag(torch.tensor([-1.0, 1.0, -1.0, 1.0], dtype=torch.float64))
    proj = torch.linalg.solve(vm[1], pm[1])                       # full_proj = world_view @ projection (row vectors)
    scene["viewmatrix"][1] = (vm[1] @ turn).float()
    scene["projmatrix"][1] = (vm[1] @ turn @ proj).float()
    return scene


def _turned_away_properties(ora):
    counts = [o["num_rendered"] for o in ora["per"]]
    assert counts[1] == 0 and counts[0] > 0 and counts[2] > 0, counts
    assert [_compact(o) for o in ora["per"]] == [True, False, True]


def test_view_that_sees_nothing_between_two_that_do(gpu_device):
    """The middle camera is turned round: no key but ~0, an empty range (kmin > kmax), so the view is not compact and carries 32-bit
    keys of ~0 through four passes between two views that narrow theirs."""
    scene = _turned_away_scene()
    ora = _oracle_views(scene)
    _turned_away_properties(ora)
    _check(scene, gpu_device, ora)


# ------------------------------------------------------------------------------------------------ the general scan
def test_more_than_64_chunks_per_view(gpu_device):
    """65 chunks per view, the fewest that take the general three-kernel scan of the depth sort's histograms: the key ranges are
    reduced behind that scan, and the compact view's fourth pass writes its stand-in histogram."""
    P = 64 * SORT_CHUNK + 1
    assert (P + SORT_CHUNK - 1) // SORT_CHUNK == 65
    scene = make_scene(P=P, res=(72, 40), s0=0.004, seed=37, view=[3])
    ora = _oracle_views(scene)
    assert _compact(ora["per"][0]) and ora["num_rendered"] > 0
    _check(scene, gpu_device, ora)


# ------------------------------------------------------------------------------------------------ two tile passes, the u32 stream
@functools.lru_cache(maxsize=None)
def _scene_512():
    return make_scene(P=600, res=(512, 512), s0=0.02, seed=19, view=range(9))


def test_two_tile_passes_and_seventy_views(gpu_device):
    """70 views of 512^2: 1,024 tiles (two tile passes, 5 + 5 bits) and (view << 10 | tile) in the u32 group stream, behind narrow
    depth keys in every view."""
    cams = [i % 9 for i in range(70)]
    assert ((len(cams) - 1) << 10 | 1023) > 0xFFFF
    per = [run_oracle(_scene_512(), c) for c in range(9)]
    assert all(_compact(o) for o in per)
    h, _ = _check(_views(_scene_512(), cams), gpu_device, _joined([per[c] for c in cams]))
    assert h["num_rendered"] > 0


# ------------------------------------------------------------------------------------------------ status and capacity
def test_overflow_by_one_reports_the_oracles_count(gpu_device):
    """A workspace one instance short of the call's count: F3DG_ERR_OVERFLOW with exactly the oracle's count, and after growing the
    lists are the oracle's."""
    scene = make_scene(P=1000, res=(72, 40), s0=0.05, seed=23, view=[0, 3, 6])
    ora = _oracle_views(scene)
    assert all(_compact(o) for o in ora["per"])
    R = ora["num_rendered"]
    cap = R - 1
    assert 0 < cap < R
    dev = lambda t: None if t is None else t.to(gpu_device)
    _, _, ws = f3d.rasterize_views(
        dev(scene["means3D"]), dev(scene["opacities"]), dev(scene["viewmatrix"]), dev(scene["projmatrix"]), dev(scene["campos"]),
        dev(scene["bg"]), image_height=scene["H"], image_width=scene["W"], tanfovx=scene["tanfovx"], tanfovy=scene["tanfovy"],
        sh=dev(scene["shs"]), scales=dev(scene["scales"]), rotations=dev(scene["rotations"]), sh_degree=scene["sh_degree"],
        max_rendered=cap, check=False, tile_cull=False, small_path=False)
    assert ws.max_rendered == cap
    n = C.c_longlong(0)
    rc = _lib.lib().f3dg_read_status(C.c_void_p(torch.cuda.current_stream().cuda_stream), C.c_void_p(ws.buffer.data_ptr()), C.byref(n))
    assert rc == _lib.ERR_OVERFLOW and n.value == R, (rc, n.value, R)
    h, _ = _check(scene, gpu_device, ora, max_rendered=cap)
    assert h["workspace"].max_rendered >= R
