"""Binning places the instances from block sums: one number per 256 consecutive depth positions of a view (gsort_gather_rects_kernel),
a view-local scan of them plus the views' totals (block_sums_scan_kernel, view_segments_kernel), the offsets inside a block rebuilt
from the rectangles (duplicate_sorted_kernel), and a per-view scan of the tile pass's histogram (tile_scan_kernel). The shapes here
are the ones at which that can go wrong. Every case holds the final list, the ranges and the count to the oracle's exactly (lists
without tile culling), and the images of the default, culled call to the plain transcription's (option reference_kernels) bit for bit.

The one-workgroup scans loop over their array in rounds and carry the sum of the earlier rounds (f3dg_scan.h: scan_array_in_place,
block_scan_exclusive). The last cases pin a second round of each, and each asserts first, from the oracle, that something the later
kernels READ lies in that round -- a round of zeros that nothing reads would pass with a wrong carry: gsort_scan_kernel (more than
4,096 entries = 16 chunks per view, Gaussians with a low key byte of 241 and up), block_sums_scan_kernel (more than 1,024 block sums
per view with instances in the blocks from 1,024 on, together with the general three-kernel scan of the depth sort, more than 64
chunks per view), tile_scan_kernel (more than 16,384 entries = 64 chunks of instances in a view of 256 tiles, instances in tiles
whose entries lie past the first round) and both scans of view_segments_kernel (more than 512 views, the 513th with instances).
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

DUP_CAP = 3072          # F3DG_DUP_CAP of f3dg_binning.hip: instances per output window of an instance-generation workgroup
SORT_CHUNK = 4096       # F3DG_SORT_CHUNK


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


def _depth_order_counts(o):
    """tiles_touched of one oracle view in the order binning walks the Gaussians: ascending (depth bits, id), the Gaussians that
    touch no tile last (their sort key is ~0)."""
    tiles = np.array(o["tiles_touched"], dtype=np.int64)
    key = np.where(tiles > 0, np.array(o["depths"], dtype=np.float32).view(np.uint32).astype(np.int64), 1 << 32)
    return tiles[np.argsort(key, kind="stable")]


def _compact(o):
    """gsort_compact of one oracle view: the keys (depth bits) of the Gaussians that touch a tile lie within 2^24 of kmin & ~0xFFFF."""
    k = np.array(o["depths"], dtype=np.float32).view(np.uint32)[np.array(o["tiles_touched"]) > 0].astype(np.int64)
    assert len(k) > 0
    return ((int(k.max()) - (int(k.min()) & ~0xFFFF)) >> 24) == 0


# ------------------------------------------------------------------------------------------------ P x V at 72 x 40
@functools.lru_cache(maxsize=None)
def _grid_scene(P):
    return make_scene(P=P, res=(72, 40), s0=0.05, seed=3, view=range(9))


@functools.lru_cache(maxsize=None)
def _grid_oracle(P, cam):
    return run_oracle(_grid_scene(P), cam)


@pytest.mark.parametrize("V", [1, 3, 9])
@pytest.mark.parametrize("P", [1, 255, 256, 257, 1000, 4097])
def test_partial_blocks_and_view_boundaries(P, V, gpu_device):
    """nb = ceil(P / 256) block sums per view: a partial last block, a view boundary inside the block-sum array at every alignment
    (nb = 1, 2, 4, 17), more views than XCDs. (run_hip keeps the one-view call on the general launch sequence.)"""
    scene = _views(_grid_scene(P), list(range(V)))
    ora = _joined([_grid_oracle(P, v) for v in range(V)])
    if P >= 255:
        assert ora["num_rendered"] > 0
    _check(scene, gpu_device, ora)


def test_one_tile_image(gpu_device):
    """16 x 12 pixels: one tile, no tile bits and no tile pass -- the bases of the instance-generation workgroups come from the
    general scan over the block sums, which also sets the status; the ranges from the group stream."""
    scene = make_scene(P=600, res=(16, 12), s0=0.05, seed=29, view=[0, 1, 2])
    h, ora = _check(scene, gpu_device)
    assert ora["num_rendered"] > 256 and all(o["num_rendered"] > 0 for o in ora["per"])


# ------------------------------------------------------------------------------------------------ views and blocks that hold nothing
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


def test_view_that_sees_nothing_between_two_that_do(gpu_device):
    """The middle camera is turned round (half a turn about its own y axis): a view total of 0 between two live views, and a view
    without chunks (cpv == 0) in the tile pass, whose neighbour's last digit ends at the start of the view after it."""
    scene = _turned_away_scene()
    ora = _oracle_views(scene)
    _turned_away_properties(ora)
    _check(scene, gpu_device, ora)


def _behind_scene():
    scene = make_scene(P=2000, res=(72, 40), s0=0.05, seed=7, view=[0, 2, 5])
    scene["means3D"] = scene["means3D"].clone()
    scene["means3D"][:1000, 2] = -1.0          # behind the first camera's near plane (and outside the other cameras' frusta)
    return scene


def _behind_properties(ora):
    for o in ora["per"]:
        c = _depth_order_counts(o)
        blocks = [int(c[b:b + 256].sum()) for b in range(0, len(c), 256)]
        assert blocks[0] > 0 and sum(1 for b in blocks if b == 0) >= 2, blocks


def test_trailing_blocks_of_culled_gaussians(gpu_device):
    """Half the Gaussians lie behind the near plane: they touch no tile, their keys sort last, so whole trailing blocks of every view have sum 0."""
    scene = _behind_scene()
    ora = _oracle_views(scene)
    _behind_properties(ora)
    _check(scene, gpu_device, ora)


# ------------------------------------------------------------------------------------------------ windows of the instance generation
def _over_cap_scene():
    scene = make_scene(P=300, res=(256, 256), s0=0.08, seed=11, view=[0, 4])
    scene["scales"] = scene["scales"].clone()
    scene["scales"][7] = 3.0
    scene["means3D"] = scene["means3D"].clone()
    scene["means3D"][7] = torch.tensor([0.0, 0.0, 7.5])          # (at this depth its run starts ~200 instances before a window's end)
    return scene


def _over_cap_properties(ora):
    whole_image_run_spans = []
    for o in ora["per"]:
        c = _depth_order_counts(o)[:256]
        assert int(o["tiles_touched"][7]) == 256, int(o["tiles_touched"][7])
        assert int(c.sum()) > 2 * DUP_CAP, int(c.sum())                       # more than two windows from the first block
        start = np.cumsum(c) - c
        spans = (start // DUP_CAP) != ((start + c - 1) // DUP_CAP)
        assert spans[c > 0].any()                                              # a run that spans two windows
        whole_image_run_spans.append(bool(spans[c == 256].any()))
    assert all(whole_image_run_spans), whole_image_run_spans                  # ... the 256-tile one among them


def test_block_over_the_window_capacity(gpu_device):
    """300 large Gaussians at 256^2 plus one that covers every tile: the first block of 256 depth positions emits several windows of
    F3DG_DUP_CAP instances with offsets rebuilt inside the workgroup, and runs -- the 256-tile one among them -- span windows."""
    scene = _over_cap_scene()
    ora = _oracle_views(scene)
    _over_cap_properties(ora)
    _check(scene, gpu_device, ora)


# ------------------------------------------------------------------------------------------------ depth sort
def _wide_depth_scene():
    return make_scene(P=1500, res=(72, 40), s0=0.05, seed=13, view=[0, 3], depth_range=(1.0, 30.0))


def _wide_depth_properties(ora):
    assert [_compact(o) for o in ora["per"]] == [False, False]


def test_wide_depth_range_takes_four_passes(gpu_device):
    """Depths over 1..30: the keys of every view span more than 2^24, so the depth sort is not compact and all four passes run -- the
    fourth one's histogram and scan included, which return at once for a compact view only."""
    scene = _wide_depth_scene()
    ora = _oracle_views(scene)
    _wide_depth_properties(ora)
    _check(scene, gpu_device, ora)


def _mixed_compact_scene():
    scene = make_scene(P=1500, res=(72, 40), s0=0.05, seed=17, view=[0, 3, 5])
    scene["means3D"] = scene["means3D"].clone()
    scene["means3D"][:40, 2] = 1.5            # close to the canonical camera, on its axis: out of the side views' frusta
    scene["means3D"][:40, :2] *= 0.1
    return scene


def _mixed_compact_properties(ora):
    flags = [_compact(o) for o in ora["per"]]
    assert flags[0] is False and True in flags[1:], flags


def test_compact_and_wide_views_in_one_call(gpu_device):
    """A few Gaussians close to the first camera, which the others do not see: the first view takes four passes while compact views of
    the same call skip the fourth one's histogram and scan."""
    scene = _mixed_compact_scene()
    ora = _oracle_views(scene)
    _mixed_compact_properties(ora)
    _check(scene, gpu_device, ora)


# ------------------------------------------------------------------------------------------------ two tile passes, the u32 stream
@functools.lru_cache(maxsize=None)
def _scene_512():
    return make_scene(P=2000, res=(512, 512), s0=0.02, seed=19, view=range(9))


@functools.lru_cache(maxsize=None)
def _oracle_512(cam):
    return run_oracle(_scene_512(), cam)


def test_two_tile_passes(gpu_device):
    """512^2: 1,024 tiles, the tile bits sorted in two passes (5 + 5), each with its own per-view scan; ranges from the final stream."""
    scene = _views(_scene_512(), [0, 1])
    h, _ = _check(scene, gpu_device, _joined([_oracle_512(0), _oracle_512(1)]))
    assert h["num_rendered"] > 0


def test_seventy_views_u32_stream(gpu_device):
    """70 views of 512^2: (view << 10 | tile) needs the u32 group stream. Held to the oracle, and -- view by view -- to the same views
    in calls of at most 64 that take the u16 stream."""
    cams = [i % 9 for i in range(70)]
    assert ((len(cams) - 1) << 10 | 1023) > 0xFFFF
    scene = _views(_scene_512(), cams)
    wide, _ = _check(scene, gpu_device, _joined([_oracle_512(c) for c in cams]))
    total = 0
    for a, b in ((0, 64), (64, 70)):
        part = _views(scene, list(range(a, b)))
        h = run_hip(part, gpu_device)
        R = h["num_rendered"]
        assert np.array_equal(wide["point_list"][total:total + R], h["point_list"][:R]), (a, b)
        wr = wide["ranges"][a:b].astype(np.int64)
        assert np.array_equal(wr - total * (wr.sum(-1, keepdims=True) > 0), h["ranges"].astype(np.int64)), (a, b)
        for k in ("out_color", "final_T", "n_contrib"):
            assert np.array_equal(wide[k][a:b].view(np.uint32), h[k].view(np.uint32)), (a, b, k)
        total += R
    assert total == wide["num_rendered"] > 0


# ------------------------------------------------------------------------------------------------ status and capacity
@pytest.mark.parametrize("short_by", ["one", "nine_tenths"])
def test_overflow_reports_the_oracles_count(short_by, gpu_device):
    """A workspace one instance short of the call's count, and one of a tenth of it: F3DG_ERR_OVERFLOW with exactly the oracle's count
    (the 64-bit total now comes from the views' totals), and after growing the lists are the oracle's."""
    scene = make_scene(P=1000, res=(72, 40), s0=0.05, seed=23, view=[0, 3, 6])
    ora = _oracle_views(scene)
    R = ora["num_rendered"]
    cap = R - 1 if short_by == "one" else R // 10
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


def test_capacity_far_above_the_count_takes_the_general_tile_scan(gpu_device):
    """The tile pass's histogram is scanned per view while the capacity allows at most 512 chunks per view on average; a workspace
    carved for more clears the table and takes the general scan, whose zero tail supplies the end of the last digit. Same lists."""
    scene = make_scene(P=1000, res=(72, 40), s0=0.05, seed=23, view=[0, 3, 6])
    cap = 3 * 512 * SORT_CHUNK + SORT_CHUNK
    assert (cap + SORT_CHUNK - 1) // SORT_CHUNK + 3 > 512 * 3
    h, _ = _check(scene, gpu_device, max_rendered=cap)
    assert h["workspace"].max_rendered == cap


# ------------------------------------------------------------------------------------------------ later rounds of the one-workgroup scans
def test_depth_sort_scan_second_round(gpu_device):
    """17 chunks per view: a view's [256][17] histogram block is 4,352 entries, more than the 4,096 (1,024 threads x 4) of one round of
    gsort_scan_kernel -- the second round starts from the first one's carry. Two views: the second one's scan starts at P."""
    P = 65537
    cps = (P + SORT_CHUNK - 1) // SORT_CHUNK
    assert cps == 17 and 256 * cps > 1024 * 4 and cps <= 64
    scene = make_scene(P=P, res=(72, 40), s0=0.01, seed=31, view=[0, 3])
    ora = _oracle_views(scene)
    for o in ora["per"]:        # digit d's entries are [17 d, 17 d + 17): the first pass reads the second round's for d >= 241
        low = np.array(o["depths"], dtype=np.float32).view(np.uint32)[np.array(o["tiles_touched"]) > 0] & 255
        assert o["num_rendered"] > 0 and int((low >= -(-4096 // cps)).sum()) > 0
    _check(scene, gpu_device, ora)


@pytest.mark.parametrize("P", [262400, 266240])
def test_general_depth_sort_scan_and_block_sums_second_round(P, gpu_device):
    """65 chunks per view: the depth sort's histograms take the general three-kernel scan (and a compact view's fourth pass its stand-in
    histogram); more than 1,024 block sums per view: block_sums_scan_kernel takes a second round. At P = 262,400 that round is the one
    block 1,024, which holds Gaussians that touch no tile only (they sort last): the round runs, but its carry reaches no instance. At
    P = 266,240 (1,040 blocks) blocks of the second round hold instances: their workgroups' bases and the view's total need the carry."""
    nb = (P + 255) // 256
    assert (P + SORT_CHUNK - 1) // SORT_CHUNK == 65 > 64 and nb > 1024
    scene = make_scene(P=P, res=(72, 40), s0=0.004, seed=37, view=[3])
    ora = _oracle_views(scene)
    c = _depth_order_counts(ora["per"][0])
    assert int(c[:1024 * 256].sum()) > 0
    if P == 266240:
        assert int(c[1024 * 256:].sum()) > 0
    _check(scene, gpu_device, ora)


def _tile_scan_rounds(ora):
    """Of one view: entries of its block of the tile pass's histogram, and the instances in tiles whose entries -- digit d's are
    [d chunks, (d + 1) chunks) -- start past the first round of tile_scan_kernel (1,024 threads x 16)."""
    chunks = (ora["num_rendered"] + SORT_CHUNK - 1) // SORT_CHUNK
    r = ora["ranges"][0].astype(np.int64)
    n = r[:, 1] - r[:, 0]
    return 256 * chunks, int(n[np.arange(len(n)) * chunks >= 1024 * 16].sum())


def test_tile_scan_second_round(gpu_device):
    """One view of more than 64 chunks of instances: its [256][chunks] block of the tile pass's histogram is more than the 16,384
    entries of one round of tile_scan_kernel, in a workspace that still takes the per-view scan. 15 tiles: the digits in use end at
    entry 15 x 79, so the second round runs over zeros that nothing reads -- it must end, no more (the next case reads it)."""
    scene = make_scene(P=30000, res=(72, 40), s0=0.2, seed=43, view=[3])
    ora = _oracle_views(scene)
    assert _tile_scan_rounds(ora)[0] > 1024 * 16
    h, _ = _check(scene, gpu_device, ora)
    assert (h["workspace"].max_rendered + SORT_CHUNK - 1) // SORT_CHUNK + 1 <= 512 * 1


def test_tile_scan_second_round_is_read(gpu_device):
    """256 tiles (one 8-bit pass, every digit a tile) and 118 chunks of instances in the one view: the entries of the tiles from 139 on
    lie in the second round of tile_scan_kernel, and the scatter and the ranges read them."""
    scene = make_scene(P=20000, res=(256, 256), s0=0.05, seed=53, view=[3])
    ora = _oracle_views(scene)
    entries, read_past_first = _tile_scan_rounds(ora)
    assert 1024 * 16 < entries <= 2 * 1024 * 16 and read_past_first > 0
    h, _ = _check(scene, gpu_device, ora)
    assert (h["workspace"].max_rendered + SORT_CHUNK - 1) // SORT_CHUNK + 1 <= 512 * 1


@functools.lru_cache(maxsize=None)
def _tiny_scene():
    return make_scene(P=40, res=(32, 16), s0=0.05, seed=47, view=range(9))


def test_view_segment_scans_second_round(gpu_device):
    """513 views of two tiles: view_segments_kernel's scans of the views' totals and of their chunk counts take a second round of
    512 views, whose one view -- it has instances -- starts where the 512 before it end."""
    cams = [i % 9 for i in range(513)]
    scene = _views(_tiny_scene(), cams)
    V, T = len(cams), ((scene["W"] + 15) // 16) * ((scene["H"] + 15) // 16)
    assert V > 512 and T == 2 and ((V - 1) << 1 | 1) <= 0xFFFF          # one tile pass, u16 group stream
    per = [run_oracle(_tiny_scene(), c) for c in range(9)]
    assert all(o["num_rendered"] > 0 for o in per), [o["num_rendered"] for o in per]
    _check(scene, gpu_device, _joined([per[c] for c in cams]))
