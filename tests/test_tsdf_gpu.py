"""GPU tests of the TSDF mesh route: f3dg_tsdf_integrate through ctypes, the cell / tetrahedron / vertex entries through
f3dgaus_amd.tsdf.TSDFVolume on hand-made volumes, the route end to end on an analytic sphere, and mesh.extract_mesh_tsdf on a synthetic
blob. Truth, fixtures, the fragile-voxel rule and the tolerance are tests/tsdf_truth.py: outside the fragile voxels weight and
color_weight are exact and tsdf weight, color color_weight lie within 4 E_ref + 1e-6 max|.| of the float64 restatement. Every figure is
printed before it is asserted (``pytest -s``).

Shapes: the integration volume is 40 x 33 x 27 (no multiple of a wave or a workgroup along any axis, 140 workgroups) under five 48 x 40
views; the chunking case 165 views (one past a full camera table and a ragged rest) of 8 x 8 pixels; the cell volumes 37 x 21 x 19
(51 workgroups of cells, a sparse active set), 2 x 2 x 2 (one cell) and 129 x 129 x 66 (4,160 workgroups of cells: the count scan's second
round begins at workgroup 4,097; cells and tets only); the sphere 48^3."""
import ctypes as C

import numpy as np
import pytest
import torch

from f3dgaus_amd import _lib, mesh, ply, synthetic, tsdf
import tsdf_truth as T

pytestmark = pytest.mark.gpu
STATE = ("tsdf", "weight", "color", "color_weight")


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _upload(state, dev):
    return {k: torch.from_numpy(np.ascontiguousarray(state[k], dtype=np.float32)).to(dev) for k in STATE}


def _download(state):
    return {k: state[k].cpu().numpy() for k in STATE}


def _same(a, b):
    return all(torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)) for k in STATE)


def _raw_integrate(c, dev, views, state=None, use_color=True, use_alpha=True, z_near=T.Z_NEAR, alpha_min=None):
    """f3dg_tsdf_integrate of the case's ``views`` (a slice) on ``state`` (device tensors, modified in place; a new empty one when None)."""
    nx, ny, nz = c["dims"]
    if state is None:
        state = _upload(T.empty_state(c["dims"]), dev)
    depth = torch.from_numpy(np.ascontiguousarray(c["depth"][views])).to(dev)
    color = torch.from_numpy(np.ascontiguousarray(c["color"][views])).to(dev) if use_color else None
    alpha = torch.from_numpy(np.ascontiguousarray(c["alpha"][views])).to(dev) if use_alpha else None
    wv = torch.from_numpy(np.ascontiguousarray(c["world_view"][views])).to(dev)
    origin = (C.c_float * 3)(*[float(v) for v in c["origin"]])
    amin = c.get("alpha_min", T.ALPHA_MIN) if alpha_min is None else alpha_min
    rc = _lib.lib().f3dg_tsdf_integrate(_stream(), nx, ny, nz, origin, float(c["voxel"]), float(c["trunc"]), z_near, depth.shape[0], c["H"], c["W"],
                                        _lib.ptr(depth), _lib.ptr(color), _lib.ptr(alpha), amin, _lib.ptr(wv), float(c["fx"]), float(c["fy"]),
                                        _lib.ptr(state["tsdf"]), _lib.ptr(state["weight"]), _lib.ptr(state["color"]), _lib.ptr(state["color_weight"]))
    assert rc == _lib.OK, rc
    torch.cuda.synchronize()
    return state


@pytest.mark.parametrize("use_alpha", [True, False])
@pytest.mark.parametrize("use_color", [True, False])
def test_integrate_against_the_float64_restatement(gpu_device, use_color, use_alpha):
    c = T.integration_case()
    t = T.case_truth(c, use_color, use_alpha)
    print(f"color={use_color} alpha={use_alpha}: observed {t['observed']} fragile share {t['share']:.4f}")
    assert t["share"] <= T.FRAGILE_CAP
    state = _upload(T.empty_state(c["dims"]), gpu_device)
    if not use_color:                       # without a colour the two colour arrays are untouched, whatever they hold
        state["color"].fill_(7.25)
        state["color_weight"].fill_(-3.0)
    got = _download(_raw_integrate(c, gpu_device, slice(0, 5), state, use_color, use_alpha))
    T.check_state(got, t["s64"], t["fragile"], t["e_ref"], label=f"C ABI color={use_color} alpha={use_alpha}", use_color=use_color)
    if not use_color:
        assert (got["color"] == 7.25).all() and (got["color_weight"] == -3.0).all()
    else:
        assert (got["color_weight"] <= got["weight"]).all() and (got["color_weight"] < got["weight"]).any()       # free space is not tinted
    assert np.abs(got["tsdf"]).max() <= 1.0


def test_special_cameras_touch_nothing(gpu_device):
    """The camera that looks away and the one with 1e30 / NaN entries leave a filled volume bitwise unchanged by their own calls; the
    camera inside the volume leaves the voxels behind its z_near alone."""
    c = T.integration_case()
    base = _raw_integrate(c, gpu_device, slice(0, 2))
    for v in (3, 4):
        after = _raw_integrate(c, gpu_device, slice(v, v + 1), {k: t.clone() for k, t in base.items()})
        assert _same(after, base), v
    inside = _download(_raw_integrate(c, gpu_device, slice(2, 3)))
    want = T.run_case(c, slice(2, 3))
    keep = ~T.case_truth(c)["fragile"]
    assert np.array_equal(inside["weight"][keep], want["weight"][keep]) and 0 < (inside["weight"] > 0).sum() < inside["weight"].size
    Z = T.voxel_centres(c["origin"], c["voxel"], c["dims"], np.float64) @ c["world_view"][2].reshape(4, 4)[:3, 2].astype(np.float64) + float(c["world_view"][2][14])
    behind = (Z < T.Z_NEAR - T.MARGIN).reshape(inside["weight"].shape)
    assert behind.any() and not inside["weight"][behind].any()


def test_accumulation_in_two_calls(gpu_device):
    """Views [0:2] then [2:5] give the weights of all five at once and a mean within the same tolerance."""
    c = T.integration_case()
    t = T.case_truth(c)
    state = _raw_integrate(c, gpu_device, slice(0, 2))
    state = _raw_integrate(c, gpu_device, slice(2, 5), state)
    got = _download(state)
    T.check_state(got, t["s64"], t["fragile"], t["e_ref"], label="two calls")
    once = _download(_raw_integrate(c, gpu_device, slice(0, 5)))
    assert np.array_equal(got["weight"], once["weight"]) and np.array_equal(got["color_weight"], once["color_weight"])


def test_bitwise_reproducible_and_one_launch(gpu_device):
    c = T.integration_case()
    L = _lib.lib()
    a = _raw_integrate(c, gpu_device, slice(0, 5))
    L.f3dg_debug_launch_count(1)
    b = _raw_integrate(c, gpu_device, slice(0, 5))
    assert int(L.f3dg_debug_launch_count(1)) == 1          # five views: one launch
    assert _same(a, b)


def test_more_views_than_the_camera_table_equal_consecutive_calls(gpu_device):
    """165 views of 8 x 8 pixels (the table holds 128): one call chunks by itself into two launches and equals the calls [0:128], [128:165]
    to the bit."""
    V, H, W = _lib.TSDF_MAX_VIEWS + 37, 8, 8
    rng = np.random.default_rng(11)
    ang = rng.uniform(0, 2 * np.pi, V)
    eyes = np.stack([2.5 * np.cos(ang), rng.uniform(-0.8, 0.8, V), 2.5 * np.sin(ang)], 1)
    wv = np.stack([T.look_at(e, (0, 0, 0)) for e in eyes]).astype(np.float32).reshape(V, 16)
    c = {"dims": (12, 10, 9), "voxel": np.float32(0.1), "trunc": np.float32(0.4), "origin": (np.float32(-0.55), np.float32(-0.45), np.float32(-0.4)),
         "H": H, "W": W, "fx": np.float32(9.0), "fy": np.float32(10.0), "world_view": wv,
         "depth": rng.uniform(2.0, 3.0, (V, H, W)).astype(np.float32), "color": rng.random((V, 3, H, W)).astype(np.float32),
         "alpha": rng.uniform(0.3, 1.0, (V, H, W)).astype(np.float32)}
    L = _lib.lib()
    L.f3dg_debug_launch_count(1)
    once = _raw_integrate(c, gpu_device, slice(0, V))
    assert int(L.f3dg_debug_launch_count(1)) == 2
    twice = _raw_integrate(c, gpu_device, slice(0, _lib.TSDF_MAX_VIEWS))
    twice = _raw_integrate(c, gpu_device, slice(_lib.TSDF_MAX_VIEWS, V), twice)
    assert _same(once, twice)
    assert float(once["weight"].max()) > _lib.TSDF_MAX_VIEWS / 4 and float(once["color_weight"].max()) > 0          # the views do see the volume


# ------------------------------------------------------------------------------------------------ cells, tets, vertices
def _hand_volume(dims, seed):
    """A hand-made volume: free space (+0.5, weight 2) with negative blobs, exact zeros, a NaN, weights below / exactly at min_weight."""
    nx, ny, nz = dims
    rng = np.random.default_rng(seed)
    s = T.empty_state(dims)
    z, y, x = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    t = np.full((nz, ny, nx), 0.5, np.float32)
    for cx, cy, cz, r in ((6, 5, 4, 3.3), (28, 14, 12, 4.1), (17, 9, 15, 2.2)):
        if cx < nx and cy < ny and cz < nz:
            d = np.sqrt((x - cx) ** 2 + (y - cy) ** 2 + (z - cz) ** 2)
            t = np.minimum(t, np.clip((d - r) / 4.0, -1, 1).astype(np.float32))
    s["tsdf"] = t
    s["weight"][:] = 2.0
    s["color"] = rng.random((3, nz, ny, nx)).astype(np.float32)
    s["color_weight"] = (rng.random((nz, ny, nx)) < 0.7).astype(np.float32) * 2
    return s


def _volume(dims, state, dev, voxel=0.05, origin=(-0.91, 0.37, 1.13)):
    vol = tsdf.TSDFVolume(origin, voxel, dims, device=dev)
    for k in STATE:
        getattr(vol, k).copy_(torch.from_numpy(np.ascontiguousarray(state[k], dtype=np.float32)))
    return vol


def _check_mesh(vol, state, min_weight, label):
    """n_active, tets, interp_v and faces equal the restatement exactly; vertices and vertex colours within 2 ulp of the largest
    coordinate (colour) of the float32 restatement.

    The bound: the restatement forms the lattice positions p = origin + voxel * index and w = t_f / (t_f - t_o) with the same single
    float32 operations on the same inputs, each correctly rounded, so the kernel's p and w are the restatement's to the bit. What is
    left is the three-operation interpolation p_f + (p_o - p_f) * w: a difference, a product and a sum, each rounded to half an ulp of a
    result no larger than the largest coordinate (colour) M -- 1.5 ulp(M) if every one of them were evaluated differently (a fused
    multiply-add, say), under the 2 ulp(M) = 2 x 2^-23 M asserted. The library is built without contraction, so 0 is expected."""
    dims = vol.dims
    s32 = {k: np.asarray(state[k], dtype=np.float32) for k in STATE}
    want = T.mesh_of(s32, vol.origin, vol.voxel_size, dims, min_weight=min_weight, dtype=np.float32)
    tets = vol.surface_tets(min_weight)
    assert tets.dtype == torch.int32 and tets.shape == (6 * want["n_active"], 4), (label, tets.shape, want["n_active"])
    assert np.array_equal(tets.cpu().numpy(), want["tets"]), label
    m = vol.extract(min_weight)
    assert np.array_equal(m["tets"].cpu().numpy(), want["tets"])
    assert np.array_equal(m["interp_v"].cpu().numpy(), want["interp_v"]) and np.array_equal(m["faces"].cpu().numpy(), want["faces"]), label
    E = len(want["interp_v"])
    assert m["vertices"].shape == (E, 3) and m["vertex_colors"].shape == (E, 3)
    if E:
        v, col = m["vertices"].cpu().numpy().astype(np.float64), m["vertex_colors"].cpu().numpy().astype(np.float64)
        big = np.abs(np.asarray(vol.origin)) + vol.voxel_size * (np.asarray(dims) - 1)
        bound_v, bound_c = 2 * 2.0 ** -23 * float(big.max()), 2 * 2.0 ** -23 * float(np.nanmax(np.abs(s32["color"])))
        err_v, err_c = np.abs(v - want["vertices"].astype(np.float64)).max(), np.abs(col - want["vertex_colors"].astype(np.float64)).max()
        print(f"{label}: {want['n_active']} active cells, E {E}, faces {len(want['faces'])}; vertex err {err_v:.3e} (bound {bound_v:.3e}) colour err {err_c:.3e} (bound {bound_c:.3e})")
        assert np.isfinite(v).all() and np.isfinite(col).all()
        assert err_v <= bound_v and err_c <= bound_c
    return want, m


def test_cells_tets_and_vertices_on_a_sparse_volume(gpu_device):
    dims = (37, 21, 19)
    s = _hand_volume(dims, 0)
    s["tsdf"][4, 5, 9] = np.nan                      # a NaN corner on the first blob's surface: its eight cells are inactive
    s["weight"][10:14, 12:16, 30:34] = 0.5           # below min_weight across the second blob's surface
    s["weight"][15, 9, 15] = 1.0                     # exactly min_weight: still active
    s["tsdf"][15, 9, 19] = 0.0                       # tsdf == 0 corners: free, not occupied
    s["tsdf"][15, 11, 17] = 0.0
    s["tsdf"][2, 5, 6] = -0.0
    s["color_weight"][4, 5, 8:11] = 0.0              # ends without a colour next to ends with one ...
    s["color_weight"][15:17, 9:12, 15:20] = 0.0      # ... and edges where neither end has one
    want, m = _check_mesh(_volume(dims, s, gpu_device), s, 1.0, "37 x 21 x 19")
    n_cells = 36 * 20 * 18
    assert 200 < want["n_active"] < n_cells // 8 and len(want["faces"]) > 0           # sparse, over several workgroups
    _, _, active = T.cells_tets(s["tsdf"], s["weight"], 1.0)
    ids = np.flatnonzero(active.reshape(-1))
    assert ids.min() // 256 != ids.max() // 256
    # the colour fallbacks all occur: both ends, one end, no end
    cw = s["color_weight"].reshape(-1)
    have = (cw[want["interp_v"]] > 0).sum(1)
    assert set(have.tolist()) == {0, 1, 2}
    zero_rows = m["vertex_colors"].cpu().numpy()[have == 0]
    assert (zero_rows == 0).all()
    # another min_weight: the 0.5 region comes back, the weight-1 corner goes
    _check_mesh(_volume(dims, s, gpu_device), s, 0.5, "37 x 21 x 19, min_weight 0.5")
    _check_mesh(_volume(dims, s, gpu_device), s, 1.5, "37 x 21 x 19, min_weight 1.5")


def test_cells_edge_volumes(gpu_device):
    dev = gpu_device
    # no active cell: free space only -> 0 tets, an empty mesh, no error
    s = T.empty_state((9, 6, 5))
    s["tsdf"][:] = 0.25
    s["weight"][:] = 3.0
    want, m = _check_mesh(_volume((9, 6, 5), s, dev), s, 1.0, "free space")
    assert want["n_active"] == 0 and m["tets"].shape == (0, 4) and m["faces"].shape == (0, 3) and m["vertices"].shape == (0, 3)
    # an empty (all-zero) volume, and all weights below min_weight over a real surface
    e = T.empty_state((9, 6, 5))
    assert _check_mesh(_volume((9, 6, 5), e, dev), e, 1.0, "empty")[0]["n_active"] == 0
    s = _hand_volume((12, 11, 10), 1)
    s["weight"][:] = 0.75
    assert _check_mesh(_volume((12, 11, 10), s, dev), s, 1.0, "weights below min_weight")[0]["n_active"] == 0
    assert _check_mesh(_volume((12, 11, 10), s, dev), s, 0.75, "weights at min_weight")[0]["n_active"] > 0
    # one cell
    s = T.empty_state((2, 2, 2))
    s["tsdf"][:] = np.array([[[0.4, -0.2], [0.3, 0.1]], [[-0.6, 0.2], [0.0, 0.5]]], np.float32)
    s["weight"][:] = 1.0
    s["color"][:] = np.linspace(0, 1, 24, dtype=np.float32).reshape(3, 2, 2, 2)
    s["color_weight"][:] = 1.0
    want, _ = _check_mesh(_volume((2, 2, 2), s, dev), s, 1.0, "2 x 2 x 2")
    assert want["n_active"] == 1 and len(want["faces"]) > 0
    s["tsdf"][:] = -np.abs(s["tsdf"]) - 0.1
    assert _check_mesh(_volume((2, 2, 2), s, dev), s, 1.0, "2 x 2 x 2 all behind")[0]["n_active"] == 0


def test_cells_past_the_first_round_of_the_count_scan(gpu_device):
    """129 x 129 x 66: 1,064,960 cells in 4,160 workgroups, so the single-workgroup scan of the workgroup counts (4,096 per round)
    takes a second round. Three blobs in free space, one of them in the last z layers: its cells get their rows from the carry."""
    dims = (129, 129, 66)
    nx, ny, nz = dims
    s = T.empty_state(dims)
    z, y, x = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    t = np.full((nz, ny, nx), 0.5, np.float32)
    for cx, cy, cz, r in ((20, 30, 3, 5.3), (100, 90, 62, 6.1), (64, 64, 33, 4.2)):
        d = np.sqrt((x - cx) ** 2 + (y - cy) ** 2 + (z - cz) ** 2)
        t = np.minimum(t, np.clip((d - r) / 4.0, -1, 1).astype(np.float32))
    s["tsdf"] = t
    s["weight"][:] = 2.0
    n_active, want, active = T.cells_tets(s["tsdf"], s["weight"], 1.0)
    groups = np.flatnonzero(active.reshape(-1)) // 256
    print(f"129 x 129 x 66: {active.size} cells, {n_active} active in workgroups {groups.min()} .. {groups.max()}, {(groups >= 4096).sum()} at or beyond 4096")
    assert active.size == 1_064_960 and n_active == 1300
    assert groups.min() == 12 and groups.max() == 4143 and (groups >= 4096).sum() == 56
    tets = _volume(dims, s, gpu_device).surface_tets()
    assert tets.dtype == torch.int32 and tets.shape == (6 * n_active, 4)
    assert np.array_equal(tets.cpu().numpy(), want)


def test_emit_on_a_workspace_without_a_count_writes_nothing(gpu_device):
    """f3dg_tsdf_cells_emit on a zeroed workspace, and on the workspace of another volume's count, leaves the tets alone."""
    dev = gpu_device
    L = _lib.lib()
    dims = (12, 11, 10)
    s = _hand_volume(dims, 1)
    vol = _volume(dims, s, dev)
    n = vol.surface_tets().shape[0] // 6
    assert n > 0
    nbytes = L.f3dg_tsdf_cells_workspace_bytes(*dims)
    ws = torch.zeros(nbytes, dtype=torch.uint8, device=dev)
    tets = torch.full((6 * n, 4), -5, dtype=torch.int32, device=dev)
    assert L.f3dg_tsdf_cells_emit(_stream(), *dims, _lib.ptr(ws), nbytes, n, _lib.ptr(tets)) == _lib.OK
    torch.cuda.synchronize()
    assert bool((tets == -5).all())
    got = C.c_longlong(0)
    big = torch.zeros(max(nbytes, L.f3dg_tsdf_cells_workspace_bytes(11, 12, 10)), dtype=torch.uint8, device=dev)
    t2, w2 = vol.tsdf.reshape(10, 12, 11).contiguous(), vol.weight.reshape(10, 12, 11).contiguous()
    assert L.f3dg_tsdf_cells_count(_stream(), 11, 12, 10, 1.0, _lib.ptr(t2), _lib.ptr(w2), _lib.ptr(big), big.numel(), C.byref(got)) == _lib.OK
    assert L.f3dg_tsdf_cells_emit(_stream(), *dims, _lib.ptr(big), big.numel(), n, _lib.ptr(tets)) == _lib.OK
    torch.cuda.synchronize()
    assert bool((tets == -5).all())
    # a capacity below the count: only the first rows are written
    assert L.f3dg_tsdf_cells_count(_stream(), *dims, 1.0, _lib.ptr(vol.tsdf), _lib.ptr(vol.weight), _lib.ptr(ws), nbytes, C.byref(got)) == _lib.OK
    assert got.value == n
    assert L.f3dg_tsdf_cells_emit(_stream(), *dims, _lib.ptr(ws), nbytes, n - 1, _lib.ptr(tets)) == _lib.OK
    torch.cuda.synchronize()
    assert bool((tets[:6 * (n - 1)] >= 0).all()) and bool((tets[6 * (n - 1):] == -5).all())


# ------------------------------------------------------------------------------------------------ end to end
def test_sphere_end_to_end_on_the_device(gpu_device):
    c = T.e2e_case()
    assert c["fragile_share"] <= T.FRAGILE_CAP
    dev = gpu_device
    vol = tsdf.TSDFVolume(c["origin"], float(c["voxel"]), c["dims"], device=dev)
    assert vol.trunc == pytest.approx(float(c["trunc"]), rel=1e-6)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    vol.integrate(t(c["depth"]), t(c["world_view"].reshape(6, 4, 4)), (float(c["fx"]), float(c["fy"])), color=t(c["color"]), alpha=t(c["alpha"]),
                  alpha_min=c["alpha_min"], z_near=T.Z_NEAR)
    m = vol.extract()
    v, f = m["vertices"].cpu().numpy(), m["faces"].cpu().numpy()
    st, ref = T.mesh_stats(v, f, (0, 0, 0)), T.mesh_stats(c["mesh"]["vertices"], c["mesh"]["faces"], (0, 0, 0))
    print(f"sphere: {len(f)} faces (restatement {len(c['mesh']['faces'])}), volume {st['volume']:.6f} (restatement {ref['volume']:.6f}), "
          f"radii {st['radius'].min():.4f} .. {st['radius'].max():.4f} (restatement {ref['radius'].min():.4f} .. {ref['radius'].max():.4f})")
    assert st["closed"] and st["euler"] == 2
    assert len(set(st["out_sign"].tolist())) == 1 and st["out_sign"][0] > 0                 # one orientation: every normal points outward
    assert abs(st["volume"] - ref["volume"]) <= 1e-3 * abs(ref["volume"])
    assert st["radius"].min() >= ref["radius"].min() - float(c["voxel"]) and st["radius"].max() <= ref["radius"].max() + float(c["voxel"])
    col = m["vertex_colors"].cpu().numpy()
    assert np.isfinite(col).all() and col.min() >= 0 and col.max() <= 1
    # reset empties the volume
    vol.reset()
    assert not bool(vol.weight.any()) and vol.extract()["faces"].shape == (0, 3)


@pytest.fixture(scope="module")
def blob(f3d, gpu_device):
    """4,096 opaque Gaussians in a ball of radius 0.4 at the orbit's centre, colours inside [0, 1], 8 orbit cameras of 64^2."""
    dev = gpu_device
    P = 4096
    g = synthetic.make_gaussians(P, s0=0.04, seed=2, device="cpu")
    gen = torch.Generator().manual_seed(5)
    d = torch.randn(P, 3, generator=gen)
    g["xyz"] = (d / d.norm(dim=1, keepdim=True) * torch.rand(P, 1, generator=gen) ** (1 / 3) * 0.4 + torch.tensor([0.0, 0.0, 7.667])).float().contiguous()
    g["opacity"] = torch.full((P, 1), 0.95)
    g["features_dc"] = torch.rand(P, 1, 3, generator=gen) * 3.0 - 1.5            # 0.5 + 0.282 dc stays inside [0.07, 0.93]
    g["features_rest"] = torch.zeros(P, 3, 3)
    cams = synthetic.orbit_cameras(8, resolution=64, device=dev)
    pc = {k: v.to(dev)[None].contiguous() for k, v in g.items()}
    return pc, cams


def test_extract_mesh_tsdf_on_a_synthetic_blob(f3d, gpu_device, blob, tmp_path):
    pc, cams = blob
    dev = gpu_device
    bg = torch.zeros(3, device=dev)
    m = mesh.extract_mesh_tsdf(pc, 0, cams["viewmatrix"], cams["projmatrix"], cams["campos"], bg, cams["cfg"], resolution=32)
    v, f, col = m["vertices"], m["faces"], m["vertex_colors"]
    print(f"blob: {v.shape[0]} vertices, {f.shape[0]} faces, {m['tets'].shape[0] // 6} active cells")
    assert v.shape[0] > 0 and f.shape[0] > 0 and int(f.max()) < v.shape[0] and int(f.min()) >= 0
    assert bool(torch.isfinite(v).all()) and bool(torch.isfinite(col).all())
    lo, hi = pc["xyz"][0].min(0)[0], pc["xyz"][0].max(0)[0]
    voxel = float((hi - lo).max()) / (32 - 9)               # the box of the Gaussians padded by trunc = 4 voxels; the lattice that covers
    pad = 4 * voxel * 1.001 + 1e-4                          # it starts at the padded corner and may end up to one voxel past the other
    assert bool((v >= lo - pad).all()) and bool((v <= hi + pad + voxel).all())      # inside the volume
    assert float(col.min()) >= 0.0 and float(col.max()) <= 1.0
    again = mesh.extract_mesh_tsdf(pc, 0, cams["viewmatrix"], cams["projmatrix"], cams["campos"], bg, cams["cfg"], resolution=32)
    assert all(torch.equal(m[k], again[k]) for k in ("vertices", "faces", "vertex_colors", "interp_v", "tets"))
    # explicit bounds and truncation
    b = mesh.extract_mesh_tsdf(pc, 0, cams["viewmatrix"], cams["projmatrix"], cams["campos"], bg, cams["cfg"], resolution=24,
                               bounds=((-0.6, -0.6, 7.0), (0.6, 0.6, 8.3)), trunc=0.2)
    assert b["faces"].shape[0] > 0 and bool((b["vertices"] >= torch.tensor([-0.6, -0.6, 7.0], device=dev) - 1e-4).all())
    # PLY round trip with colours
    rgb8 = (col.clamp(0, 1) * 255).round().to(torch.uint8)
    p = str(tmp_path / "tsdf_mesh.ply")
    ply.save_mesh_ply(p, v, f, rgb8)
    rv, rf, rc = ply.read_mesh_ply(p)
    assert np.array_equal(rv, v.cpu().numpy()) and np.array_equal(rf, f.cpu().numpy()) and np.array_equal(rc, rgb8.cpu().numpy())


def test_grad_and_host_tensors_raise(f3d, gpu_device, blob):
    dev = gpu_device
    vol = tsdf.TSDFVolume((0.0, 0.0, 0.0), 0.1, (8, 8, 8), device=dev)
    depth, wv = torch.ones(2, 16, 16, device=dev), torch.eye(4, device=dev).repeat(2, 1, 1)
    color = torch.rand(2, 3, 16, 16, device=dev)
    for kw in (dict(depth=depth.clone().requires_grad_()), dict(world_views=wv.clone().requires_grad_()), dict(color=color.clone().requires_grad_()),
               dict(alpha=depth.clone().requires_grad_())):
        a = dict(depth=depth, world_views=wv, color=color, alpha=None)
        a.update(kw)
        with pytest.raises(NotImplementedError, match="no gradient"):
            vol.integrate(a["depth"], a["world_views"], 30.0, color=a["color"], alpha=a["alpha"])
    with torch.no_grad():                   # under no_grad such a tensor is data
        vol.integrate(depth.clone().requires_grad_(), wv, 30.0, color=color)
    for kw in (dict(depth=depth.cpu()), dict(world_views=wv.cpu()), dict(color=color.cpu()), dict(alpha=depth.cpu())):
        a = dict(depth=depth, world_views=wv, color=color, alpha=None)
        a.update(kw)
        with pytest.raises(RuntimeError, match="HIP device"):
            vol.integrate(a["depth"], a["world_views"], 30.0, color=a["color"], alpha=a["alpha"])
    with pytest.raises(TypeError):
        vol.integrate(depth.double(), wv, 30.0)
    with pytest.raises(ValueError):
        vol.integrate(depth, wv[:1], 30.0)
    pc, cams = blob
    host = {k: v.cpu() for k, v in pc.items()}
    with pytest.raises(RuntimeError, match="HIP device"):
        mesh.extract_mesh_tsdf(host, 0, cams["viewmatrix"], cams["projmatrix"], cams["campos"], torch.zeros(3, device=dev), cams["cfg"], resolution=32)
