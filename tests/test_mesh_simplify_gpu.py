"""GPU tests of the mesh simplification: f3dg_mesh_simplify_count / _emit through ctypes, mesh.simplify_mesh on top of them, and the TSDF
route with the new keyword. Truth and the shared cases are tests/mesh_simplify_truth.py. EVERY comparison is exact equality of bytes:
faces, vertex_map, roots, sizes, counts, and the float32 vertices and colours of all three placements (the kernel and the restatement
share the operation order and use IEEE + - * / and floor only, with one rounding to float32).

Shapes: one triangle inside one cell and across three; two triangles over the same three clusters in either winding; 63 / 64 / 65 and
255 / 256 / 257 vertices and faces (wave and workgroup edges) all in one cell and all in cells of their own; vertices on cell boundaries,
at the origin and at -0.0; clusters of 33 and of 5,000 members (both sides of the one-thread limit of the member-row sort, the second past
its LDS limit) with colours; two sheets closer than a cell; a 129 x 129 grid at 2.5 edges (int32 and int64 faces, three runs); the cube
of the quality test; a 513 x 513 grid once (the single-workgroup scans run many rounds, the face table holds 524,288 faces)."""
import ctypes as C

import numpy as np
import pytest
import torch

from f3dgaus_amd import _lib, mesh
import mesh_simplify_truth as T
from mesh_smooth_truth import small_cases

pytestmark = pytest.mark.gpu
SENT = -5
SENT_F = -123.25
_TRUTH = {}


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _truth(name, v, f, origin, cell, placement, attrs=None):
    """Computed once per (case, placement), shared, never modified."""
    key = (name, placement)
    if key not in _TRUTH:
        _TRUTH[key] = T.simplify(v, f, origin, cell, placement, attrs)
    return _TRUTH[key]


def _dev(a, dev, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    return t if dtype is None else t.to(dtype)


def _bytes_equal(t, a):
    a = np.ascontiguousarray(a)
    got = t.detach().cpu().numpy()
    return got.shape == a.shape and got.dtype == a.dtype and got.tobytes() == a.tobytes()


def _assert_equals_truth(r, want, what):
    assert [r["counts"][k] for k in T.COUNTS] == list(want["counts"]), (what, r["counts"], want["counts"])
    for k in ("faces", "vertex_map", "cluster_root", "cluster_size", "vertices"):
        assert _bytes_equal(r[k], want[k]), (what, k)
    if want["attrs"] is None:
        assert r["vertex_colors"] is None, what
    else:
        assert _bytes_equal(r["vertex_colors"], want["attrs"]), (what, "vertex_colors")


def _run_all(name, v, f, origin, cell, dev, attrs=None, dtype=torch.int64, placements=T.PLACEMENTS):
    vt, ft = _dev(v, dev), _dev(f, dev, dtype).reshape(-1, 3)
    ct = None if attrs is None else _dev(attrs, dev)
    out = {}
    for placement in placements:
        r = mesh.simplify_mesh(vt, ft, cell, origin=origin, placement=placement, vertex_colors=ct)
        _assert_equals_truth(r, _truth(name, v, f, origin, cell, placement, attrs), (name, placement))
        out[placement] = r
    return out


def _raw_count(vt, ft, origin, cell):
    """f3dg_mesh_simplify_count with a sentinel h_counts: (rc, h_counts, workspace)."""
    L = _lib.lib()
    N, F = vt.shape[0], ft.shape[0]
    nbytes = L.f3dg_mesh_simplify_workspace_bytes(N, F)
    assert nbytes > 0
    ws = torch.zeros(nbytes, dtype=torch.uint8, device=vt.device)
    h = (C.c_longlong * 8)(*([-7] * 8))
    rc = L.f3dg_mesh_simplify_count(_stream(), _lib.ptr(ws), nbytes, N, F, _lib.ptr(vt), _lib.ptr(ft), int(ft.dtype == torch.int32),
                                    (C.c_double * 3)(*origin), float(cell), h)
    torch.cuda.synchronize()
    return rc, list(h), ws


def _raw_emit(ws, vt, ft, placement, n, f, adj_ws=None, attrs=None):
    """f3dg_mesh_simplify_emit on outputs pre-filled with sentinels: (rc, vertices, faces, attrs, vertex_map, root, size)."""
    dev, N, F = vt.device, vt.shape[0], ft.shape[0]
    Cn = 0 if attrs is None else attrs.shape[1]
    vo = torch.full((n, 3), SENT_F, dtype=torch.float32, device=dev)
    ao = torch.full((n, Cn), SENT_F, dtype=torch.float32, device=dev) if Cn else None
    fo = torch.full((f, 3), SENT, dtype=torch.int64, device=dev)
    vmap, root, size = (torch.full((k,), SENT, dtype=torch.int64, device=dev) for k in (N, n, n))
    rc = _lib.lib().f3dg_mesh_simplify_emit(_stream(), _lib.ptr(ws), ws.numel(), N, F, _lib.ptr(vt), _lib.ptr(ft), int(ft.dtype == torch.int32),
                                            _lib.SIMPLIFY_PLACEMENT[placement], Cn, _lib.ptr(attrs), _lib.ptr(adj_ws),
                                            0 if adj_ws is None else adj_ws.numel(), n, f, _lib.ptr(vo), _lib.ptr(fo), _lib.ptr(ao), _lib.ptr(vmap),
                                            _lib.ptr(root), _lib.ptr(size))
    torch.cuda.synchronize()
    return rc, vo, fo, ao, vmap, root, size


def _untouched(outs):
    return all(o is None or bool((o == (SENT_F if o.dtype == torch.float32 else SENT)).all()) for o in outs)


# ------------------------------------------------------------------------------------------------ the smallest meshes
def test_one_triangle_inside_one_cell_and_across_three(f3d, gpu_device):
    v = np.array([[0.1, 0.1, 0.1], [0.9, 0.2, 0.1], [0.2, 0.9, 0.3]], np.float32)
    f = np.array([[0, 1, 2]])
    r = _run_all("tri in a cell", v, f, (0.0, 0.0, 0.0), 1.0, gpu_device, attrs=T.colors_for(3))
    for placement in T.PLACEMENTS:
        o = r[placement]
        assert o["vertices"].shape == (0, 3) and o["faces"].shape == (0, 3) and o["vertex_colors"].shape == (0, 3)
        assert o["vertex_map"].tolist() == [-1, -1, -1] and o["counts"]["collapsed"] == 1 and o["counts"]["clusters"] == 1
    r = _run_all("tri across three", v, f, (0.0, 0.0, 0.0), 0.5, gpu_device, attrs=T.colors_for(3))
    for placement in T.PLACEMENTS:
        o = r[placement]
        assert _bytes_equal(o["vertices"], v) and o["faces"].tolist() == [[0, 1, 2]] and _bytes_equal(o["vertex_colors"], T.colors_for(3))


@pytest.mark.parametrize("second", ([3, 4, 5], [4, 5, 3], [3, 5, 4], [5, 4, 3]))
def test_two_triangles_over_the_same_clusters(f3d, gpu_device, second):
    v = np.array([[0.5, 0.5, 0], [2.5, 0.5, 0], [0.5, 2.5, 0], [0.6, 0.4, 0.1], [2.4, 0.6, 0.1], [0.4, 2.6, 0.1]], np.float32)
    for faces in ([[0, 1, 2], second], [second, [0, 1, 2]]):
        r = _run_all("pair %s" % (faces,), v, np.array(faces), (0.0, 0.0, 0.0), 1.0, gpu_device)["mean"]
        assert r["counts"]["duplicate"] == 1 and r["counts"]["kept"] == 1
        assert r["faces"].tolist() == [r["vertex_map"][faces[0]].tolist()]          # the lower id survives, in its own winding


@pytest.mark.parametrize("n", (63, 64, 65, 255, 256, 257))
def test_wave_and_workgroup_edges(f3d, gpu_device, n):
    rng = np.random.default_rng(n)
    f = np.stack([rng.permutation(n), rng.permutation(n), rng.permutation(n)], 1)      # n faces over n vertices, a few of them degenerate
    inside = rng.uniform(0.1, 0.9, (n, 3)).astype(np.float32)
    r = _run_all("one cell %d" % n, inside, f, (0.0, 0.0, 0.0), 1.0, gpu_device, attrs=T.colors_for(n, 2))["quadric"]
    c = r["counts"]
    assert (c["clusters"], c["used_clusters"], c["kept"], c["max_cluster"]) == (1, 0, 0, n) and c["degenerate"] + c["collapsed"] == n
    apart = (rng.permutation(n)[:, None] * 1.0 + rng.uniform(0.1, 0.9, (n, 3))).astype(np.float32)
    r = _run_all("own cells %d" % n, apart, f, (0.0, 0.0, 0.0), 1.0, gpu_device, attrs=T.colors_for(n, 2), dtype=torch.int32)["quadric"]
    c = r["counts"]
    assert (c["clusters"], c["collapsed"], c["max_cluster"]) == (n, 0, 1) and c["degenerate"] + c["duplicate"] + c["kept"] == n


def test_vertices_on_cell_boundaries(f3d, gpu_device):
    """Coordinates equal to the origin, -0.0, exactly on a boundary (the upper cell's) and one float32 below it."""
    v = np.array([[0.0, -0.0, 0.0], [1.0, 0.0, 0.0], [0.99999994, 0.5, -0.0], [2.0, 2.0, 2.0], [-0.0, 1.0, 0.0], [0.25, 0.99999994, 0.0],
                  [2.0, 1.9999999, 2.0], [1.0, 1.0, 0.0], [3.0, 0.0, 0.5], [3.0, -0.0, 1.0]], np.float32)
    f = np.array([[0, 1, 4], [2, 7, 5], [0, 3, 6], [1, 7, 3], [8, 9, 3], [2, 1, 4], [5, 6, 8]])
    r = _run_all("boundaries", v, f, (0.0, 0.0, 0.0), 1.0, gpu_device, attrs=T.colors_for(len(v)))["root"]
    assert r["vertex_map"][0] == r["vertex_map"][2] == r["vertex_map"][5] and r["vertex_map"][0] != r["vertex_map"][1]
    w = v * np.float32(0.25) - np.float32(1.5)                                     # a negative origin and a cell that is no integer
    _run_all("boundaries moved", w, f, (-1.5, -1.5, -1.5), 0.25, gpu_device)
    # the degenerate faces and unused vertices of the smoothing suite, at a cell that merges nothing
    g, N = small_cases()["oddities"]
    p = (np.arange(N)[:, None] * 2.0 + np.array([0.5, 0.25, 0.75])).astype(np.float32)
    r = _run_all("oddities", p, g, (0.0, 0.0, 0.0), 1.0, gpu_device)["quadric"]
    assert r["counts"]["degenerate"] == 2 and r["counts"]["kept"] == 3 and r["vertex_map"].tolist() == [0, 1, 2, 3, 4, -1, 5, -1]


@pytest.mark.parametrize("members", (33, 5000))
def test_long_member_rows(f3d, gpu_device, members):
    v, f, colors = T.fan_in_one_cell(members)
    r = _run_all("fan %d" % members, v, f, (0.0, 0.0, 0.0), 1.0, gpu_device, attrs=colors)["quadric"]
    assert r["counts"]["max_cluster"] == members and r["counts"]["kept"] == members and int(r["cluster_size"].max()) == members
    assert r["counts"]["used_clusters"] == members + 2


def test_two_sheets_closer_than_a_cell(f3d, gpu_device):
    v, f = T.two_sheets(9)
    r = _run_all("sheets", v, f, (-0.5, -0.5, 0.0), 1.0, gpu_device, attrs=T.colors_for(len(v)))["mean"]
    c = r["counts"]
    assert c["duplicate"] == c["kept"] == len(f) // 2 and c["collapsed"] == 0 and c["used_clusters"] == 81 and c["max_cluster"] == 2
    assert _bytes_equal(r["faces"], f[:len(f) // 2])                               # the first sheet's faces survive


# ------------------------------------------------------------------------------------------------ grids and the cube
def test_grid_129_in_both_face_types_and_three_runs(f3d, gpu_device):
    v, f = T.bumpy_grid(129, 129)
    colors = T.colors_for(len(v))
    origin, cell = (-1.0, -1.0, -2.0), 2.5
    a = _run_all("grid 129", v, f, origin, cell, gpu_device, attrs=colors, dtype=torch.int64)
    b = _run_all("grid 129", v, f, origin, cell, gpu_device, attrs=colors, dtype=torch.int32)
    keys = ("vertices", "faces", "vertex_colors", "vertex_map", "cluster_root", "cluster_size")
    for placement in T.PLACEMENTS:
        assert all(torch.equal(a[placement][k], b[placement][k]) for k in keys) and a[placement]["counts"] == b[placement]["counts"]
    vt, ft, ct = _dev(v, gpu_device), _dev(f, gpu_device), _dev(colors, gpu_device)
    adjacency = mesh.mesh_adjacency(ft, len(v))
    for _ in range(3):
        again = mesh.simplify_mesh(vt, ft, cell, origin=origin, vertex_colors=ct, adjacency=adjacency)
        assert all(torch.equal(a["quadric"][k], again[k]) for k in keys) and again["counts"] == a["quadric"]["counts"]
    moved = int((a["quadric"]["vertices"] != a["mean"]["vertices"]).any(dim=1).sum())
    print("grid 129: %d -> %d vertices, %d -> %d faces; quadric moved %d off the mean" % (len(v), a["mean"]["vertices"].shape[0], len(f),
                                                                                         a["mean"]["faces"].shape[0], moved))
    assert moved > 0
    # origin=None is the vertices' minimum, grid_resolution the longest side of their box over it
    lo, hi = v.min(0).astype(np.float64), v.max(0).astype(np.float64)
    auto = mesh.simplify_mesh(vt, ft, grid_resolution=40, placement="mean", vertex_colors=ct)
    _assert_equals_truth(auto, T.simplify(v, f, lo, float((hi - lo).max()) / 40, "mean", colors), "grid_resolution")
    auto = mesh.simplify_mesh(vt, ft, 2.5, placement="root")
    _assert_equals_truth(auto, T.simplify(v, f, lo, 2.5, "root"), "origin=None")


def test_planar_grid_quadric_is_the_mean(f3d, gpu_device):
    v, f = T.plane_grid(65, 33)
    r = _run_all("plane", v, f, (-0.5, -0.5, 0.0), 2.5, gpu_device)
    assert torch.equal(r["quadric"]["vertices"], r["mean"]["vertices"]) and bool((r["quadric"]["vertices"][:, 2] == 0.25).all())


def test_cube_all_placements(f3d, gpu_device):
    v, f = T.cube()
    r = _run_all("cube", v, f, T.CUBE_ORIGIN, T.CUBE_CELL, gpu_device, attrs=T.colors_for(len(v)))
    d_mean = T.cube_distance(r["mean"]["vertices"].cpu().numpy()).max()
    d_quad = T.cube_distance(r["quadric"]["vertices"].cpu().numpy()).max()
    print("cube on the device: largest distance from the surface under mean %.6g, under quadric %.6g" % (d_mean, d_quad))
    assert d_quad <= d_mean / 100.0


def test_grid_513_once(f3d, gpu_device):
    v, f = T.bumpy_grid(513, 513)
    r = _run_all("grid 513", v, f, (-1.0, -1.0, -2.0), 2.5, gpu_device, attrs=T.colors_for(len(v)), placements=("quadric",))["quadric"]
    print("grid 513: %d -> %d vertices, %d -> %d faces" % (len(v), r["vertices"].shape[0], len(f), r["faces"].shape[0]))
    assert r["counts"]["kept"] > 0 and r["counts"]["degenerate"] == 0


# ------------------------------------------------------------------------------------------------ refusals on the device
def test_device_refusals_leave_everything_untouched(f3d, gpu_device):
    dev = gpu_device
    v, f = T.bumpy_grid(20, 17)
    origin, cell = (-1.0, -1.0, -2.0), 2.5
    want = _truth("grid 20", v, f, origin, cell, "mean")
    n, nf = want["counts"][1], want["counts"][5]
    vt, ft = _dev(v, dev), _dev(f, dev)
    adj = mesh.mesh_adjacency(ft, len(v))
    bad_face, nan_vertex, far_vertex, low_vertex = f.copy(), v.copy(), v.copy(), v.copy()
    bad_face[len(f) // 2, 1] = len(v)
    nan_vertex[77, 2] = np.nan
    far_vertex[300, 0] = np.float32(-1.0 + 2.5 * (1 << 21))                        # cell index 2^21
    low_vertex[5, 1] = np.float32(-1.0001)                                         # cell index -1
    neg_face = f.copy()
    neg_face[0, 0] = -1
    for what, vv, ff in (("face id N", v, bad_face), ("face id -1", v, neg_face), ("NaN", nan_vertex, f), ("cell 2^21", far_vertex, f),
                         ("cell -1", low_vertex, f)):
        vb, fb = _dev(vv, dev), _dev(ff, dev)
        rc, h, ws = _raw_count(vb, fb, origin, cell)
        assert rc == _lib.ERR_BAD_ARG and h == [-7] * 8, (what, rc, h)
        for placement in T.PLACEMENTS:                                            # no completed count on the workspace: nothing is written
            rc, *outs = _raw_emit(ws, vb, fb, placement, n, nf, adj_ws=adj["workspace"] if placement == "quadric" else None)
            assert rc == _lib.OK and _untouched(outs), (what, placement)
        with pytest.raises(_lib.F3dgError):
            mesh.simplify_mesh(vb, fb, cell, origin=origin, placement="mean")
    with pytest.raises(ValueError, match="not finite"):
        mesh.simplify_mesh(_dev(nan_vertex, dev), ft, cell)                       # origin=None: the box is read first
    # a good count, then: the quadric placement on an adjacency workspace that holds no completed build, and on another mesh's
    rc, h, ws = _raw_count(vt, ft, origin, cell)
    assert rc == _lib.OK and h[:7] == want["counts"] and h[7] == 0
    blank = torch.zeros_like(adj["workspace"])
    rc, *outs = _raw_emit(ws, vt, ft, "quadric", n, nf, adj_ws=blank)
    assert rc == _lib.OK and _untouched(outs)
    rc, *outs = _raw_emit(torch.zeros_like(ws), vt, ft, "mean", n, nf)
    assert rc == _lib.OK and _untouched(outs)
    # ... and the real thing through ctypes, the colours included
    colors = T.colors_for(len(v))
    rc, vo, fo, ao, vmap, root, size = _raw_emit(ws, vt, ft, "quadric", n, nf, adj_ws=adj["workspace"], attrs=_dev(colors, dev))
    q = _truth("grid 20", v, f, origin, cell, "quadric", colors)
    assert rc == _lib.OK and all(_bytes_equal(t, q[k]) for t, k in ((vo, "vertices"), (fo, "faces"), (ao, "attrs"), (vmap, "vertex_map"),
                                                                    (root, "cluster_root"), (size, "cluster_size")))
    # capacities below the counts: the rows beyond them are not written
    rc, vo, fo, ao, vmap, root, size = _raw_emit(ws, vt, ft, "mean", n - 3, nf - 5)
    assert rc == _lib.OK and _bytes_equal(vo, want["vertices"][:n - 3]) and _bytes_equal(fo, want["faces"][:nf - 5])
    assert _bytes_equal(root, want["cluster_root"][:n - 3]) and _bytes_equal(vmap, want["vertex_map"])
    # a mesh without faces: the clusters are counted, nothing survives
    rc, h, _ = _raw_count(vt, ft[:0], origin, cell)
    assert rc == _lib.OK and h == [want["counts"][0], 0, 0, 0, 0, 0, want["counts"][6], 0]
    r = mesh.simplify_mesh(vt, ft[:0], cell, origin=origin)
    assert r["vertices"].shape == (0, 3) and r["faces"].shape == (0, 3) and bool((r["vertex_map"] == -1).all())
    e = mesh.simplify_mesh(vt[:0], ft[:0], cell)
    assert e["vertices"].shape == (0, 3) and e["vertex_map"].shape == (0,) and e["counts"]["kept"] == 0


# ------------------------------------------------------------------------------------------------ the purpose, end to end
def test_extract_mesh_simplifies(f3d, gpu_device):
    """The tetrahedral route (the scene of its own suite, rebuilt here: 300 opaque Gaussians in a ball under 3 cameras of 64^2, a 9^3 Kuhn
    grid of spacing 0.15): without the keyword the dict is the earlier one; with it the earlier keys are untouched, the simplified mesh
    and its maps are added, and the normals are those of the simplified mesh."""
    import mesh_truth
    from f3dgaus_amd import cameras
    from helpers import make_scene
    dev = gpu_device
    P, centre = 300, (0.0, 0.0, 7.667)
    scene = make_scene(P=P, res=(64, 64), s0=0.08, seed=0, view=[0, 1, 3])
    g = torch.Generator().manual_seed(1)
    d = torch.randn(P, 3, generator=g)
    scene["means3D"] = (d / d.norm(dim=1, keepdim=True) * torch.rand(P, 1, generator=g) ** (1 / 3) * 0.3 + torch.tensor(centre)).float().contiguous()
    scene["opacities"] = torch.full((P, 1), 0.99)
    cfg = cameras.default_cfg(resolution=64)
    cfg["model"]["max_sh_degree"] = scene["sh_degree"]
    t = lambda k: scene[k].to(dev)
    pc = {"xyz": t("means3D")[None], "opacity": t("opacities")[None], "scaling": t("scales")[None], "rotation": t("rotations")[None],
          "features_dc": t("shs")[None, :, :1], "features_rest": t("shs")[None, :, 1:]}
    pts, tets = mesh_truth.kuhn_grid(9)
    pts = torch.from_numpy(((pts - 0.5) * 1.2 + np.array(centre, dtype=np.float32)).astype(np.float32)).to(dev)
    args = (pc, 0, pts, torch.full((len(pts), 1), 0.04, device=dev), torch.from_numpy(tets).to(dev), t("viewmatrix"), t("projmatrix"), t("campos"), t("bg"), cfg)
    plain = mesh.extract_mesh(*args)
    none = mesh.extract_mesh(*args, simplify_cell=None, simplify_placement="quadric")
    assert sorted(plain) == sorted(none) == ["faces", "faces_filtered", "keep", "vertices", "vertices_filtered"]
    assert all(torch.equal(plain[k], none[k]) for k in plain) and plain["faces_filtered"].shape[0] > 0
    got = mesh.extract_mesh(*args, simplify_cell=0.2, simplify_placement="mean", vertex_normals=True)
    assert sorted(got) == sorted(list(plain) + ["faces_simplified", "simplify", "vertex_normals", "vertices_simplified"])
    assert all(torch.equal(plain[k], got[k]) for k in plain) and sorted(got["simplify"]) == ["cluster_root", "counts", "vertex_map"]
    want = mesh.simplify_mesh(plain["vertices_filtered"], plain["faces_filtered"], 0.2, placement="mean")
    assert torch.equal(got["vertices_simplified"], want["vertices"]) and torch.equal(got["faces_simplified"], want["faces"])
    assert torch.equal(got["simplify"]["vertex_map"], want["vertex_map"]) and got["simplify"]["counts"] == want["counts"]
    assert torch.equal(got["vertex_normals"], mesh.vertex_normals(want["vertices"], want["faces"]))
    print("tetrahedral route: %d -> %d vertices, %d -> %d faces at a cell of 0.2" % (plain["vertices_filtered"].shape[0], want["vertices"].shape[0],
                                                                                    plain["faces_filtered"].shape[0], want["faces"].shape[0]))
    assert 0 < want["faces"].shape[0] < plain["faces_filtered"].shape[0]
    both = mesh.extract_mesh(*args, keep_largest=1, simplify_cell=0.2, smooth_iterations=2)
    s2 = mesh.simplify_mesh(both["vertices_clean"], both["faces_clean"], 0.2)
    assert torch.equal(both["vertices_simplified"], s2["vertices"])
    assert torch.equal(both["vertices_smooth"], mesh.smooth_mesh(s2["vertices"], s2["faces"], iterations=2)["vertices"])


def test_extract_mesh_tsdf_simplifies(f3d, gpu_device):
    """The synthetic blob of the TSDF suite (4,096 opaque Gaussians in a ball of radius 0.4, 8 orbit cameras of 64^2) fused into a 32^3
    volume, simplified at three voxels."""
    from f3dgaus_amd import synthetic
    dev = gpu_device
    Pn = 4096
    g = synthetic.make_gaussians(Pn, s0=0.04, seed=2, device="cpu")
    gen = torch.Generator().manual_seed(5)
    d = torch.randn(Pn, 3, generator=gen)
    g["xyz"] = (d / d.norm(dim=1, keepdim=True) * torch.rand(Pn, 1, generator=gen) ** (1 / 3) * 0.4 + torch.tensor([0.0, 0.0, 7.667])).float().contiguous()
    g["opacity"] = torch.full((Pn, 1), 0.95)
    g["features_dc"] = torch.rand(Pn, 1, 3, generator=gen) * 3.0 - 1.5
    g["features_rest"] = torch.zeros(Pn, 3, 3)
    cams = synthetic.orbit_cameras(8, resolution=64, device=dev)
    pc = {k: v.to(dev)[None].contiguous() for k, v in g.items()}
    args = (pc, 0, cams["viewmatrix"], cams["projmatrix"], cams["campos"], torch.zeros(3, device=dev), cams["cfg"])
    plain = mesh.extract_mesh_tsdf(*args, resolution=32)
    none = mesh.extract_mesh_tsdf(*args, resolution=32, simplify_cell=None, simplify_placement="quadric")
    assert sorted(plain) == sorted(none) == ["faces", "interp_v", "tets", "vertex_colors", "vertices"]
    assert all(torch.equal(plain[k], none[k]) for k in plain)                     # the defaults: today's dict, key for key
    cell = 0.1
    for placement in ("quadric", "root"):
        m = mesh.extract_mesh_tsdf(*args, resolution=32, simplify_cell=cell, simplify_placement=placement, vertex_normals=True)
        want = mesh.simplify_mesh(plain["vertices"], plain["faces"], cell, placement=placement, vertex_colors=plain["vertex_colors"])
        assert sorted(m) == sorted(list(plain) + ["simplify", "vertex_normals"]) and sorted(m["simplify"]) == ["cluster_root", "counts", "vertex_map"]
        assert all(torch.equal(m[k], want[k]) for k in ("vertices", "faces", "vertex_colors"))
        assert all(torch.equal(m["simplify"][k], want[k]) for k in ("vertex_map", "cluster_root")) and m["simplify"]["counts"] == want["counts"]
        assert torch.equal(m["vertex_normals"], mesh.vertex_normals(want["vertices"], want["faces"]))      # the later steps act on the result
        assert torch.equal(m["interp_v"], plain["interp_v"]) and torch.equal(m["tets"], plain["tets"])
    c = want["counts"]
    print("blob at 32^3: %d -> %d vertices, %d -> %d faces at a cell of %.2f" % (plain["vertices"].shape[0], c["used_clusters"],
                                                                                 plain["faces"].shape[0], c["kept"], cell))
    assert 0 < c["kept"] < plain["faces"].shape[0] // 2 and c["degenerate"] + c["collapsed"] + c["duplicate"] + c["kept"] == plain["faces"].shape[0]
    # ... and equals the restatement on the same mesh
    pv, pf = plain["vertices"].cpu().numpy(), plain["faces"].cpu().numpy()
    _assert_equals_truth(want, T.simplify(pv, pf, pv.min(0).astype(np.float64), cell, "root", plain["vertex_colors"].cpu().numpy()), "blob")
