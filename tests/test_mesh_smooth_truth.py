"""The restatement of tests/mesh_smooth_truth.py checked on the CPU: against an independent dense route (0/1 adjacency matrix, D^-1 A - I) on
small meshes, the properties Taubin smoothing is chosen for on a noisy icosphere, the boundary of an open grid, Euler's formula on closed
meshes, and the mesh PLY with and without normals. No GPU, no library call."""
import numpy as np
import pytest

import mesh_smooth_truth as S
from f3dgaus_amd import ply


def _small():
    cases = dict(S.small_cases())
    cases["fan 7"] = S.closed_fan(7)
    cases["strip 9"] = S.strip(9)
    f, N, _ = S.grid(5, 4)
    cases["grid 5x4"] = (f, N)
    v, f = S.icosphere(1)
    cases["icosphere 80"] = (f, len(v))
    return cases


@pytest.mark.parametrize("name", sorted(_small()))
def test_restatement_agrees_with_the_dense_route(name):
    faces, N = _small()[name]
    adj = S.adjacency(faces, N)
    P = S.rand_vertices(N, seed=11)
    pinned = (np.arange(N) % 5 == 0).astype(np.uint8)
    worst = 0.0
    for pin in (None, pinned):
        for s in (0.5, -0.53, 1.0):
            want, A = S.dense_step(P, faces, N, pin, s)
            got = S.smooth_step(P, adj["nbr_start"], adj["nbr"], pin, s, exact=True)
            worst = max(worst, float(np.abs(got - want).max()))
            # |p| <= 1 and |s| <= 1: a handful of float64 roundings of numbers of magnitude <= 3
            assert np.abs(got - want).max() <= 16 * np.finfo(np.float64).eps, (name, s)
            assert np.array_equal(S.smooth_step(P, adj["nbr_start"], adj["nbr"], pin, s), got.astype(np.float32))
    # every incidence row is strictly ascending, and the pairs are np.unique's
    start, key, _ = S.incidence(faces, N)
    owner = np.repeat(np.arange(N), np.diff(start))
    assert all((key[start[v] + 1:start[v + 1]] > key[start[v]:start[v + 1] - 1]).all() for v in range(N))
    pairs = np.unique((owner.astype(np.int64) << 32) | (key >> np.uint64(32)).astype(np.int64))
    assert np.array_equal(pairs & 0xFFFFFFFF, adj["nbr"]) and np.array_equal(np.bincount(pairs >> 32, minlength=N), np.diff(adj["nbr_start"]))
    # the CSR is the matrix: distinct neighbours, ascending
    for v in range(N):
        assert np.array_equal(adj["nbr"][adj["nbr_start"][v]:adj["nbr_start"][v + 1]], np.nonzero(A[v])[0]), (name, v)
    assert adj["counts"][0] == int(A.sum())
    print(f"{name}: N {N}, 2E {adj['counts'][0]}, max |restatement - dense| {worst:.3e}")


def test_boundary_and_counts_of_the_small_cases():
    c = S.small_cases()
    a = S.adjacency(*c["one triangle"])
    assert a["boundary"].tolist() == [1, 1, 1] and a["counts"] == [6, 3, 0, 2] and a["nbr"].tolist() == [1, 2, 0, 2, 0, 1]
    a = S.adjacency(*c["two on an edge"])
    assert a["counts"] == [10, 4, 0, 4] and a["nbr_start"].tolist() == [0, 2, 5, 8, 10]         # the shared edge is listed once per end
    a = S.adjacency(*c["tetrahedron"])
    assert a["counts"] == [12, 0, 0, 6] and not a["boundary"].any()
    a = S.adjacency(*c["oddities"])
    assert a["counts"][2] == 2 and np.diff(a["nbr_start"]).tolist() == [2, 3, 3, 4, 2, 0, 2, 0]
    # an edge with three faces is non-manifold, not boundary
    a = S.adjacency(np.array([[0, 1, 2], [0, 1, 3], [0, 1, 4]]), 5)
    rows = {v: a["nbr"][a["nbr_start"][v]:a["nbr_start"][v + 1]].tolist() for v in range(5)}
    assert rows[0] == [1, 2, 3, 4] and a["boundary"].tolist() == [1, 1, 1, 1, 1]                 # (0,2) (0,3) (0,4) are boundary edges
    a = S.adjacency(np.array([[0, 1, 2], [0, 1, 3], [0, 1, 4], [0, 2, 1], [0, 3, 1], [0, 4, 1]]), 5)
    assert not a["boundary"].any() and a["counts"][3] == 12                                      # every edge has two or six entries


def test_taubin_removes_noise_without_the_laplacian_shrinkage():
    v, f = S.icosphere(3, noise=0.02, seed=4)
    adj = S.adjacency(f, len(v))
    r0, d0 = S.radial_stats(v)
    taubin = S.smooth(v, adj["nbr_start"], adj["nbr"], None, 10, 0.5, -0.53)
    laplace = S.smooth(v, adj["nbr_start"], adj["nbr"], None, 10, 0.5, 0.0)
    rt, dt = S.radial_stats(taubin)
    rl, dl = S.radial_stats(laplace)
    print(f"icosphere {len(f)} faces: radius {r0:.5f} rms {d0:.5f}; Taubin {rt:.5f} rms {dt:.5f}; Laplacian {rl:.5f} rms {dl:.5f}")
    assert dt < d0
    assert abs(rt - r0) < abs(rl - r0)
    assert np.array_equal(S.smooth(v, adj["nbr_start"], adj["nbr"], None, 0), v)                 # no iteration: the input


def test_open_grid_rim_is_the_boundary_and_stays_when_pinned():
    f, N, v = S.grid(9, 7)
    adj = S.adjacency(f, N)
    rim = S.grid_rim(9, 7)
    assert np.array_equal(adj["boundary"].astype(bool), rim) and adj["counts"][1] == int(rim.sum()) == 2 * (9 + 7) - 4
    out = S.smooth(v, adj["nbr_start"], adj["nbr"], adj["boundary"], 10)
    assert np.array_equal(out[rim].view(np.uint32), v[rim].view(np.uint32)) and (out[~rim] != v[~rim]).any(axis=1).all()
    free = S.smooth(v, adj["nbr_start"], adj["nbr"], None, 10)
    assert (free[rim] != v[rim]).any()
    n = S.normals(v, f, N, adj)
    assert (n[:, 2] > 0).all() and np.abs(np.linalg.norm(n.astype(np.float64), axis=1) - 1).max() < 1e-6


@pytest.mark.parametrize("case", ["tetrahedron", "icosphere 0", "icosphere 2"])
def test_euler_formula_on_closed_genus_0_meshes(case):
    if case == "tetrahedron":
        f, N = S.small_cases()[case]
        v = np.array([[1, 1, 1], [1, -1, -1], [-1, 1, -1], [-1, -1, 1]], dtype=np.float32)
    else:
        v, f = S.icosphere(int(case.split()[1]))
        N = len(v)
    adj = S.adjacency(f, N)
    E = adj["counts"][0] // 2
    assert N - E + len(f) == 2 and not adj["boundary"].any() and adj["counts"][2] == 0
    n = S.normals(v, f, N, adj)
    assert ((n.astype(np.float64) * v).sum(1) > 0).all()                                          # outward winding, outward normals


def test_normals_of_vertices_without_a_face_and_of_collapsed_faces_are_zero():
    faces, N = S.small_cases()["oddities"]
    P = S.rand_vertices(N, 3)
    n = S.normals(P, faces, N)
    assert not n[5].any() and not n[7].any() and n[[0, 1, 2, 3, 4, 6]].any(axis=1).all()
    flat = np.zeros((3, 3), np.float32)                                                         # a face of zero area
    assert not S.normals(flat, np.array([[0, 1, 2]]), 3).any()
    # one triangle: the normal of its plane at every corner
    tri = np.array([[0, 0, 0], [2, 0, 0], [0, 3, 0]], np.float32)
    assert np.array_equal(S.normals(tri, np.array([[0, 1, 2]]), 3), np.tile(np.float32([0, 0, 1]), (3, 1)))


def _write_mesh_ply_as_before(path, v, f, colors=None):
    """The writer as it was before normals could be written, restated: header, packed vertex rows, packed face rows."""
    v = np.ascontiguousarray(v, dtype="<f4").reshape(-1, 3)
    f = np.asarray(f).reshape(-1, 3)
    vdt = [("x", "<f4"), ("y", "<f4"), ("z", "<f4")]
    header = "ply\nformat binary_little_endian 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\n" % len(v)
    if colors is not None:
        vdt += [("red", "u1"), ("green", "u1"), ("blue", "u1")]
        header += "property uchar red\nproperty uchar green\nproperty uchar blue\n"
    header += "element face %d\nproperty list uchar int vertex_indices\nend_header\n" % len(f)
    vrows = np.zeros(len(v), dtype=vdt)
    vrows["x"], vrows["y"], vrows["z"] = v[:, 0], v[:, 1], v[:, 2]
    if colors is not None:
        vrows["red"], vrows["green"], vrows["blue"] = colors[:, 0], colors[:, 1], colors[:, 2]
    frows = np.zeros(len(f), dtype=[("n", "u1"), ("i", "<i4", (3,))])
    frows["n"] = 3
    frows["i"] = f
    with open(path, "wb") as out:
        out.write(header.encode("ascii") + vrows.tobytes() + frows.tobytes())


def test_mesh_ply_with_and_without_normals(tmp_path):
    v, f = S.icosphere(1, noise=0.05, seed=2)
    n = S.normals(v, f, len(v))
    rgb = np.random.default_rng(0).integers(0, 256, (len(v), 3)).astype(np.uint8)
    for colors in (None, rgb):
        a, b, c = str(tmp_path / "a.ply"), str(tmp_path / "b.ply"), str(tmp_path / "c.ply")
        ply.save_mesh_ply(a, v, f, colors)
        _write_mesh_ply_as_before(b, v, f, colors)
        assert open(a, "rb").read() == open(b, "rb").read()                                      # None: byte for byte the earlier file
        ply.save_mesh_ply(a, v, f, colors, vertex_normals=None)
        assert open(a, "rb").read() == open(b, "rb").read()
        ply.save_mesh_ply(c, v, f, colors, vertex_normals=n)
        head = open(c, "rb").read().split(b"end_header\n")[0].decode().splitlines()
        props = [ln.split()[-1] for ln in head if ln.startswith("property") and "list" not in ln]
        assert props == ["x", "y", "z", "nx", "ny", "nz"] + (["red", "green", "blue"] if colors is not None else [])
        three = ply.read_mesh_ply(c)
        assert len(three) == 3 and np.array_equal(three[0], v) and np.array_equal(three[1], f)
        rv, rf, rc, rn = ply.read_mesh_ply(c, with_normals=True)
        assert np.array_equal(rv, v) and np.array_equal(rf, f) and np.array_equal(rn.view(np.uint32), n.view(np.uint32))
        assert (rc is None) if colors is None else np.array_equal(rc, rgb)
        assert ply.read_mesh_ply(a, with_normals=True)[3] is None and len(ply.read_mesh_ply(a)) == 3
