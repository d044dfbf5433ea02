"""The restatement of the mesh simplification (tests/mesh_simplify_truth.py) against its independent plain-Python route, and the
properties the definition of include/f3dg.h promises (no GPU)."""
import numpy as np
import pytest

import mesh_simplify_truth as T
from mesh_smooth_truth import icosphere, small_cases


def _cases():
    """name -> (vertices, faces, origin, cell, attrs)"""
    rng = np.random.default_rng(11)
    out = {}
    v, f = T.bumpy_grid(13, 11)
    out["bumpy grid"] = (v, f, (-1.0, -1.0, -2.0), 2.5, T.colors_for(len(v)))
    v, f = icosphere(2, noise=0.02, seed=1)
    out["icosphere"] = (v, f, (-1.5, -1.5, -1.5), 0.4, T.colors_for(len(v), 5))
    v, f = T.two_sheets(5)
    out["two sheets"] = (v, f, (-0.5, -0.5, 0.0), 1.0, None)
    v, f, c = T.fan_in_one_cell(40)
    out["fan"] = (v, f, (0.0, 0.0, 0.0), 1.0, c)
    f, N = small_cases()["oddities"]                                               # degenerate faces, unreferenced vertices
    out["oddities"] = (rng.uniform(0, 4, (N, 3)).astype(np.float32), f, (0.0, 0.0, 0.0), 1.5, T.colors_for(N, 1))
    v, f = T.cube(6)
    out["small cube"] = (v, f, (-1.25, -1.25, -1.25), 0.7, None)
    # random soup: repeated faces in both windings, degenerate faces, many collapses
    v = rng.uniform(0, 3, (60, 3)).astype(np.float32)
    f = rng.integers(0, 60, (399, 3))
    f[::7] = f[1::7][:, [1, 0, 2]]
    out["soup"] = (v, f, (0.0, 0.0, 0.0), 0.75, T.colors_for(60, 2))
    return out


CASES = _cases()


@pytest.mark.parametrize("placement", T.PLACEMENTS)
@pytest.mark.parametrize("name", sorted(CASES))
def test_restatement_equals_the_independent_route(name, placement):
    v, f, origin, cell, attrs = CASES[name]
    a, b = T.simplify(v, f, origin, cell, placement, attrs), T.independent(v, f, origin, cell, placement, attrs)
    assert T.same(a, b), (name, placement, a["counts"], b["counts"])


@pytest.mark.parametrize("name", sorted(CASES))
def test_invariants(name):
    v, f, origin, cell, attrs = CASES[name]
    r = T.simplify(v, f, origin, cell, "mean", attrs)
    clusters, n, deg, col, dup, kept, biggest = r["counts"]
    F, N = len(np.asarray(f).reshape(-1, 3)), len(v)
    assert deg + col + dup + kept == F                                            # the counting identity
    fo = r["faces"]
    assert fo.shape == (kept, 3) and r["vertices"].shape == (n, 3) and len(r["cluster_root"]) == n
    assert ((fo[:, 0] != fo[:, 1]) & (fo[:, 1] != fo[:, 2]) & (fo[:, 0] != fo[:, 2])).all()        # three distinct ids
    assert len(np.unique(np.sort(fo, axis=1), axis=0)) == kept                    # no two faces share an id set
    assert np.array_equal(np.unique(fo), np.arange(n))                            # every output vertex is used
    root, vmap = r["cluster_root"], r["vertex_map"]
    assert (np.diff(root) > 0).all() and np.array_equal(vmap[root], np.arange(n))         # inverse on the used roots
    assert ((vmap >= -1) & (vmap < n)).all() and clusters >= n and 1 <= biggest <= N
    assert np.array_equal(np.bincount(vmap[vmap >= 0], minlength=n), r["cluster_size"])
    assert np.all(np.diff(r["kept_faces"]) > 0)                                   # survivors keep their input order
    # ... and their own winding: the surviving face's corners, mapped, in its own order
    assert np.array_equal(fo, vmap[np.asarray(f).reshape(-1, 3)[r["kept_faces"]]])
    # every placement shares the combinatorics
    for placement in ("root", "quadric"):
        o = T.simplify(v, f, origin, cell, placement, attrs)
        assert o["counts"] == r["counts"] and np.array_equal(o["faces"], fo) and np.array_equal(o["vertex_map"], vmap)
    assert np.array_equal(T.simplify(v, f, origin, cell, "root")["vertices"], np.asarray(v, np.float32)[root])      # bit for bit


def test_duplicates_keep_the_lower_id_in_either_winding():
    v = np.array([[0.5, 0.5, 0], [2.5, 0.5, 0], [0.5, 2.5, 0], [0.6, 0.4, 0.1], [2.4, 0.6, 0.1], [0.4, 2.6, 0.1]], np.float32)
    for second in ([3, 4, 5], [3, 5, 4], [5, 4, 3]):
        r = T.simplify(v, [[0, 1, 2], second], (0, 0, 0), 1.0, "root")
        assert r["counts"] == [3, 3, 0, 0, 1, 1, 2] and r["kept_faces"].tolist() == [0] and r["faces"].tolist() == [[0, 1, 2]]
    r = T.simplify(v, [[5, 4, 3], [0, 1, 2]], (0, 0, 0), 1.0, "root")
    assert r["kept_faces"].tolist() == [0] and r["faces"].tolist() == [[2, 1, 0]]         # the survivor's own winding


def test_everything_collapses_inside_one_cell_and_nothing_across_three():
    v = np.array([[0.1, 0.1, 0.1], [0.9, 0.2, 0.1], [0.2, 0.9, 0.3]], np.float32)
    r = T.simplify(v, [[0, 1, 2]], (0, 0, 0), 1.0)
    assert r["counts"] == [1, 0, 0, 1, 0, 0, 3] and r["vertices"].shape == (0, 3) and r["vertex_map"].tolist() == [-1, -1, -1]
    r = T.simplify(v, [[0, 1, 2]], (0, 0, 0), 0.5, "mean")
    assert r["counts"] == [3, 3, 0, 0, 0, 1, 1] and np.array_equal(r["vertices"], v) and r["faces"].tolist() == [[0, 1, 2]]


def test_cell_boundaries_and_refusals():
    # a coordinate equal to the origin and -0.0 are in cell 0; a coordinate on a boundary belongs to the upper cell
    v = np.array([[0.0, -0.0, 0.0], [1.0, 0.0, 0.0], [0.99999994, 0.5, 0.0], [2.0, 2.0, 2.0]], np.float32)
    k = T.cell_keys(v, (0, 0, 0), 1.0)
    assert k.tolist() == [0, 1, 0, 2 | 2 << 21 | 2 << 42]
    assert T.cell_keys(np.array([[-1.5, -1.5, -1.5]], np.float32), (-1.5, -1.5, -1.5), 0.25).tolist() == [0]
    far = np.array([[float(T.CELLS), 0, 0]], np.float32)
    assert T.cell_keys(far - np.array([1, 0, 0], np.float32), (0, 0, 0), 1.0).tolist() == [T.CELLS - 1]
    for bad in (far, np.array([[-1e-3, 0, 0]], np.float32), np.array([[np.nan, 0, 0]], np.float32), np.array([[0, np.inf, 0]], np.float32)):
        with pytest.raises(ValueError):
            T.cell_keys(bad, (0, 0, 0), 1.0)
    with pytest.raises(ValueError, match="face id"):
        T.simplify(v, [[0, 1, 4]], (0, 0, 0), 1.0)


def test_a_cell_below_the_least_separation_only_cleans():
    """No two vertices share a cell: what is left is the input without its degenerate faces and the vertices no other face uses -- the
    mesh clean_mesh with no criteria describes --, for every placement, the coordinates bit for bit."""
    rng = np.random.default_rng(5)
    N = 50
    v = (rng.permutation(N)[:, None] * 0.5 + rng.uniform(0.0, 0.2, (N, 3))).astype(np.float32)     # x, y, z all >= 0.3 apart
    f = np.stack([rng.permutation(N)[:30], rng.permutation(N)[:30], rng.permutation(N)[:30]], 1)
    f = f[np.sort(np.unique(np.sort(f, 1), axis=0, return_index=True)[1])]           # (no repeated id sets)
    f[3] = [f[3, 0], f[3, 0], f[3, 2]]
    live = f[(f[:, 0] != f[:, 1]) & (f[:, 1] != f[:, 2]) & (f[:, 0] != f[:, 2])]
    assert len(np.unique(np.sort(live, 1), axis=0)) == len(live)
    used = np.unique(live)
    new = np.full(N, -1)
    new[used] = np.arange(len(used))
    for placement in T.PLACEMENTS:
        r = T.simplify(v, f, (0.0, 0.0, 0.0), 0.25, placement)
        assert r["counts"] == [N, len(used), len(f) - len(live), 0, 0, len(live), 1]
        assert np.array_equal(r["faces"], new[live]) and np.array_equal(r["cluster_root"], used) and np.array_equal(r["vertex_map"], new)
        assert r["vertices"].tobytes() == v[used].tobytes(), placement


def test_a_planar_grid_under_quadric_is_the_mean_to_the_bit():
    v, f = T.plane_grid(31, 23)
    c = T.colors_for(len(v))
    m, q = T.simplify(v, f, (-0.5, -0.5, 0.0), 2.5, "mean", c), T.simplify(v, f, (-0.5, -0.5, 0.0), 2.5, "quadric", c)
    assert m["counts"][1] > 50 and T.same(m, q)
    assert (q["vertices"][:, 2] == np.float32(0.25)).all()


def test_quadric_keeps_the_edges_and_corners_of_a_cube():
    """The cube [-1, 1]^3, 32 x 32 quads a side (edge 1/16), clustered at a cell of three edges from the origin -1 - 1.5 edges on every
    axis: the cube's planes lie 1.5 and 0.5 edges inside their cells and no lattice coordinate falls on a cell boundary. The largest
    distance of a `quadric` vertex from the cube's surface is at most 1/100 of the largest under `mean`: the regulariser leaves a fraction
    mu / (lambda_min + mu) <= 1e-3 of the mean's offset in a constrained direction, and 1/100 leaves a factor of ten for unequal face
    counts in a cell."""
    v, f = T.cube()
    assert len(v) == 6 * 32 * 32 + 2 and len(f) == 12 * 32 * 32
    mean = T.simplify(v, f, T.CUBE_ORIGIN, T.CUBE_CELL, "mean")
    quad = T.simplify(v, f, T.CUBE_ORIGIN, T.CUBE_CELL, "quadric")
    assert mean["counts"] == quad["counts"] and mean["counts"][1] < len(v) // 5
    d_mean, d_quad = T.cube_distance(mean["vertices"]).max(), T.cube_distance(quad["vertices"]).max()
    print("cube: largest distance from the surface under mean %.6g, under quadric %.6g, ratio %.3g" % (d_mean, d_quad, d_quad / d_mean))
    assert d_mean > 0.25 * T.CUBE_EDGE                                             # the mean does cut the corners
    assert d_quad <= d_mean / 100.0
    # the eight corner clusters sit on the corners
    corner = np.abs(quad["vertices"]).min(axis=1) > 1.0 - T.CUBE_EDGE
    assert corner.sum() == 8 and np.abs(np.abs(quad["vertices"][corner]) - 1.0).max() < 1e-3 * T.CUBE_EDGE * 10
