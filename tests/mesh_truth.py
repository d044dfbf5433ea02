"""numpy restatement of the marching-tetrahedra topology (src/utils_tetmesh.py:47-138 of the reference) and the small meshes the mesh
tests share. Test infrastructure, like fwd_truth.py: tests/test_marching_tets.py holds it to the reference's own outputs
(tests/golden/marching_tets.npz), the GPU tests hold the library to it.

Semantics: a point is occupied when sdf > 0 (NaN and 0 are outside); a tetrahedron is on the surface when 1..3 of its corners are; its
case index is sum occ_i 2^i over its corners as given; its edges are (0,1) (0,2) (0,3) (1,2) (1,3) (2,3) with the ends sorted. Only an
edge with exactly one occupied end reaches the output: interp_v is the ascending lexicographic unique of those, faces index it."""
import itertools
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "marching_tets.npz")
CASES = ("single", "outside", "dup_nan_zero", "kuhn3", "kuhn6")          # the fixture's cases (tests/tools/gen_mesh_golden.py)

TRIANGLE_TABLE = np.array([
    [-1, -1, -1, -1, -1, -1], [1, 0, 2, -1, -1, -1], [4, 0, 3, -1, -1, -1], [1, 4, 2, 1, 3, 4],
    [3, 1, 5, -1, -1, -1], [2, 3, 0, 2, 5, 3], [1, 4, 0, 1, 5, 4], [4, 2, 5, -1, -1, -1],
    [4, 5, 2, -1, -1, -1], [4, 1, 0, 4, 5, 1], [3, 2, 0, 3, 5, 2], [1, 3, 5, -1, -1, -1],
    [4, 1, 2, 4, 3, 1], [3, 0, 4, -1, -1, -1], [2, 0, 1, -1, -1, -1], [-1, -1, -1, -1, -1, -1]], dtype=np.int64)
NUM_TRIANGLES = np.array([0, 1, 1, 2, 1, 2, 2, 1, 1, 2, 2, 1, 2, 1, 1, 0], dtype=np.int64)
EDGE_A = np.array([0, 0, 0, 1, 1, 2])
EDGE_B = np.array([1, 2, 3, 2, 3, 3])


def marching_tets(sdf, tets):
    """sdf [N] float, tets [F,4] int -> interp_v [E,2] int64, faces [n1 + 2 n2, 3] int64, stats dict."""
    sdf = np.asarray(sdf)
    tets = np.asarray(tets, dtype=np.int64).reshape(-1, 4)
    N = sdf.shape[0]
    occ = sdf > 0
    o = occ[tets]
    n_occ = o.sum(1)
    surface = (n_occ > 0) & (n_occ < 4)
    vt, vo = tets[surface], o[surface]
    a, b = vt[:, EDGE_A], vt[:, EDGE_B]                         # [S,6]
    lo, hi = np.minimum(a, b), np.maximum(a, b)
    crossing = vo[:, EDGE_A] != vo[:, EDGE_B]
    key = lo * N + hi                                           # lexicographic order of (lo, hi) as one integer
    uniq = np.unique(key[crossing])
    interp_v = np.stack([uniq // N, uniq % N], 1).astype(np.int64).reshape(-1, 2)
    row = np.where(crossing, np.searchsorted(uniq, key), -1)    # [S,6]: row of every crossing edge of the tetrahedron
    case = (vo * np.array([1, 2, 4, 8])).sum(1)
    nt = NUM_TRIANGLES[case]
    one, two = nt == 1, nt == 2
    f1 = np.take_along_axis(row[one], TRIANGLE_TABLE[case[one]][:, :3], 1).reshape(-1, 3)
    f2 = np.take_along_axis(row[two], TRIANGLE_TABLE[case[two]][:, :6], 1).reshape(-1, 3)
    faces = np.concatenate([f1, f2], 0).astype(np.int64)
    assert (faces >= 0).all()
    return interp_v, faces, {"surface": int(surface.sum()), "emitted": int(crossing.sum()), "n_one": int(one.sum()), "n_two": int(two.sum())}


def kuhn_grid(n):
    """n^3 lattice points on [0, 1]^3 (x slowest) and the 6 (n-1)^3 tetrahedra of the Kuhn split of every cell."""
    ax = np.linspace(0.0, 1.0, n, dtype=np.float32)
    pts = np.stack(np.meshgrid(ax, ax, ax, indexing="ij"), -1).reshape(-1, 3)
    idx = lambda i, j, k: (i * n + j) * n + k
    c = np.stack(np.meshgrid(np.arange(n - 1), np.arange(n - 1), np.arange(n - 1), indexing="ij"), -1).reshape(-1, 3)
    tets = []
    for perm in itertools.permutations(range(3)):
        corner = c.copy()
        path = [idx(*corner.T)]
        for axis in perm:
            corner = corner.copy()
            corner[:, axis] += 1
            path.append(idx(*corner.T))
        tets.append(np.stack(path, 1))
    tets = np.stack(tets, 1).reshape(-1, 4).astype(np.int64)
    return pts, tets


def permuted(tets, seed):
    """Seeded permutation of the rows and, independently per row, of the four corners."""
    rng = np.random.default_rng(seed)
    tets = tets[rng.permutation(len(tets))]
    order = np.argsort(rng.random(tets.shape), axis=1)
    return np.ascontiguousarray(np.take_along_axis(tets, order, 1))


def noisy_sphere_sdf(pts, seed, radius=0.37, noise=0.03, centre=(0.5, 0.5, 0.5)):
    """Positive inside a sphere, with seeded noise (float32)."""
    rng = np.random.default_rng(seed)
    d = np.linalg.norm(pts.astype(np.float64) - np.asarray(centre), axis=1)
    return (radius - d + rng.normal(0, noise, len(pts))).astype(np.float32)


def fan(centre_last=False, n_lat=40, n_lon=50, seed=5):
    """One inside vertex and an outside latitude-longitude shell of n_lat * n_lon vertices; one tetrahedron (centre, a, b, c) per
    shell triangle, corners permuted. centre_last=False: the centre is id 0, so every crossing edge lands in ONE bucket;
    centre_last=True: it is the last id, so every bucket holds one edge. Returns points, sdf, tets."""
    th = np.linspace(0.15, np.pi - 0.15, n_lat)
    ph = np.linspace(0.0, 2 * np.pi, n_lon, endpoint=False)
    T, P = np.meshgrid(th, ph, indexing="ij")
    shell = np.stack([np.sin(T) * np.cos(P), np.sin(T) * np.sin(P), np.cos(T)], -1).reshape(-1, 3)
    S = len(shell)
    sid = lambda i, j: i * n_lon + (j % n_lon)
    tri = []
    for i in range(n_lat - 1):
        for j in range(n_lon):
            tri.append((sid(i, j), sid(i + 1, j), sid(i, j + 1)))
            tri.append((sid(i, j + 1), sid(i + 1, j), sid(i + 1, j + 1)))
    tri = np.array(tri, dtype=np.int64)
    if centre_last:
        pts = np.concatenate([shell, np.zeros((1, 3))]).astype(np.float32)
        centre = S
    else:
        pts = np.concatenate([np.zeros((1, 3)), shell]).astype(np.float32)
        centre = 0
        tri = tri + 1
    sdf = np.full(S + 1, -1.0, dtype=np.float32)
    sdf[centre] = 1.0
    tets = np.concatenate([np.full((len(tri), 1), centre, dtype=np.int64), tri], 1)
    rng = np.random.default_rng(seed)
    tets = np.take_along_axis(tets, np.argsort(rng.random(tets.shape), axis=1), 1)
    return pts, sdf, np.ascontiguousarray(tets)
