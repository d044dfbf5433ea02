"""The TSDF route's restatement (tests/tsdf_truth.py) held to analytic facts, on the CPU: the band of a fronto-parallel plane, the Kuhn
split, the closed outward mesh of an analytic sphere volume, and the fragile-voxel cap of every case the GPU tests use."""
import itertools

import numpy as np

import mesh_truth
import tsdf_truth as T


def test_fronto_parallel_plane_gives_the_clamped_band():
    """A plane z = 1 seen by two cameras on the z axis (at z = -2 and z = -3, both looking along +z): inside the band every voxel holds
    clamp((d - Z) / trunc) = clamp((1 - z) / trunc), the same from both cameras; voxels more than trunc behind the plane hold nothing."""
    dims, voxel, trunc = (9, 8, 21), np.float32(0.05), np.float32(0.2)
    origin = (np.float32(-0.2), np.float32(-0.175), np.float32(0.5))
    H = W = 64
    f = np.float32(100.0)
    wv = np.stack([T.look_at((0, 0, -2.0), (0, 0, 1.0)), T.look_at((0, 0, -3.0), (0, 0, 1.0))]).astype(np.float32)
    depth = np.stack([np.full((H, W), 3.0, np.float32), np.full((H, W), 4.0, np.float32)])
    color = np.stack([np.full((3, H, W), 0.25, np.float32), np.full((3, H, W), 0.75, np.float32)])
    s = T.integrate(T.empty_state(dims), origin, voxel, dims, trunc, depth, wv, f, f, color=color)
    z = (np.float64(origin[2]) + np.float64(voxel) * np.arange(dims[2]))[:, None, None] * np.ones((1, dims[1], dims[0]))
    sdf = 1.0 - z
    seen = sdf >= -np.float64(trunc) - 1e-9
    near_edge = np.abs(sdf + np.float64(trunc)) < 1e-6
    want = np.minimum(1.0, sdf / np.float64(trunc))
    ok = ~near_edge
    assert np.array_equal(s["weight"][ok], np.where(seen, 2.0, 0.0)[ok])
    assert np.abs(s["tsdf"] - np.where(seen, want, 0.0))[ok].max() < 1e-6
    assert (s["tsdf"][ok & ~seen] == 0).all() and (s["weight"][ok & ~seen] == 0).all()          # nothing behind the band
    band = ok & (np.abs(sdf) < np.float64(trunc) - 1e-6)
    free = ok & (sdf > np.float64(trunc) + 1e-6)
    assert (s["color_weight"][band] == 2).all() and np.abs(s["color"][:, band] - 0.5).max() < 1e-12
    assert (s["color_weight"][free] == 0).all() and (s["color"][:, free] == 0).all()            # free space is not tinted
    # a second call accumulates: the same two views again double the weights and keep the means
    s2 = T.integrate(s, origin, voxel, dims, trunc, depth, wv, f, f, color=color)
    assert np.array_equal(s2["weight"], 2 * s["weight"]) and np.abs(s2["tsdf"] - s["tsdf"]).max() < 1e-12


def test_kuhn_tetrahedra_share_one_orientation_and_tile_the_cube():
    corners = T.kuhn_corners()
    assert corners.shape == (6, 4, 3)
    vols = [np.linalg.det((c[:3] - c[3]).astype(np.float64)) / 6.0 for c in corners]           # (v0 - v3) . ((v1 - v3) x (v2 - v3)) / 6
    assert all(abs(v - 1.0 / 6.0) < 1e-12 for v in vols), vols            # equal and positive: together the unit cube's volume
    assert all((c[0] == 0).all() and (c[3] == 1).all() for c in corners)   # all share the (0,0,0)-(1,1,1) diagonal
    # they tile the cube: every sample point lies in exactly one tetrahedron (barycentric coordinates all positive)
    rng = np.random.default_rng(0)
    pts = rng.random((2000, 3))
    inside = np.zeros(len(pts), dtype=np.int64)
    for c in corners:
        A = (c[1:] - c[0]).astype(np.float64).T
        lam = np.linalg.solve(A, pts.T).T
        inside += ((lam > 0).all(1) & (lam.sum(1) < 1)).astype(np.int64)
    assert (inside == 1).all()
    # the order of the header: xyz, xzy, yxz, yzx, zxy, zyx with the middle vertices of the even ones swapped
    assert T.KUHN_ORDERS == [(0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0)]
    assert corners[0].tolist() == [[0, 0, 0], [1, 1, 0], [1, 0, 0], [1, 1, 1]] and corners[1].tolist() == [[0, 0, 0], [1, 0, 0], [1, 0, 1], [1, 1, 1]]
    # on a lattice: the ids of a 3 x 4 x 5 volume's first and last cell
    n, tets, active = T.cells_tets(np.where(np.arange(60).reshape(5, 4, 3) % 2 == 0, -0.5, 0.5).astype(np.float32), np.ones((5, 4, 3), np.float32))
    assert n == 2 * 3 * 4 and active.all() and tets.shape == (6 * n, 4) and tets.dtype == np.int32
    assert tets[0].tolist() == [0, 1 + 3, 1, 1 + 3 + 12] and tets[5].tolist() == [0, 12, 3 + 12, 16]
    assert tets[-6].tolist() == [(3 * 4 + 2) * 3 + 1 + k for k in (0, 4, 1, 16)] and tets.max() == 59


def test_analytic_sphere_volume_gives_a_closed_outward_mesh():
    dims, voxel, radius = (30, 28, 26), 0.05, 0.45
    origin, tsdf, weight = T.analytic_sphere_volume(dims, voxel, radius, 4 * voxel)
    n_active, tets, _ = T.cells_tets(tsdf, weight)
    assert n_active > 0
    interp_v, faces, _ = mesh_truth.marching_tets(-tsdf.reshape(-1), tets)
    verts, _ = T.vertices(interp_v, tsdf, origin, voxel, dims)
    st = T.mesh_stats(verts, faces, (0, 0, 0))
    assert st["closed"]                                  # every edge in exactly two faces, once in each direction
    assert st["euler"] == 2                              # V - E + F of a sphere
    assert (st["out_sign"] > 0).all()                    # all face normals point outward
    assert abs(st["volume"] - 4 / 3 * np.pi * radius ** 3) < 0.02 * 4 / 3 * np.pi * radius ** 3
    assert np.abs(st["radius"] - radius).max() < 0.5 * voxel
    # float32 vertices: the same arithmetic rounded, within the three-operation bound of a coordinate below 1
    v32, _ = T.vertices(interp_v, tsdf, origin, voxel, dims, dtype=np.float32)
    assert np.abs(v32.astype(np.float64) - verts).max() < 8 * 2.0 ** -24


def test_gpu_cases_keep_the_fragile_cap():
    """For every GPU case the fragile voxels are at most 1 % of the observed ones, and outside them the float32 restatement already
    agrees with the float64 one on every count -- so E_ref is rounding error, not a flipped test."""
    c = T.integration_case()
    assert np.isnan(c["depth"]).any() and np.isinf(c["depth"]).any() and (c["depth"] == 0).any() and (c["depth"] < 0).any()
    for use_color, use_alpha in itertools.product((True, False), repeat=2):
        t = T.case_truth(c, use_color, use_alpha)
        print(f"integration case color={use_color} alpha={use_alpha}: observed {t['observed']} fragile share {t['share']:.4f} E_ref {t['e_ref']}")
        assert t["observed"] > 5000 and t["share"] <= T.FRAGILE_CAP
        keep = ~t["fragile"]
        assert np.array_equal(t["s32"]["weight"][keep], t["s64"]["weight"][keep])
        assert np.array_equal(t["s32"]["color_weight"][keep], t["s64"]["color_weight"][keep])
        assert t["e_ref"]["tsdf"] < 1e-4 and t["e_ref"]["color"] < 1e-4
        assert np.isfinite(t["s64"]["tsdf"]).all() and np.isfinite(t["s64"]["color"]).all()      # no dead pixel's NaN got in
    full = T.case_truth(c)
    # the special cameras: the inside camera leaves voxels behind z_near, the other two see nothing
    for v in (3, 4):
        alone = T.run_case(c, [v])
        assert not alone["weight"].any() and not alone["color_weight"].any()
    inside = T.run_case(c, [2])
    assert 0 < (inside["weight"] > 0).sum() < inside["weight"].size
    assert full["s64"]["weight"].max() == 3 and (full["s64"]["color_weight"] < full["s64"]["weight"]).any()
    # alpha matters, and so do depth edges: both spheres are seen
    assert not np.array_equal(T.case_truth(c, True, False)["s64"]["weight"], full["s64"]["weight"])


def test_e2e_case_restatement_mesh_is_closed():
    c = T.e2e_case()
    m = c["mesh"]
    st = T.mesh_stats(m["vertices"], m["faces"], (0, 0, 0))
    print(f"e2e: {m['n_active']} active cells, {len(m['faces'])} faces, volume {st['volume']:.5f} (sphere {4 / 3 * np.pi * 0.125:.5f})")
    assert c["fragile_share"] <= T.FRAGILE_CAP
    assert st["closed"] and st["euler"] == 2 and (st["out_sign"] > 0).all()
    assert np.abs(st["radius"] - 0.5).max() < float(c["voxel"])
    assert np.nanmin(m["vertex_colors"]) >= 0 and np.nanmax(m["vertex_colors"]) <= 1
