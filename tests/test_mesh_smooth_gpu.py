"""GPU tests of mesh smoothing and vertex normals: f3dg_mesh_adjacency / f3dg_mesh_smooth / f3dg_mesh_vertex_normals through ctypes,
mesh.mesh_adjacency / smooth_mesh / vertex_normals on top of them, and the TSDF route end to end. Truth and the shared cases are
tests/mesh_smooth_truth.py. nbr_start, nbr, boundary and the counts are compared for EXACT equality; smoothed vertices for exact equality of
their BIT PATTERNS after one step and after 10 Taubin iterations (the kernel and the restatement share the operation order, use IEEE
+ - * / only and round to float32 once per step); normals are equal or within one float32 ulp per component -- the slack covers only a
device sqrt / divide that differs from numpy's in the last float64 bit. Every figure is printed before it is asserted (``pytest -s``).

Shapes: one and two triangles, a tetrahedron, a mesh with degenerate faces and unused vertices; ids of N and -1; 63 / 64 / 65 / 257
independent triangles (wave and workgroup edges); closed fans of 16 / 17 / 2,048 / 2,049 rim vertices (the hub's row has 32 / 34 / 4,096 /
4,098 entries: both sides of the one-thread limit and of the LDS limit of the row sort); a 1025 x 1025 grid (1,050,625 vertices: the
single-workgroup scans of the per-vertex arrays run many rounds); an icosphere of 1,280 faces."""
import ctypes as C

import numpy as np
import pytest
import torch

from f3dgaus_amd import _lib, mesh, ply, synthetic
import mesh_smooth_truth as S

pytestmark = pytest.mark.gpu
SENT = -5
SENT_F = -123.25
_TRUTH = {}


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _truth(name, faces, N, P):
    """Computed once per case, shared, never modified."""
    if name not in _TRUTH:
        adj = S.adjacency(faces, N)
        _TRUTH[name] = {"adj": adj, "normals": S.normals(P, faces, N, adj)}
    return _TRUTH[name]


def _faces(faces, dev, dtype=torch.int64):
    return torch.from_numpy(np.ascontiguousarray(faces)).to(dev).to(dtype).reshape(-1, 3)


def _raw_adjacency(ft, N, ws=None):
    """f3dg_mesh_adjacency on outputs pre-filled with a sentinel: (rc, nbr_start, nbr [6 F], boundary, h_counts, workspace)."""
    L = _lib.lib()
    F, dev = ft.shape[0], ft.device
    nbytes = L.f3dg_mesh_adjacency_workspace_bytes(N, F)
    assert nbytes > 0 and (ws is None or ws.numel() >= nbytes)
    ws = torch.zeros(nbytes, dtype=torch.uint8, device=dev) if ws is None else ws
    nbytes = ws.numel()
    start = torch.full((N + 1,), SENT, dtype=torch.int32, device=dev)
    nbr = torch.full((6 * F,), SENT, dtype=torch.int32, device=dev)
    bnd = torch.full((N,), 77, dtype=torch.uint8, device=dev)
    h = (C.c_longlong * 4)(-7, -7, -7, -7)
    rc = L.f3dg_mesh_adjacency(_stream(), _lib.ptr(ws), nbytes, N, F, _lib.ptr(ft), int(ft.dtype == torch.int32), _lib.ptr(start), _lib.ptr(nbr),
                               _lib.ptr(bnd), h)
    torch.cuda.synchronize()
    return rc, start, nbr, bnd, list(h), ws


def _raw_smooth(start, nbr, pinned, vin, lam, mu, iterations):
    """f3dg_mesh_smooth on an output and a scratch pre-filled with a sentinel."""
    out, scratch = torch.full_like(vin, SENT_F), torch.full_like(vin, SENT_F)
    before = vin.clone()
    rc = _lib.lib().f3dg_mesh_smooth(_stream(), vin.shape[0], _lib.ptr(start), _lib.ptr(nbr), _lib.ptr(pinned), _lib.ptr(vin), lam, mu, iterations,
                                     _lib.ptr(scratch), _lib.ptr(out))
    torch.cuda.synchronize()
    assert rc == _lib.OK, rc
    assert torch.equal(vin, before)                                               # the input is never written
    return out


def _raw_normals(ws, ft, N, vt):
    out = torch.full((N, 3), SENT_F, dtype=torch.float32, device=vt.device)
    rc = _lib.lib().f3dg_mesh_vertex_normals(_stream(), _lib.ptr(ws), ws.numel(), N, ft.shape[0], _lib.ptr(ft), int(ft.dtype == torch.int32),
                                             _lib.ptr(vt), _lib.ptr(out))
    torch.cuda.synchronize()
    assert rc == _lib.OK, rc
    return out


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _ulp_apart(a, b):
    """Components that differ, and the largest difference in units of the last float32 place (ordered-integer distance)."""
    def key(x):
        i = _bits(x).astype(np.int64)
        return np.where(i < 0x80000000, i, 0x80000000 - i)
    d = np.abs(key(a) - key(b))
    d[(_bits(a) << 1 == 0) & (_bits(b) << 1 == 0)] = 0                               # +0 and -0
    return int(np.count_nonzero(d)), int(d.max()) if d.size else 0


def _check_case(name, faces, N, P, dev, dtype=torch.int64, pinned=None, iterations=10):
    """Adjacency exactly, one step and ``iterations`` Taubin iterations bit for bit (with ``pinned`` [N] uint8 or None, and with the
    boundary pinned through smooth_mesh), normals within one ulp. Returns the device outputs."""
    t = _truth(name, faces, N, P)
    adj = t["adj"]
    ft = _faces(faces, dev, dtype)
    rc, start, nbr, bnd, h, ws = _raw_adjacency(ft, N)
    two_e = adj["counts"][0]
    print(f"{name} ({dtype}): N {N} F {len(faces)}; rc {rc}; 2E {h[0]} boundary {h[1]} degenerate {h[2]} longest row {h[3]} (truth {adj['counts']})")
    assert rc == _lib.OK and h == adj["counts"]
    assert np.array_equal(start.cpu().numpy(), adj["nbr_start"])
    assert np.array_equal(nbr[:two_e].cpu().numpy(), adj["nbr"]) and bool((nbr[two_e:] == SENT).all())
    assert np.array_equal(bnd.cpu().numpy(), adj["boundary"])

    vt = torch.from_numpy(P).to(dev)
    pin_t = None if pinned is None else torch.from_numpy(pinned).to(dev)
    for label, lam, mu, it in (("1 step", 0.5, 0.0, 1), (f"{iterations} Taubin", 0.5, -0.53, iterations)):
        want = S.smooth(P, adj["nbr_start"], adj["nbr"], pinned, it, lam, mu)
        got = _raw_smooth(start, nbr, pin_t, vt, lam, mu, it).cpu().numpy()
        n_diff = int(np.count_nonzero(_bits(got) != _bits(want)))
        print(f"    smooth {label}: {n_diff} of {want.size} components differ in their bits; moved {int((_bits(want) != _bits(P)).any(axis=1).sum())} vertices")
        assert n_diff == 0
    got0 = _raw_smooth(start, nbr, pin_t, vt, 0.5, -0.53, 0).cpu().numpy()
    assert np.array_equal(_bits(got0), _bits(P))                                  # no iteration: the input

    got_n = _raw_normals(ws, ft, N, vt).cpu().numpy()
    n_diff, worst = _ulp_apart(got_n, t["normals"])
    print(f"    normals: {n_diff} of {got_n.size} components unequal, at most {worst} ulp apart")
    assert worst <= 1

    # the Python entries on top: the same numbers
    a = mesh.mesh_adjacency(ft, N)
    assert torch.equal(a["nbr_start"], start) and torch.equal(a["nbr"], nbr[:two_e]) and a["nbr"].shape[0] == two_e
    assert a["boundary"].dtype == torch.bool and np.array_equal(a["boundary"].cpu().numpy(), adj["boundary"].astype(bool))
    assert [2 * a["n_edges"], a["n_boundary_vertices"], a["n_degenerate"], a["max_row"]] == adj["counts"]
    sm = mesh.smooth_mesh(vt, ft, iterations=iterations, adjacency=a, pinned=pin_t)
    rim = adj["boundary"] if pinned is None else adj["boundary"] | (pinned != 0)
    want = S.smooth(P, adj["nbr_start"], adj["nbr"], rim, iterations)
    assert sm["adjacency"] is a and np.array_equal(_bits(sm["vertices"].cpu().numpy()), _bits(want))
    assert np.array_equal(_bits(sm["vertices"].cpu().numpy()[rim != 0]), _bits(P[rim != 0]))      # pinned: unchanged bit for bit
    assert torch.equal(mesh.vertex_normals(vt, ft, adjacency=a), torch.from_numpy(got_n).to(dev))
    assert torch.equal(mesh.vertex_normals(vt, ft), torch.from_numpy(got_n).to(dev))
    return {"start": start, "nbr": nbr, "boundary": bnd, "normals": got_n, "h": h, "ws": ws, "faces": ft, "vertices": vt}


@pytest.mark.parametrize("name", ["one triangle", "two on an edge", "tetrahedron", "oddities"])
def test_the_smallest_meshes(gpu_device, name):
    faces, N = S.small_cases()[name]
    P = S.rand_vertices(N, seed=5)
    pinned = np.zeros(N, np.uint8)
    pinned[0] = 1
    for pin in (None, pinned):
        r = _check_case(name, faces, N, P, gpu_device, pinned=pin)
    if name == "one triangle":
        assert r["boundary"].tolist() == [1, 1, 1] and r["h"] == [6, 3, 0, 2]
    if name == "two on an edge":
        assert r["h"][0] == 10 and r["boundary"].tolist() == [1, 1, 1, 1]         # the shared edge is no boundary edge; its ends have others
        assert np.diff(r["start"].cpu().numpy()).tolist() == [2, 3, 3, 2]         # duplicates of the shared edge's ends are merged
    if name == "tetrahedron":
        assert r["h"] == [12, 0, 0, 6] and not r["boundary"].any()
    if name == "oddities":
        assert r["h"][2] == 2 and not r["normals"][5].any() and not r["normals"][7].any()
        out = _raw_smooth(r["start"], r["nbr"], None, r["vertices"], 0.5, -0.53, 10).cpu().numpy()
        assert np.array_equal(_bits(out[[5, 7]]), _bits(P[[5, 7]]))               # no neighbour: copied through


def test_one_triangle_pinned_and_free(gpu_device):
    faces, N = S.small_cases()["one triangle"]
    P = S.rand_vertices(N, seed=6)
    ft, vt = _faces(faces, gpu_device), torch.from_numpy(P).to(gpu_device)
    pinned = mesh.smooth_mesh(vt, ft)["vertices"]                                 # all boundary, pin_boundary by default
    free = mesh.smooth_mesh(vt, ft, pin_boundary=False)["vertices"].cpu().numpy()
    adj = S.adjacency(faces, N)
    want = S.smooth(P, adj["nbr_start"], adj["nbr"], None, 10)
    print(f"one triangle: pinned equal {torch.equal(pinned, vt)}, free differs from the input in {int((_bits(free) != _bits(P)).sum())} components")
    assert np.array_equal(_bits(pinned.cpu().numpy()), _bits(P)) and np.array_equal(_bits(free), _bits(want)) and (free != P).any()
    lap = mesh.smooth_mesh(vt, ft, iterations=3, lam=1.0, mu=0.0, pin_boundary=False)["vertices"].cpu().numpy()
    assert np.array_equal(_bits(lap), _bits(S.smooth(P, adj["nbr_start"], adj["nbr"], None, 3, 1.0, 0.0)))
    with pytest.raises(ValueError):
        mesh.smooth_mesh(vt, ft, lam=0.5, mu=-0.4)


@pytest.mark.parametrize("dtype", [torch.int64, torch.int32])
@pytest.mark.parametrize("bad", ["N", "-1"])
def test_an_id_out_of_range_refuses_the_mesh_and_writes_nothing(gpu_device, dtype, bad):
    faces, N, _ = S.grid(20, 20)
    faces = faces.copy()
    faces[len(faces) // 2, 1] = N if bad == "N" else -1
    ft = _faces(faces, gpu_device, dtype)
    rc, start, nbr, bnd, h, ws = _raw_adjacency(ft, N)
    print(f"id {bad} ({dtype}): rc {rc}, h_counts {h}")
    assert rc == _lib.ERR_BAD_ARG and h == [-7] * 4
    assert bool((start == SENT).all()) and bool((nbr == SENT).all()) and bool((bnd == 77).all())
    vt = torch.rand(N, 3, device=gpu_device)
    assert bool((_raw_normals(ws, ft, N, vt) == SENT_F).all())                    # no completed build on the workspace: nothing written
    with pytest.raises(_lib.F3dgError):
        mesh.mesh_adjacency(ft, N)


def test_normals_need_a_completed_build_of_the_same_sizes(gpu_device):
    dev = gpu_device
    faces, N, P = S.grid(6, 5)
    ft, vt = _faces(faces, dev), torch.from_numpy(P).to(dev)
    L = _lib.lib()
    other, N2 = S.strip(len(faces))                                               # as many faces over other vertices
    assert N2 != N
    big = torch.zeros(max(L.f3dg_mesh_adjacency_workspace_bytes(n, len(faces)) for n in (N, N2)), dtype=torch.uint8, device=dev)
    assert bool((_raw_normals(big, ft, N, vt) == SENT_F).all())                   # a zeroed workspace
    rc, *_ = _raw_adjacency(_faces(other, dev), N2, ws=big)
    assert rc == _lib.OK
    assert bool((_raw_normals(big, ft, N, vt) == SENT_F).all())                   # the workspace of another mesh's build
    rc, *_ = _raw_adjacency(ft, N, ws=big)
    assert rc == _lib.OK
    n_diff, worst = _ulp_apart(_raw_normals(big, ft, N, vt).cpu().numpy(), S.normals(P, faces, N))
    print(f"grid 6x5 normals after a build: {n_diff} components unequal, at most {worst} ulp")
    assert worst <= 1


@pytest.mark.parametrize("n", [63, 64, 65, 257])
def test_independent_triangles_at_the_wave_and_workgroup_edges(gpu_device, n):
    faces, N = S.independent(n)
    r = _check_case(f"{n} independent", faces, N, S.rand_vertices(N, seed=n), gpu_device)
    assert r["h"] == [6 * n, 3 * n, 0, 2]


@pytest.mark.parametrize("n", [16, 17, 2048, 2049])
def test_closed_fans_on_both_sides_of_the_row_sort_limits(gpu_device, n):
    faces, N = S.closed_fan(n)
    rng = np.random.default_rng(n)
    faces = faces[rng.permutation(n)]                                             # the hub's entries arrive in no particular order
    r = _check_case(f"fan {n}", faces, N, S.fan_vertices(n, seed=n), gpu_device)
    assert r["h"] == [4 * n, n, 0, 2 * n] and r["boundary"].tolist() == [0] + [1] * n
    free = _raw_smooth(r["start"], r["nbr"], None, r["vertices"], 0.5, 0.0, 1).cpu().numpy()
    adj = _TRUTH[f"fan {n}"]["adj"]
    assert np.array_equal(_bits(free), _bits(S.smooth(S.fan_vertices(n, seed=n), adj["nbr_start"], adj["nbr"], None, 1, 0.5, 0.0)))


def test_a_grid_of_more_than_2_pow_20_vertices(gpu_device):
    """1025 x 1025: adjacency, one step and the normals (the truth is vectorised: seconds)."""
    dev = gpu_device
    faces, N, P = S.grid(1025, 1025)
    assert N == 1_050_625 > 1 << 20
    adj = S.adjacency(faces, N)
    ft, vt = _faces(faces, dev, torch.int32), torch.from_numpy(P).to(dev)
    rc, start, nbr, bnd, h, ws = _raw_adjacency(ft, N)
    two_e = adj["counts"][0]
    print(f"grid 1025^2: N {N} F {len(faces)}; rc {rc}; counts {h} (truth {adj['counts']})")
    assert rc == _lib.OK and h == adj["counts"] and h[1] == 4 * 1024
    assert np.array_equal(start.cpu().numpy(), adj["nbr_start"]) and np.array_equal(nbr[:two_e].cpu().numpy(), adj["nbr"])
    assert np.array_equal(bnd.cpu().numpy().astype(bool), S.grid_rim(1025, 1025))
    pin = torch.from_numpy(adj["boundary"]).to(dev)
    got = _raw_smooth(start, nbr, pin, vt, 0.5, 0.0, 1).cpu().numpy()
    want = S.smooth(P, adj["nbr_start"], adj["nbr"], adj["boundary"], 1, 0.5, 0.0)
    n_diff = int(np.count_nonzero(_bits(got) != _bits(want)))
    print(f"    one step: {n_diff} of {want.size} components differ in their bits")
    assert n_diff == 0
    n_diff, worst = _ulp_apart(_raw_normals(ws, ft, N, vt).cpu().numpy(), S.normals(P, faces, N, adj))
    print(f"    normals: {n_diff} of {3 * N} components unequal, at most {worst} ulp apart")
    assert worst <= 1


def test_icosphere_int32_int64_repeat_runs_and_outward_normals(gpu_device):
    dev = gpu_device
    P, faces = S.icosphere(3, noise=0.02, seed=4)
    assert len(faces) == 1280
    N = len(P)
    r64 = _check_case("icosphere 1280", faces, N, P, dev, torch.int64)
    r32 = _check_case("icosphere 1280", faces, N, P, dev, torch.int32)
    vt = r64["vertices"]
    runs = []
    for ft in (r64["faces"], r32["faces"], r64["faces"]):
        a = mesh.mesh_adjacency(ft, N)
        sm = mesh.smooth_mesh(vt, ft, adjacency=a)["vertices"]
        runs.append((a["nbr_start"], a["nbr"], a["boundary"], sm, mesh.vertex_normals(sm, ft, adjacency=a)))
    for r in runs[1:]:
        assert all(torch.equal(x, y) for x, y in zip(runs[0], r))                 # int32 = int64 = a second run, byte for byte
    assert r64["h"] == r32["h"] == [2 * 1920, 0, 0, 12] and N - 1920 + 1280 == 2
    dots = (r64["normals"].astype(np.float64) * P).sum(1)
    r0, d0 = S.radial_stats(P)
    r1, d1 = S.radial_stats(runs[0][3].cpu().numpy())
    print(f"icosphere: least normal . direction {dots.min():.4f}; radius {r0:.5f} rms {d0:.5f} -> {r1:.5f} rms {d1:.5f} after 10 Taubin iterations")
    assert (dots > 0).all() and d1 < d0
    smooth_n = runs[0][4].cpu().numpy().astype(np.float64)
    assert ((smooth_n * runs[0][3].cpu().numpy()).sum(1) > 0).all()


# ------------------------------------------------------------------------------------------------ the purpose, end to end
def test_extract_mesh_tsdf_smooths_and_writes_normals(f3d, gpu_device, tmp_path):
    """The synthetic blob of the TSDF suite (4,096 opaque Gaussians in a ball of radius 0.4, 8 orbit cameras of 64^2) fused into a 32^3
    volume."""
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
    bg = torch.zeros(3, device=dev)
    args = (pc, 0, cams["viewmatrix"], cams["projmatrix"], cams["campos"], bg, cams["cfg"])
    plain = mesh.extract_mesh_tsdf(*args, resolution=32)
    none = mesh.extract_mesh_tsdf(*args, resolution=32, smooth_iterations=None, smooth_lambda=0.5, smooth_mu=-0.53, vertex_normals=False)
    assert sorted(plain) == sorted(none) == ["faces", "interp_v", "tets", "vertex_colors", "vertices"]
    assert all(torch.equal(plain[k], none[k]) for k in plain)                     # the defaults: today's dict, key for key
    m = mesh.extract_mesh_tsdf(*args, resolution=32, smooth_iterations=5, vertex_normals=True)
    assert sorted(m) == sorted(list(plain) + ["vertex_normals"])
    assert all(torch.equal(plain[k], m[k]) for k in ("faces", "interp_v", "tets", "vertex_colors"))
    want = mesh.smooth_mesh(plain["vertices"], plain["faces"], iterations=5)
    moved = int((m["vertices"] != plain["vertices"]).any(dim=1).sum())
    print(f"blob at 32^3: {plain['vertices'].shape[0]} vertices, {plain['faces'].shape[0]} faces, {want['adjacency']['n_boundary_vertices']} on the "
          f"boundary; 5 Taubin iterations moved {moved}")
    assert plain["faces"].shape[0] > 0 and moved > 0
    assert torch.equal(m["vertices"], want["vertices"])
    assert torch.equal(m["vertex_normals"], mesh.vertex_normals(want["vertices"], plain["faces"]))
    length = m["vertex_normals"].double().norm(dim=1)
    assert bool(((length - 1).abs() < 1e-6).logical_or(length == 0).all()) and bool((length > 0).any())
    only_n = mesh.extract_mesh_tsdf(*args, resolution=32, vertex_normals=True)
    assert torch.equal(only_n["vertices"], plain["vertices"]) and torch.equal(only_n["vertex_normals"], mesh.vertex_normals(plain["vertices"], plain["faces"]))
    rgb8 = (m["vertex_colors"].clamp(0, 1) * 255).round().to(torch.uint8)
    path = str(tmp_path / "smooth.ply")
    ply.save_mesh_ply(path, m["vertices"], m["faces"], rgb8, vertex_normals=m["vertex_normals"])
    rv, rf, rc, rn = ply.read_mesh_ply(path, with_normals=True)
    assert np.array_equal(rv, m["vertices"].cpu().numpy()) and np.array_equal(rf, m["faces"].cpu().numpy())
    assert np.array_equal(rc, rgb8.cpu().numpy()) and np.array_equal(_bits(rn), _bits(m["vertex_normals"].cpu().numpy()))
    assert len(ply.read_mesh_ply(path)) == 3


def test_extract_mesh_keywords(f3d, gpu_device):
    """The tetrahedral route (the scene of its own suite, rebuilt here: 300 opaque Gaussians in a ball under 3 cameras of 64^2, a 9^3 Kuhn
    grid): without the keywords the dict is the earlier one; with them its keys are untouched and the smoothed vertices and the normals of
    the last mesh are added."""
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
    assert sorted(plain) == ["faces", "faces_filtered", "keep", "vertices", "vertices_filtered"] and plain["faces_filtered"].shape[0] > 0
    got = mesh.extract_mesh(*args, smooth_iterations=3, vertex_normals=True)
    assert sorted(got) == sorted(list(plain) + ["vertices_smooth", "vertex_normals"]) and all(torch.equal(plain[k], got[k]) for k in plain)
    want = mesh.smooth_mesh(plain["vertices_filtered"], plain["faces_filtered"], iterations=3)
    print(f"tetrahedral route: {plain['vertices_filtered'].shape[0]} filtered vertices, {plain['faces_filtered'].shape[0]} faces, "
          f"{want['adjacency']['n_boundary_vertices']} on the boundary; 3 iterations moved {int((want['vertices'] != plain['vertices_filtered']).any(dim=1).sum())}")
    assert torch.equal(got["vertices_smooth"], want["vertices"])
    assert torch.equal(got["vertex_normals"], mesh.vertex_normals(want["vertices"], plain["faces_filtered"]))
    both = mesh.extract_mesh(*args, keep_largest=1, smooth_iterations=3, smooth_mu=0.0, vertex_normals=True)
    lap = mesh.smooth_mesh(both["vertices_clean"], both["faces_clean"], iterations=3, mu=0.0)
    assert torch.equal(both["vertices_smooth"], lap["vertices"]) and both["vertex_normals"].shape == both["vertices_clean"].shape
    only_n = mesh.extract_mesh(*args, vertex_normals=True)
    assert "vertices_smooth" not in only_n and torch.equal(only_n["vertex_normals"], mesh.vertex_normals(plain["vertices_filtered"], plain["faces_filtered"]))
