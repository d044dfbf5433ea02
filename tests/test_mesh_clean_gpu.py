"""GPU tests of the mesh clean-up: f3dg_mesh_components and f3dg_mesh_compact_count / _emit through ctypes, mesh.mesh_components and
mesh.clean_mesh on top of them, and the purpose end to end (a floater removed from a TSDF mesh). Truth and the shared cases are
tests/mesh_clean_truth.py. Labels, sizes, counts, faces and vertex ids are integers and compared for EXACT equality: there is no tolerance
anywhere. Every figure is printed before it is asserted (``pytest -s``).

Shapes: one, two and three faces; 63 / 64 / 65 / 257 independent triangles (the wave and workgroup edges of the ballot aggregation and the
scans); a 4,099-face strip (17 workgroups, one dependency chain across all of them) in three vertex orders; the strip among 1,000
triangles (1,001 components, 20 workgroups); 1,048,833 independent triangles for the compaction alone (the smallest that enters the second
round of its single-workgroup count scan, at workgroup 4,097); 48^3 and 32^3 volumes for the routes."""
import ctypes as C

import numpy as np
import pytest
import torch

from f3dgaus_amd import _lib, mesh, ply, synthetic, tsdf
import mesh_clean_truth as M
import tsdf_truth as T

pytestmark = pytest.mark.gpu
SENT = -5
MAX_ROUNDS = 32
_TRUTH = {}


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _truth(name, faces, N):
    """Computed once per case, shared, never modified."""
    if name not in _TRUTH:
        labels, sizes, n_deg = M.components(faces, N)
        roots, ranked = M.ranking(sizes)
        _TRUTH[name] = {"labels": labels, "sizes": sizes, "n_deg": n_deg, "roots": roots, "ranked": ranked, "dense": M.dense(labels, roots)}
    return _TRUTH[name]


def _dev(faces, dev, dtype=torch.int64):
    return torch.from_numpy(np.ascontiguousarray(faces)).to(dev).to(dtype).reshape(-1, 3)


def _raw_components(faces_t, N):
    """f3dg_mesh_components on outputs pre-filled with a sentinel: (rc, face_component, component_faces, h_counts)."""
    L = _lib.lib()
    F, dev = faces_t.shape[0], faces_t.device
    nbytes = L.f3dg_mesh_components_workspace_bytes(N, F)
    assert nbytes > 0
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    fc = torch.full((F,), SENT, dtype=torch.int32, device=dev)
    cf = torch.full((N,), SENT, dtype=torch.int32, device=dev)
    h = (C.c_longlong * 4)(-7, -7, -7, -7)
    rc = L.f3dg_mesh_components(_stream(), _lib.ptr(ws), nbytes, N, F, _lib.ptr(faces_t), int(faces_t.dtype == torch.int32), _lib.ptr(fc), _lib.ptr(cf), h)
    torch.cuda.synchronize()
    return rc, fc, cf, list(h)


def _attributes(N, dev):
    v = torch.arange(3 * N, dtype=torch.float32, device=dev).reshape(N, 3)
    return v, (v * 0.5 + 1.0).contiguous()


def _check_case(name, faces, N, dev, dtype=torch.int64, criteria=({}, {"keep_largest": 1})):
    """The C ABI's labels, sizes and counts, mesh_components' ranking and clean_mesh under ``criteria`` against the truth, exactly."""
    t = _truth(name, faces, N)
    ft = _dev(faces, dev, dtype)
    rc, fc, cf, h = _raw_components(ft, N)
    n_comp, largest = int(np.count_nonzero(t["sizes"])), int(t["sizes"].max()) if len(faces) else 0
    print(f"{name} ({dtype}): N {N} F {len(faces)}; components {h[0]} (truth {n_comp}) largest {h[1]} (truth {largest}) degenerate {h[2]} "
          f"(truth {t['n_deg']}) rounds {h[3]} (cap {MAX_ROUNDS})")
    assert rc == _lib.OK, rc
    assert np.array_equal(fc.cpu().numpy(), t["labels"]) and np.array_equal(cf.cpu().numpy(), t["sizes"])
    assert h[:3] == [n_comp, largest, t["n_deg"]]
    assert (1 <= h[3] <= MAX_ROUNDS) if len(faces) else h[3] == 0
    mc = mesh.mesh_components(ft, N)
    assert mc["face_component"].dtype == torch.int64 and np.array_equal(mc["face_component"].cpu().numpy(), t["dense"])
    assert np.array_equal(mc["component_sizes"].cpu().numpy(), t["ranked"]) and np.array_equal(mc["component_roots"].cpu().numpy(), t["roots"])
    assert mc["n_degenerate"] == t["n_deg"] and mc["rounds"] == h[3]
    v, col = _attributes(N, dev)
    outs = []
    for kw in criteria:
        want = M.clean(faces, N, **kw)
        got = mesh.clean_mesh(v, ft, col, **kw)
        print(f"    clean_mesh({kw}): {got['faces'].shape[0]} faces (truth {len(want['faces'])}), {got['vertex_ids'].shape[0]} vertices "
              f"(truth {len(want['vertex_ids'])}), {got['component_sizes'].shape[0]} components")
        for k in ("faces", "vertex_ids", "face_component", "component_sizes"):
            assert got[k].dtype == torch.int64 and np.array_equal(got[k].cpu().numpy(), want[k]), (name, kw, k)
        assert got["faces"].shape[1:] == (3,)
        assert torch.equal(got["vertices"], v[got["vertex_ids"]]) and torch.equal(got["vertex_colors"], col[got["vertex_ids"]])
        outs.append(got)
    return h, fc, cf, outs


@pytest.mark.parametrize("name", ["one triangle", "two sharing a vertex", "two disjoint"])
def test_the_smallest_meshes(gpu_device, name):
    faces, N = M.small_cases()[name]
    h, _, _, _ = _check_case(name, faces, N, gpu_device)
    assert h[0] == {"one triangle": 1, "two sharing a vertex": 1, "two disjoint": 2}[name]


@pytest.mark.parametrize("n", [63, 64, 65, 257])
def test_independent_triangles_at_the_wave_and_workgroup_edges(gpu_device, n):
    faces, N = M.independent(n)
    h, _, cf, _ = _check_case(f"{n} independent", faces, N, gpu_device)
    assert h[0] == n and h[1] == 1 and int(cf.sum()) == n


@pytest.mark.parametrize("order", ["ascending", "descending", "random"])
def test_a_strip_is_one_component_whatever_the_vertex_order(gpu_device, order):
    faces, N = M.strip(M.STRIP, order, seed=3)
    h, fc, cf, _ = _check_case(f"strip {order}", faces, N, gpu_device)
    assert h[:3] == [1, M.STRIP, 0] and bool((fc == 0).all()) and int(cf[0]) == M.STRIP
    assert 1 <= h[3] <= MAX_ROUNDS


def test_a_strip_among_a_thousand_triangles(gpu_device):
    faces, N = M.mixed()
    kept_strip = ({"keep_largest": 1}, {"min_faces": 2}, {"min_fraction": 0.5}, {"min_faces": 2, "keep_largest": 3, "min_fraction": 0.01})
    h, _, _, outs = _check_case("mixed", faces, N, gpu_device, criteria=({},) + kept_strip + ({"keep_largest": 0}, {"keep_largest": 7}))
    assert h[0] == 1001 and h[1] == M.STRIP
    for got in outs[1:5]:                                   # all keep exactly the strip
        assert got["faces"].shape[0] == M.STRIP and got["vertex_ids"].shape[0] == M.STRIP + 2 and got["component_sizes"].tolist() == [M.STRIP]
        assert int(got["vertex_ids"].min()) >= 3000 and torch.equal(got["faces"], outs[1]["faces"])
    assert outs[5]["faces"].shape == (0, 3) and outs[5]["vertex_ids"].shape == (0,) and outs[5]["vertices"].shape == (0, 3)
    assert outs[6]["component_sizes"].tolist() == [M.STRIP] + [1] * 6


def test_duplicates_degenerates_unreferenced_vertices_and_both_index_types(gpu_device):
    faces, N = M.oddities()
    h64, fc64, cf64, o64 = _check_case("oddities", faces, N, gpu_device, torch.int64, criteria=({}, {"keep_largest": 2}, {"min_faces": 3}))
    h32, fc32, cf32, o32 = _check_case("oddities", faces, N, gpu_device, torch.int32, criteria=({}, {"keep_largest": 2}, {"min_faces": 3}))
    assert h64 == h32 and torch.equal(fc64, fc32) and torch.equal(cf64, cf32)
    for a, b in zip(o64, o32):
        assert all(torch.equal(a[k], b[k]) for k in ("faces", "vertex_ids", "face_component", "component_sizes", "vertices"))
    assert h64[:3] == [3, 3, 5]
    assert o64[0]["faces"].shape[0] == 7 and o64[0]["vertex_ids"].tolist() == [1, 2, 3, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18]
    # no faces at all: every count 0, every element of component_faces written
    for dtype in (torch.int64, torch.int32):
        _, _, cf, outs = _check_case("empty", np.zeros((0, 3), np.int64), 4, gpu_device, dtype)
        assert cf.tolist() == [0, 0, 0, 0] and outs[0]["faces"].shape == (0, 3) and outs[0]["vertices"].shape == (0, 3)


@pytest.mark.parametrize("bad_id", ["N", "-1"])
@pytest.mark.parametrize("dtype", [torch.int64, torch.int32])
def test_an_id_out_of_range_is_refused_and_nothing_is_written(gpu_device, bad_id, dtype):
    """The range check comes before anything is indexed: the call returns F3DG_ERR_BAD_ARG and the sentinel-filled outputs are untouched."""
    dev = gpu_device
    faces, N = M.strip(300, "random", seed=5)
    faces = faces.copy()
    faces[177, 1] = N if bad_id == "N" else -1
    ft = _dev(faces, dev, dtype)
    rc, fc, cf, h = _raw_components(ft, N)
    print(f"id {bad_id} ({dtype}): rc {rc}")
    assert rc == _lib.ERR_BAD_ARG
    assert bool((fc == SENT).all()) and bool((cf == SENT).all()) and h == [-7] * 4
    with pytest.raises(_lib.F3dgError):
        mesh.mesh_components(ft, N)
    # the compaction's own check: labels that keep the bad face
    L = _lib.lib()
    nbytes = L.f3dg_mesh_compact_workspace_bytes(N, 300)
    ws = torch.zeros(nbytes, dtype=torch.uint8, device=dev)
    labels, keep = torch.zeros(300, dtype=torch.int32, device=dev), torch.ones(N, dtype=torch.uint8, device=dev)
    hc = (C.c_longlong * 2)(-7, -7)
    rc = L.f3dg_mesh_compact_count(_stream(), _lib.ptr(ws), nbytes, N, 300, _lib.ptr(ft), int(dtype == torch.int32), _lib.ptr(labels), _lib.ptr(keep), hc)
    assert rc == _lib.ERR_BAD_ARG and list(hc) == [-7, -7]
    out, ids = torch.full((300, 3), SENT, dtype=torch.int64, device=dev), torch.full((N,), SENT, dtype=torch.int64, device=dev)
    assert L.f3dg_mesh_compact_emit(_stream(), _lib.ptr(ws), nbytes, N, 300, _lib.ptr(ft), int(dtype == torch.int32), _lib.ptr(labels), _lib.ptr(keep),
                                    300, N, _lib.ptr(out), _lib.ptr(ids)) == _lib.OK
    torch.cuda.synchronize()
    assert bool((out == SENT).all()) and bool((ids == SENT).all())          # a refused count leaves nothing to emit from


def test_emit_on_a_workspace_without_a_count_writes_nothing(gpu_device):
    """f3dg_mesh_compact_emit on a zeroed workspace, and on the workspace of another mesh's count, leaves its outputs alone; a capacity
    below the counts writes the first rows only."""
    dev = gpu_device
    L = _lib.lib()
    faces, N = M.mixed()
    F = len(faces)
    ft = _dev(faces, dev)
    rc, fc, _, _ = _raw_components(ft, N)
    assert rc == _lib.OK
    keep = torch.ones(N, dtype=torch.uint8, device=dev)
    nbytes = L.f3dg_mesh_compact_workspace_bytes(N, F)
    other, N2 = M.strip(F, "ascending")                     # as many faces, other vertices
    big = torch.zeros(max(nbytes, L.f3dg_mesh_compact_workspace_bytes(N2, F)), dtype=torch.uint8, device=dev)
    out, ids = torch.full((F, 3), SENT, dtype=torch.int64, device=dev), torch.full((N,), SENT, dtype=torch.int64, device=dev)
    emit = lambda ws, nf, nv: L.f3dg_mesh_compact_emit(_stream(), _lib.ptr(ws), ws.numel(), N, F, _lib.ptr(ft), 0, _lib.ptr(fc), _lib.ptr(keep), nf, nv,
                                                       _lib.ptr(out), _lib.ptr(ids))
    assert emit(big, F, N) == _lib.OK
    torch.cuda.synchronize()
    assert bool((out == SENT).all()) and bool((ids == SENT).all())
    ot = _dev(other, dev)
    rc2, fc2, _, _ = _raw_components(ot, N2)
    hc = (C.c_longlong * 2)()
    assert rc2 == _lib.OK and L.f3dg_mesh_compact_count(_stream(), _lib.ptr(big), big.numel(), N2, F, _lib.ptr(ot), 0, _lib.ptr(fc2),
                                                        _lib.ptr(torch.ones(N2, dtype=torch.uint8, device=dev)), hc) == _lib.OK
    assert list(hc) == [F, N2]
    assert emit(big, F, N) == _lib.OK                       # counted on N2 vertices, asked for N
    torch.cuda.synchronize()
    assert bool((out == SENT).all()) and bool((ids == SENT).all())
    # the real count, then a capacity below it
    assert L.f3dg_mesh_compact_count(_stream(), _lib.ptr(big), big.numel(), N, F, _lib.ptr(ft), 0, _lib.ptr(fc), _lib.ptr(keep), hc) == _lib.OK
    assert list(hc) == [F, N]
    assert emit(big, F - 3, N - 2) == _lib.OK
    torch.cuda.synchronize()
    want = M.clean(faces, N)
    assert np.array_equal(out[:F - 3].cpu().numpy(), want["faces"][:F - 3]) and bool((out[F - 3:] == SENT).all())
    assert np.array_equal(ids[:N - 2].cpu().numpy(), want["vertex_ids"][:N - 2]) and bool((ids[N - 2:] == SENT).all())


def _second_round_case():
    """4096 * 256 + 257 independent triangles: 4,098 workgroups of faces and 12,292 of vertices, so the single-workgroup scan of the
    counts (4,096 per round) takes two rounds over the faces and four over the vertices. Computed once, shared, never modified."""
    if "second round" not in _TRUTH:
        n = 4096 * 256 + 257
        faces, N = M.independent(n)
        f = np.arange(n, dtype=np.int64)
        kept = (f * 2654435761) % 7 < 3
        kept[[0, 4096 * 256 - 1, 4096 * 256, n - 1]] = True               # the faces on either side of the round's edge, and both ends
        labels = 3 * f                                                      # each triangle's least vertex id
        keep_root = np.zeros(N, dtype=np.uint8)
        keep_root[labels[kept]] = 1
        faces_out, vertex_ids, kept_truth = M.compact(faces, N, labels, keep_root)
        assert np.array_equal(kept_truth, kept)
        _TRUTH["second round"] = (faces, N, labels.astype(np.int32), keep_root, faces_out, vertex_ids)
    return _TRUTH["second round"]


@pytest.mark.parametrize("dtype", [torch.int64, torch.int32])
def test_compaction_past_the_first_round_of_the_count_scan(gpu_device, dtype):
    """Kept faces and used vertices beyond workgroup 4,096 (element 1,048,577): the carry of the count scan, the length of its padding
    and the word index of the rank are exercised only from there."""
    dev = gpu_device
    L = _lib.lib()
    faces, N, labels, keep_root, faces_out, vertex_ids = _second_round_case()
    F = len(faces)
    assert F == 1_048_833 and N == 3_146_499 and (F + 255) // 256 > 4096 and (N + 255) // 256 == 12_292
    ft = _dev(faces, dev, dtype)
    fc, keep = torch.from_numpy(labels).to(dev), torch.from_numpy(keep_root).to(dev)
    nbytes = L.f3dg_mesh_compact_workspace_bytes(N, F)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    hc = (C.c_longlong * 2)(-7, -7)
    rc = L.f3dg_mesh_compact_count(_stream(), _lib.ptr(ws), nbytes, N, F, _lib.ptr(ft), int(dtype == torch.int32), _lib.ptr(fc), _lib.ptr(keep), hc)
    print(f"second round ({dtype}): rc {rc}, kept {list(hc)} (truth {[len(faces_out), len(vertex_ids)]})")
    assert rc == _lib.OK
    assert list(hc) == [len(faces_out), len(vertex_ids)] == [449_502, 1_348_506]
    out = torch.full((hc[0], 3), SENT, dtype=torch.int64, device=dev)
    ids = torch.full((hc[1],), SENT, dtype=torch.int64, device=dev)
    assert L.f3dg_mesh_compact_emit(_stream(), _lib.ptr(ws), nbytes, N, F, _lib.ptr(ft), int(dtype == torch.int32), _lib.ptr(fc), _lib.ptr(keep),
                                    hc[0], hc[1], _lib.ptr(out), _lib.ptr(ids)) == _lib.OK
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), faces_out)
    assert np.array_equal(ids.cpu().numpy(), vertex_ids)


def test_bitwise_repeatable(gpu_device):
    dev = gpu_device
    faces, N = M.mixed()
    ft = _dev(faces, dev)
    v, col = _attributes(N, dev)
    runs = []
    for _ in range(5):
        rc, fc, cf, h = _raw_components(ft, N)
        assert rc == _lib.OK
        mc = mesh.mesh_components(ft, N)
        cm = mesh.clean_mesh(v, ft, col, min_faces=1, keep_largest=500)
        runs.append([fc, cf, torch.tensor(h[:3])] + [mc[k] for k in ("face_component", "component_sizes", "component_roots")]
                    + [cm[k] for k in ("vertices", "faces", "vertex_colors", "vertex_ids", "face_component", "component_sizes")])
    for r in runs[1:]:
        assert all(torch.equal(a, b) for a, b in zip(runs[0], r))


# ------------------------------------------------------------------------------------------------ the purpose, end to end
BODY, FLOATER = ((-6.0, 0.5, -0.25), 14.0), ((18.0, 1.0, 0.5), 3.0)        # centres and radii in voxels about the volume's centre


def test_a_floater_is_removed_from_a_tsdf_mesh(gpu_device, tmp_path):
    """A 48^3 volume holding the minimum of two analytic sphere distances (built as tsdf_truth.analytic_sphere_volume builds one): a body of
    radius 14 voxels and a floater of radius 3 voxels whose surface is 7 voxels from the body's."""
    dev = gpu_device
    dims, voxel = (48, 48, 48), 0.03
    trunc = 4 * voxel
    origin, _, weight = T.analytic_sphere_volume(dims, voxel, 1.0, trunc)
    p = T.voxel_centres(origin, voxel, dims, np.float64)
    centre = lambda c: np.asarray(c) * voxel
    t = np.minimum(*[np.clip((np.linalg.norm(p - centre(c), axis=1) - r * voxel) / trunc, -1, 1) for c, r in (BODY, FLOATER)])
    assert np.linalg.norm(centre(BODY[0]) - centre(FLOATER[0])) / voxel - BODY[1] - FLOATER[1] >= 6.0
    vol = tsdf.TSDFVolume(origin, voxel, dims, device=dev)
    vol.tsdf.copy_(torch.from_numpy(t.astype(np.float32).reshape(48, 48, 48)))
    vol.weight.copy_(torch.from_numpy(weight))
    vol.color.copy_(torch.from_numpy(np.random.default_rng(1).random((3, 48, 48, 48)).astype(np.float32)))
    vol.color_weight.fill_(1.0)
    m = vol.extract()
    n_v, n_f = m["vertices"].shape[0], m["faces"].shape[0]
    mc = mesh.mesh_components(m["faces"], n_v)
    sizes = mc["component_sizes"].tolist()
    print(f"two spheres: {n_v} vertices, {n_f} faces, components {sizes}, rounds {mc['rounds']}")
    assert len(sizes) == 2 and sizes[0] > sizes[1] > 0 and mc["n_degenerate"] == 0 and sum(sizes) == n_f
    threshold = (sizes[0] + sizes[1]) // 2
    c = mesh.clean_mesh(m["vertices"], m["faces"], m["vertex_colors"], min_faces=threshold)
    v, f = c["vertices"].cpu().numpy(), c["faces"].cpu().numpy()
    st = T.mesh_stats(v, f, centre(BODY[0]))
    print(f"cleaned with min_faces={threshold}: {len(v)} vertices, {len(f)} faces, closed {st['closed']}, euler {st['euler']}, "
          f"radii {st['radius'].min() / voxel:.3f} .. {st['radius'].max() / voxel:.3f} voxels")
    assert len(f) == sizes[0] and c["component_sizes"].tolist() == [sizes[0]] and bool((c["face_component"] == 0).all())
    assert st["closed"] and st["euler"] == 2 and bool((st["out_sign"] > 0).all())
    assert abs(st["radius"] - BODY[1] * voxel).max() <= voxel              # the body, not the floater
    whole = T.mesh_stats(m["vertices"].cpu().numpy(), m["faces"].cpu().numpy(), centre(BODY[0]))
    assert whole["closed"] and whole["euler"] == 4                         # two spheres before
    # the kept faces are the body's faces of the uncleaned mesh, in their order, under vertex_ids
    assert torch.equal(c["vertex_ids"][c["faces"]], m["faces"][mc["face_component"] == 0])
    assert torch.equal(c["vertices"], m["vertices"][c["vertex_ids"]]) and torch.equal(c["vertex_colors"], m["vertex_colors"][c["vertex_ids"]])
    for kw in (dict(keep_largest=1), dict(min_fraction=0.5)):
        again = mesh.clean_mesh(m["vertices"], m["faces"], m["vertex_colors"], **kw)
        assert all(torch.equal(again[k], c[k]) for k in ("vertices", "faces", "vertex_colors", "vertex_ids"))
    rgb8 = (c["vertex_colors"].clamp(0, 1) * 255).round().to(torch.uint8)
    path = str(tmp_path / "clean.ply")
    ply.save_mesh_ply(path, c["vertices"], c["faces"], rgb8)
    rv, rf, rc = ply.read_mesh_ply(path)
    assert np.array_equal(rv, v) and np.array_equal(rf, f) and np.array_equal(rc, rgb8.cpu().numpy())


@pytest.fixture(scope="module")
def blob(f3d, gpu_device):
    """The synthetic blob of the TSDF suite: 4,096 opaque Gaussians in a ball of radius 0.4 at the orbit's centre, 8 orbit cameras of 64^2."""
    dev = gpu_device
    P = 4096
    g = synthetic.make_gaussians(P, s0=0.04, seed=2, device="cpu")
    gen = torch.Generator().manual_seed(5)
    d = torch.randn(P, 3, generator=gen)
    g["xyz"] = (d / d.norm(dim=1, keepdim=True) * torch.rand(P, 1, generator=gen) ** (1 / 3) * 0.4 + torch.tensor([0.0, 0.0, 7.667])).float().contiguous()
    g["opacity"] = torch.full((P, 1), 0.95)
    g["features_dc"] = torch.rand(P, 1, 3, generator=gen) * 3.0 - 1.5
    g["features_rest"] = torch.zeros(P, 3, 3)
    cams = synthetic.orbit_cameras(8, resolution=64, device=dev)
    pc = {k: v.to(dev)[None].contiguous() for k, v in g.items()}
    return pc, cams


def test_extract_mesh_tsdf_keywords(f3d, gpu_device, blob):
    pc, cams = blob
    bg = torch.zeros(3, device=gpu_device)
    args = (pc, 0, cams["viewmatrix"], cams["projmatrix"], cams["campos"], bg, cams["cfg"])
    plain = mesh.extract_mesh_tsdf(*args, resolution=32)
    none = mesh.extract_mesh_tsdf(*args, resolution=32, min_component_faces=None, keep_largest=None)
    assert sorted(plain) == sorted(none) == ["faces", "interp_v", "tets", "vertex_colors", "vertices"]
    assert all(torch.equal(plain[k], none[k]) for k in plain)
    mc = mesh.mesh_components(plain["faces"], plain["vertices"].shape[0])
    sizes = mc["component_sizes"].tolist()
    clean = mesh.extract_mesh_tsdf(*args, resolution=32, keep_largest=1)
    after = mesh.mesh_components(clean["faces"], clean["vertices"].shape[0])
    print(f"blob: {plain['faces'].shape[0]} faces in {len(sizes)} components (largest {sizes[:4]}); keep_largest=1 leaves {clean['faces'].shape[0]} faces")
    assert len(sizes) >= 1 and after["component_sizes"].tolist() == [sizes[0]] and clean["faces"].shape[0] == sizes[0]
    assert clean["components"]["component_sizes"].tolist() == [sizes[0]] and clean["components"]["face_component"].shape[0] == sizes[0]
    ids = clean["components"]["vertex_ids"]
    assert torch.equal(clean["vertices"], plain["vertices"][ids]) and torch.equal(clean["vertex_colors"], plain["vertex_colors"][ids])
    assert torch.equal(clean["interp_v"], plain["interp_v"]) and torch.equal(clean["tets"], plain["tets"])
    assert torch.equal(ids[clean["faces"]], plain["faces"][mc["face_component"] == 0])
    both = mesh.extract_mesh_tsdf(*args, resolution=32, min_component_faces=sizes[0], keep_largest=5)
    assert torch.equal(both["faces"], clean["faces"]) and torch.equal(both["vertices"], clean["vertices"])


def test_clean_mesh_keeps_gradients(gpu_device):
    dev = gpu_device
    faces, N = M.oddities()
    ft = _dev(faces, dev)
    v = torch.rand(N, 3, device=dev).requires_grad_()
    col = torch.rand(N, 3, device=dev).requires_grad_()
    c = mesh.clean_mesh(v, ft, col, keep_largest=2)
    ids = c["vertex_ids"]
    assert ids.tolist() == [1, 2, 3, 9, 10, 11, 12, 13] and c["vertices"].requires_grad and not c["faces"].requires_grad
    w = torch.arange(1, ids.shape[0] + 1, dtype=torch.float32, device=dev)[:, None].expand(-1, 3)
    (c["vertices"] * w).sum().backward(retain_graph=True)
    want = torch.zeros(N, 3, device=dev)
    want[ids] = w
    print(f"gradient rows {torch.nonzero(v.grad.abs().sum(1)).reshape(-1).tolist()} (kept vertices {ids.tolist()})")
    assert torch.equal(v.grad, want) and col.grad is None
    (c["vertex_colors"] * 2.0).sum().backward()
    assert torch.equal(col.grad, (want > 0).float() * 2.0)
    with pytest.raises(RuntimeError, match="HIP device"):
        mesh.clean_mesh(v.detach().cpu(), ft, keep_largest=1)
    with pytest.raises(ValueError):
        mesh.clean_mesh(v, ft.reshape(-1, 4)[:, :2])


def test_extract_mesh_keywords(f3d, gpu_device):
    """The tetrahedral route (the scene of its own suite, rebuilt here: 300 opaque Gaussians in a ball under 3 cameras of 64^2, a 9^3 Kuhn
    grid): without the keywords the dict is the earlier one; with them its keys are untouched and the cleaned pair is added."""
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
    assert sorted(plain) == ["faces", "faces_filtered", "keep", "vertices", "vertices_filtered"]
    got = mesh.extract_mesh(*args, keep_largest=1)
    assert sorted(got) == sorted(list(plain) + ["vertices_clean", "faces_clean"]) and all(torch.equal(plain[k], got[k]) for k in plain)
    want = mesh.clean_mesh(plain["vertices_filtered"], plain["faces_filtered"], keep_largest=1)
    mc = mesh.mesh_components(plain["faces_filtered"], plain["vertices_filtered"].shape[0])
    print(f"tetrahedral route: {plain['faces_filtered'].shape[0]} filtered faces in components {mc['component_sizes'].tolist()[:8]}; "
          f"keep_largest=1 leaves {got['faces_clean'].shape[0]}")
    assert plain["faces_filtered"].shape[0] > 0 and got["faces_clean"].shape[0] == int(mc["component_sizes"][0])
    assert torch.equal(got["faces_clean"], want["faces"]) and torch.equal(got["vertices_clean"], want["vertices"])
    least = int(mc["component_sizes"][-1])
    some, want = mesh.extract_mesh(*args, min_component_faces=least + 1), mesh.clean_mesh(plain["vertices_filtered"], plain["faces_filtered"], min_faces=least + 1)
    assert torch.equal(some["faces_clean"], want["faces"]) and torch.equal(some["vertices_clean"], want["vertices"])
