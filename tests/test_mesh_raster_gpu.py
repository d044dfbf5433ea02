"""GPU tests of the mesh rasteriser: f3dg_mesh_raster through ctypes, mesh.render_mesh / interpolate_vertex_attributes /
mesh_depth_agreement on top of it, and the TSDF route end to end. Truth and the shared meshes are tests/mesh_raster_truth.py. Against the
restatement, face_id and every entry of h_counts (the covered pixels among them) are compared for EXACT equality and depth, bary and the
interpolated attributes for exact equality of their BIT PATTERNS over every pixel: the kernels and the restatement share the operation
order and use IEEE + - * / and rint in float64 only, with one rounding to float32. Every figure is printed before it is asserted
(``pytest -s``).

The image is 33 x 29 (no multiple of a wave or a tile) under V = 3 orbit cameras, or under an identity camera where a mesh has to land
on the sub-pixel lattice exactly."""
import ctypes as C

import numpy as np
import pytest
import torch

from f3dgaus_amd import _lib, mesh, synthetic
import mesh_raster_truth as R
import mesh_smooth_truth as S

pytestmark = pytest.mark.gpu
H, W = 29, 33
CENTRE = np.array([0.0, 0.0, 7.667])
SENT_I, SENT_F = -5, -123.25
_TRUTH = {}


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _orbit(n=3):
    cams = synthetic.orbit_cameras(n, resolution=32)
    return cams["viewmatrix"].numpy().astype(np.float32), float(cams["cfg"]["model"]["fov"])


def _truth(name, *args, **kw):
    """Computed once per case, shared, never modified."""
    if name not in _TRUTH:
        _TRUTH[name] = R.raster(*args, **kw)
    return _TRUTH[name]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _raw(P, faces, wv, fx, fy, dev, *, z_near=0.01, cull="none", attrs=None, dtype=torch.int64, h=H, w=W):
    """f3dg_mesh_raster on outputs pre-filled with a sentinel: (rc, dict of numpy outputs, h_counts)."""
    L = _lib.lib()
    vt = torch.from_numpy(np.ascontiguousarray(P, np.float32)).to(dev)
    ft = torch.from_numpy(np.ascontiguousarray(faces)).to(dev).to(dtype).reshape(-1, 3)
    wt = torch.from_numpy(np.ascontiguousarray(wv, np.float32)).to(dev).reshape(-1, 4, 4)
    at = None if attrs is None else torch.from_numpy(np.ascontiguousarray(attrs, np.float32)).to(dev)
    N, F, V, Cn = vt.shape[0], ft.shape[0], wt.shape[0], 0 if at is None else at.shape[1]
    nbytes = L.f3dg_mesh_raster_workspace_bytes(V, F, h, w)
    assert nbytes > 0
    ws = torch.zeros(nbytes, dtype=torch.uint8, device=dev)
    face_id = torch.full((V, h, w), SENT_I, dtype=torch.int32, device=dev)
    depth = torch.full((V, h, w), SENT_F, dtype=torch.float32, device=dev)
    bary = torch.full((V, 3, h, w), SENT_F, dtype=torch.float32, device=dev)
    out = torch.full((V, Cn, h, w), SENT_F, dtype=torch.float32, device=dev) if Cn else None
    hc = (C.c_longlong * 7)(*([-7] * 7))
    rc = L.f3dg_mesh_raster(_stream(), _lib.ptr(ws), nbytes, N, F, _lib.ptr(vt), _lib.ptr(ft), int(dtype == torch.int32), V, _lib.ptr(wt),
                            float(fx), float(fy), h, w, float(z_near), R.CULL[cull], Cn, _lib.ptr(at), _lib.ptr(face_id), _lib.ptr(depth),
                            _lib.ptr(bary), _lib.ptr(out), hc)
    torch.cuda.synchronize()
    got = {"face_id": face_id.cpu().numpy(), "depth": depth.cpu().numpy(), "bary": bary.cpu().numpy(),
           "attrs_out": None if out is None else out.cpu().numpy()}
    return rc, got, list(hc)


def _compare(name, rc, got, hc, want):
    """Everything against the restatement, over every pixel; the figures first."""
    n_id = int((got["face_id"] != want["face_id"]).sum())
    diffs = {k: int((_bits(got[k]) != _bits(want[k])).sum()) for k in ("depth", "bary", "attrs_out") if want[k] is not None}
    print(f"{name}: rc {rc}; h_counts {hc} (truth {want['counts']}); face_id differs at {n_id} of {want['face_id'].size} pixels; "
          f"elements whose bits differ: {diffs}")
    assert rc == _lib.OK and hc == want["counts"]
    assert n_id == 0 and hc[6] == int((got["face_id"] >= 0).sum())
    assert all(v == 0 for v in diffs.values())
    assert (got["attrs_out"] is None) == (want["attrs_out"] is None)


def _sphere(subdivisions, radius=0.5):
    P, faces = S.icosphere(subdivisions, noise=0.02, seed=4)
    rng = np.random.default_rng(11)
    normals = P / np.linalg.norm(P, axis=1, keepdims=True)
    attrs = np.concatenate([rng.uniform(0, 1, (len(P), 3)), normals], axis=1).astype(np.float32)
    return (P * radius + CENTRE).astype(np.float32), faces, attrs


@pytest.mark.parametrize("cull", ["none", "back", "front"])
def test_icosphere_with_colours_and_normals_under_the_orbit(gpu_device, cull):
    wv, fov = _orbit()
    fx, fy = R.focal(fov, H, W)
    P, faces, attrs = _sphere(2)
    assert len(faces) == 320
    want = _truth(f"icosphere {cull}", P, faces, wv, fx, fy, H, W, cull=cull, attrs=attrs)
    runs = []
    for dtype in (torch.int64, torch.int32, torch.int64):
        rc, got, hc = _raw(P, faces, wv, fx, fy, gpu_device, cull=cull, attrs=attrs, dtype=dtype)
        _compare(f"icosphere 320, cull {cull}, {dtype}", rc, got, hc, want)
        runs.append(got)
    for r in runs[1:]:                                             # int32 = int64 = a second run, byte for byte
        assert all(r[k].tobytes() == runs[0][k].tobytes() for k in r)
    assert want["counts"][6] > 300 and (cull == "none") == (want["counts"][4] == 0)
    # the Python face: the same numbers, colours and normals in one call of C = 6
    t = lambda a, dt=None: torch.from_numpy(np.ascontiguousarray(a)).to(gpu_device)
    r = mesh.render_mesh(t(P), t(faces), t(wv), fov, (H, W), vertex_colors=t(attrs[:, :3].copy()), vertex_normals=t(attrs[:, 3:].copy()), cull=cull)
    g = runs[0]
    assert np.array_equal(r["face_id"].cpu().numpy(), g["face_id"]) and np.array_equal(_bits(r["depth"].cpu().numpy()), _bits(g["depth"]))
    assert np.array_equal(_bits(r["bary"].cpu().numpy()), _bits(g["bary"])) and np.array_equal(_bits(r["color"].cpu().numpy()), _bits(g["attrs_out"][:, :3]))
    assert np.array_equal(r["alpha"].cpu().numpy(), (g["face_id"] >= 0).astype(np.float32))
    assert [r["counts"][k] for k in R.COUNT_NAMES] == want["counts"]
    n = r["normal"].cpu().numpy().astype(np.float64)
    length = np.sqrt((n * n).sum(axis=1))
    hit = g["face_id"] >= 0
    assert np.abs(length[hit] - 1).max() < 1e-6 and not n.transpose(0, 2, 3, 1)[~hit].any()
    only_c = mesh.render_mesh(t(P), t(faces), t(wv), fov, (H, W), vertex_colors=t(attrs[:, :3].copy()), cull=cull)
    assert only_c["normal"] is None and torch.equal(only_c["color"], r["color"])
    plain = mesh.render_mesh(t(P), t(faces), t(wv), fov, (H, W), cull=cull)
    assert plain["color"] is None and plain["normal"] is None and torch.equal(plain["depth"], r["depth"])


def test_the_half_pixel_jittered_grid_lands_on_the_lattice(gpu_device):
    on_edge = 0
    for seed in (0, 1, 2):
        U, V, faces, (i0, i1, j0, j1) = R.jittered_grid(6, 5, seed)
        P = R.lattice_to_world(U, V, H, W, 16.0, 4.0)
        want = _truth(f"jittered {seed}", P, faces, R.identity_view(), 16.0, 16.0, H, W)
        inside = np.zeros((H, W), bool)
        inside[j0:j1 + 1, i0:i1 + 1] = True
        assert np.array_equal(want["face_id"][0] >= 0, inside) and want["counts"][0] == 60       # every interior centre once, none outside
        for f in faces:                                            # the case contains centres that lie exactly on an edge
            _, sE = R.cover_all_pixels([int(U[i]) for i in f], [int(V[i]) for i in f], H, W)
            on_edge += int(sum(((e == 0) & inside).sum() for e in sE))
        rc, got, hc = _raw(P, faces, R.identity_view(), 16.0, 16.0, gpu_device)
        _compare(f"jittered grid {seed}", rc, got, hc, want)
    print(f"pixel centres exactly on an edge or a corner: {on_edge}")
    assert on_edge > 0


def test_a_40_by_40_grid_seen_small(gpu_device):
    wv, fov = _orbit()
    fx, fy = R.focal(fov, H, W)
    P, faces = R.plane_grid(40, 40, CENTRE, 0.5, seed=2)
    attrs = np.random.default_rng(1).uniform(-1, 1, (len(P), 1)).astype(np.float32)
    want = _truth("grid 40", P, faces, wv, fx, fy, H, W, attrs=attrs)
    boxes = np.array(want["boxes"])
    print(f"40 x 40 grid: {len(boxes)} rasterised pairs, {int((boxes == 0).sum())} with no pixel centre in their box, largest box {boxes.max()}")
    assert (boxes == 0).any() and (boxes > 0).any()                # some faces cover no centre and some do
    rc, got, hc = _raw(P, faces, wv, fx, fy, gpu_device, attrs=attrs, dtype=torch.int32)
    _compare("40 x 40 grid, C = 1", rc, got, hc, want)


def test_full_frame_triangles_behind_small_ones(gpu_device):
    P, faces = R.big_and_small((0.0, 0.0, 4.0))
    attrs = np.random.default_rng(2).uniform(0, 1, (len(P), 8)).astype(np.float32)
    want = _truth("big and small", P, faces, R.identity_view(), 16.0, 16.0, H, W, attrs=attrs)
    boxes = np.array(want["boxes"])
    classes = [int(((boxes > 0) & (boxes <= R.SMALL)).sum()), int(((boxes > R.SMALL) & (boxes <= R.WAVE)).sum()), int((boxes > R.WAVE).sum())]
    print(f"boxes: {sorted(boxes.tolist())}; one thread / one wave / one workgroup: {classes}")
    assert all(classes) and classes[2] >= 2 and want["counts"][5] == classes[1] + classes[2]     # both sides of both limits
    for dtype in (torch.int64, torch.int32):
        rc, got, hc = _raw(P, faces, R.identity_view(), 16.0, 16.0, gpu_device, attrs=attrs, dtype=dtype)
        _compare(f"two full-frame triangles behind 20, C = 8, {dtype}", rc, got, hc, want)
    assert hc[5] == want["counts"][5] and hc[6] == H * W           # the queue count; the two large triangles fill the frame
    assert set(np.unique(got["face_id"]).tolist()) > {0, 1}        # and the small ones in front of them show


def test_equal_depth_duplicates_go_to_the_lower_id(gpu_device):
    wv, fov = _orbit()
    fx, fy = R.focal(fov, H, W)
    P, faces, _ = _sphere(1)
    twice = np.concatenate([faces, faces])
    want = _truth("duplicates", P, twice, wv, fx, fy, H, W)
    rc, got, hc = _raw(P, twice, wv, fx, fy, gpu_device)
    _compare("every face twice", rc, got, hc, want)
    assert got["face_id"].max() < len(faces) and hc[6] > 0
    rc, rev, _ = _raw(P, twice[::-1].copy(), wv, fx, fy, gpu_device)
    assert rc == _lib.OK and rev["face_id"].max() < len(faces) and np.array_equal(_bits(rev["depth"]), _bits(got["depth"]))


def test_dropped_corners_are_counted_and_leave_the_other_faces_alone(gpu_device):
    P, faces = R.plane_grid(2, 2, (0.0, 0.0, 4.0), 1.0)
    P = np.concatenate([P, np.array([[0, 0, -1.0], [np.nan, 0, 4.0], [1e5, 0, 4.0], [0, 0, np.inf]], np.float32)])
    n0 = len(P) - 4
    extra = np.array([[0, 1, n0], [0, 1, n0 + 1], [0, 1, n0 + 2], [0, 1, n0 + 3], [0, 0, 1], [0, 4, 8]])
    both = np.concatenate([faces, extra])
    want = _truth("dropped", P, both, R.identity_view(), 16.0, 16.0, H, W)
    assert want["counts"][:5] == [8, 3, 1, 2, 0]
    rc, got, hc = _raw(P, both, R.identity_view(), 16.0, 16.0, gpu_device)
    _compare("behind z_near, NaN, infinite, beyond the guard band, degenerate", rc, got, hc, want)
    rc, base, _ = _raw(P, faces, R.identity_view(), 16.0, 16.0, gpu_device)
    assert rc == _lib.OK and all(base[k].tobytes() == got[k].tobytes() for k in ("face_id", "depth", "bary"))
    near = _truth("z_near 4.5", P, faces, R.identity_view(), 16.0, 16.0, H, W, z_near=4.5)          # the whole plane at z = 4 is in front of it
    rc, got, hc = _raw(P, faces, R.identity_view(), 16.0, 16.0, gpu_device, z_near=4.5)
    _compare("everything behind z_near", rc, got, hc, near)
    assert hc[:2] == [0, 8] and hc[6] == 0 and (got["face_id"] == -1).all() and not got["depth"].any()


@pytest.mark.parametrize("dtype", [torch.int64, torch.int32])
@pytest.mark.parametrize("bad", ["N", "-1"])
def test_an_id_out_of_range_refuses_the_mesh_and_writes_nothing(gpu_device, dtype, bad):
    wv, fov = _orbit()
    fx, fy = R.focal(fov, H, W)
    P, faces, attrs = _sphere(2)
    faces = faces.copy()
    faces[len(faces) // 2, 1] = len(P) if bad == "N" else -1
    rc, got, hc = _raw(P, faces, wv, fx, fy, gpu_device, attrs=attrs, dtype=dtype)
    print(f"id {bad} ({dtype}): rc {rc}, h_counts {hc}")
    assert rc == _lib.ERR_BAD_ARG and hc == [-7] * 7
    assert (got["face_id"] == SENT_I).all() and all((got[k] == np.float32(SENT_F)).all() for k in ("depth", "bary", "attrs_out"))
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(gpu_device)
    with pytest.raises(_lib.F3dgError):
        mesh.render_mesh(t(P), t(faces).to(dtype), t(wv), fov, (H, W))


def test_one_face_one_view_and_no_face(gpu_device):
    P = np.array([[-0.6, -0.5, 4.0], [0.9, -0.4, 4.5], [0.1, 0.8, 5.0]], np.float32)
    attrs = np.array([[1, 0], [0, 1], [0.5, 0.25]], np.float32)
    for faces in (np.array([[0, 1, 2]]), np.array([[0, 2, 1]])):
        want = R.raster(P, faces, R.identity_view(), 16.0, 16.0, H, W, attrs=attrs)
        rc, got, hc = _raw(P, faces, R.identity_view(), 16.0, 16.0, gpu_device, attrs=attrs)
        _compare(f"F = 1, V = 1, {faces.tolist()}", rc, got, hc, want)
        assert hc[0] == 1 and hc[6] > 0
    rc, got, hc = _raw(P, np.zeros((0, 3), np.int64), R.identity_view(), 16.0, 16.0, gpu_device, attrs=attrs)
    assert rc == _lib.OK and hc == [0] * 7 and (got["face_id"] == -1).all() and not got["depth"].any() and not got["attrs_out"].any()
    want = R.raster(P, np.array([[0, 1, 2]]), R.identity_view(), 16.0, 16.0, 1, 1)
    rc, got, hc = _raw(P, np.array([[0, 1, 2]]), R.identity_view(), 16.0, 16.0, gpu_device, h=1, w=1)
    _compare("a 1 x 1 image", rc, got, hc, want)


def test_the_attribute_grad_route_matches_the_fused_output(gpu_device):
    dev = gpu_device
    wv, fov = _orbit()
    P, faces, attrs = _sphere(2)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    vt, ft, wt = t(P), t(faces), t(wv)
    colors = t(attrs[:, :3].copy())
    fused = mesh.render_mesh(vt, ft, wt, fov, (H, W), vertex_colors=colors)
    leaf = colors.clone().requires_grad_()
    r = mesh.render_mesh(vt, ft, wt, fov, (H, W), vertex_colors=leaf)
    assert r["color"].requires_grad and torch.equal(r["face_id"], fused["face_id"]) and torch.equal(r["bary"], fused["bary"])
    again = mesh.interpolate_vertex_attributes(leaf, ft, r["face_id"], r["bary"])
    assert torch.equal(again, r["color"])
    # float32 weights (2^-24), three float32 products (2^-24 each) and two float32 additions (2^-24 each) of terms that sum to at
    # most max |a|, against the fused double sum rounded once (2^-24): under 4 * 2^-23 * max |a|
    bound = 4 * 2.0 ** -23 * float(colors.abs().max())
    err = float((r["color"].detach().double() - fused["color"].double()).abs().max())
    print(f"torch gather against the fused output: max |difference| {err:.3e} (bound {bound:.3e})")
    assert err <= bound
    G = torch.rand(r["color"].shape, device=dev, generator=torch.Generator(device=dev).manual_seed(3))
    (r["color"] * G).sum().backward()
    hit = r["face_id"] >= 0
    corners = ft[r["face_id"].clamp(min=0).long()]                                  # [V,H,W,3]
    want = torch.zeros(leaf.shape, dtype=torch.float64, device=dev)
    mass = torch.zeros(leaf.shape, dtype=torch.float64, device=dev)
    terms = torch.zeros(leaf.shape[0], dtype=torch.float64, device=dev)
    for k in range(3):
        wk = (r["bary"][:, k].double() * hit)[..., None] * G.permute(0, 2, 3, 1).double()           # [V,H,W,3]
        want.index_add_(0, corners[..., k][hit], wk[hit])
        mass.index_add_(0, corners[..., k][hit], wk[hit].abs())
        terms.index_add_(0, corners[..., k][hit], torch.ones(int(hit.sum()), dtype=torch.float64, device=dev))
    # a float32 sum of n terms in any order is within (n + 2) 2^-24 sum |terms| of the exact one (each term rounded once more)
    slack = (terms[:, None] + 2) * 2.0 ** -24 * mass
    worst = float(((leaf.grad.double() - want).abs() - slack).max())
    print(f"gradient to the attributes against the index_add_ of the weights: largest excess over the summation bound {worst:.3e}")
    assert worst <= 0 and float(want.abs().max()) > 0
    assert not vt.requires_grad and leaf.grad.shape == leaf.shape


def test_extract_mesh_tsdf_then_render_mesh_from_the_same_cameras(f3d, gpu_device):
    """The synthetic blob of the TSDF suite (4,096 opaque Gaussians in a ball of radius 0.4, 8 orbit cameras of 64^2) fused into a 32^3
    volume, drawn again from its cameras and held against the depth the Gaussians composited."""
    from f3dgaus_amd.gaussian_renderer import render_views
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
    m = mesh.extract_mesh_tsdf(*args, resolution=32, vertex_normals=True)
    fov = cams["cfg"]["model"]["fov"]
    r = mesh.render_mesh(m["vertices"], m["faces"], cams["viewmatrix"], fov, 64, vertex_colors=m["vertex_colors"].contiguous(),
                         vertex_normals=m["vertex_normals"])
    assert r["face_id"].shape == r["depth"].shape == r["alpha"].shape == (8, 64, 64) and r["bary"].shape == (8, 3, 64, 64)
    assert r["color"].shape == r["normal"].shape == (8, 3, 64, 64) and r["face_id"].dtype == torch.int32
    assert sum(r["counts"][k] for k in ("rasterised", "near", "guard", "degenerate", "culled")) == 8 * m["faces"].shape[0]
    assert r["counts"]["covered"] == int((r["face_id"] >= 0).sum()) > 0
    out = render_views(*args, channels="rgb_depth_alpha", epilogue=False)
    a = mesh.mesh_depth_agreement(r["depth"], r["alpha"], out["rendered_depth"], out["rendered_alpha"])
    print(f"blob at 32^3: {m['faces'].shape[0]} faces, {r['counts']}; depth agreement {a}")
    assert np.isfinite(a["mean"]) and np.isfinite(a["max"]) and 0 <= a["mean"] <= a["max"]
    assert a["n_mesh"] == r["counts"]["covered"] and 0 < a["n_both"] <= min(a["n_mesh"], a["n_render"])
