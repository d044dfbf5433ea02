"""GPU tests of the vertex colour baking: f3dg_mesh_bake_colors through ctypes, mesh.bake_vertex_colors on top of it, and both mesh
routes with ``color_from_views``. Truth and the shared scenes are tests/mesh_bake_truth.py. Against the restatement, n_used, best_view and
all eight counts are compared for EXACT equality and colors and weight for exact equality of their BIT PATTERNS over every vertex: the
kernel and the restatement share the operation order and use IEEE + - * /, rint and floor in float64 only, with one rounding to
float32. The four outputs are pre-filled with sentinels, so every element is shown to be assigned. Every figure is printed before it is
asserted (``pytest -s``). The raw calls take face_id and depth from mesh_raster_truth.raster; the Python face draws them itself."""
import ctypes as C

import numpy as np
import pytest
import torch

from f3dgaus_amd import _lib, mesh, synthetic
import mesh_bake_truth as B
import mesh_raster_truth as R
import mesh_smooth_truth as S

pytestmark = pytest.mark.gpu
H, W = 29, 33
SENT_I, SENT_F = -5, -123.25
DEPTH_TOL, COS_MIN = 0.05, 0.3
_CACHE = {}


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _once(name, make):
    """Computed once, shared, never modified."""
    if name not in _CACHE:
        _CACHE[name] = make()
    return _CACHE[name]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _raw(dev, P, normals, wv, fx, fy, images, face_id, depth, *, alpha=None, alpha_min=0.5, depth_tol=DEPTH_TOL, cos_min=COS_MIN, mode="blend",
         z_near=0.01):
    """f3dg_mesh_bake_colors on outputs pre-filled with a sentinel: (rc, dict of numpy outputs, h_counts)."""
    L = _lib.lib()
    t = lambda a, dt: None if a is None else torch.from_numpy(np.ascontiguousarray(a, dt)).to(dev)
    vt, nt, wt, it = t(P, np.float32), t(normals, np.float32), t(wv, np.float32).reshape(-1, 4, 4), t(images, np.float32)
    ft, dt, at = t(face_id, np.int32), t(depth, np.float32), t(alpha, np.float32)
    N, (V, Cn, h, w) = vt.shape[0], it.shape
    nbytes = L.f3dg_mesh_bake_workspace_bytes(V, N, h, w)
    assert nbytes > 0
    ws = torch.zeros(nbytes, dtype=torch.uint8, device=dev)
    colors = torch.full((N, Cn), SENT_F, dtype=torch.float32, device=dev)
    weight = torch.full((N,), SENT_F, dtype=torch.float32, device=dev)
    n_used = torch.full((N,), SENT_I, dtype=torch.int32, device=dev)
    best_view = torch.full((N,), SENT_I, dtype=torch.int32, device=dev)
    hc = (C.c_longlong * 8)(*([-7] * 8))
    rc = L.f3dg_mesh_bake_colors(_stream(), _lib.ptr(ws), nbytes, N, _lib.ptr(vt), _lib.ptr(nt), V, _lib.ptr(wt), float(fx), float(fy), h, w,
                                 float(z_near), Cn, _lib.ptr(it), _lib.ptr(ft), _lib.ptr(dt), _lib.ptr(at), float(alpha_min), float(depth_tol),
                                 float(cos_min), mode if isinstance(mode, int) else B.MODES[mode], _lib.ptr(colors), _lib.ptr(weight),
                                 _lib.ptr(n_used), _lib.ptr(best_view), hc)
    torch.cuda.synchronize()
    got = {"colors": colors.cpu().numpy(), "weight": weight.cpu().numpy(), "n_used": n_used.cpu().numpy(), "best_view": best_view.cpu().numpy()}
    return rc, got, list(hc)


def _compare(name, rc, got, hc, want):
    """Everything against the restatement, over every vertex; the figures first."""
    ints = {k: int((got[k] != want[k]).sum()) for k in ("n_used", "best_view")}
    bits = {k: int((_bits(got[k]) != _bits(want[k])).sum()) for k in ("colors", "weight")}
    print(f"{name}: rc {rc}; h_counts {hc} (truth {want['counts']}); vertices that differ: {ints}; elements whose bits differ: {bits} "
          f"of {want['colors'].size} / {want['weight'].size}")
    assert rc == _lib.OK and hc == want["counts"] and sum(hc[:7]) == want["cls"].size
    assert all(v == 0 for v in ints.values()) and all(v == 0 for v in bits.values())
    assert got["colors"].shape == want["colors"].shape and hc[7] == int((got["n_used"] > 0).sum())


def _sphere(Cn):
    def make():
        sc = B.sphere_scene(2, 3, H, W, Cn, 4)
        assert len(sc["P"]) == 162 and len(sc["faces"]) == 320
        sc["raster"] = _once("sphere raster", lambda: R.raster(sc["P"], sc["faces"], sc["wv"], sc["fx"], sc["fy"], H, W))
        perm = np.random.default_rng(6).permutation(162)                   # new vertex k is old vertex perm[k]
        inv = np.argsort(perm)
        sc["perm"] = perm
        if "sphere raster permuted" not in _CACHE:                         # the same faces over re-indexed vertices: the same z-buffer
            r2 = R.raster(sc["P"][perm], inv[sc["faces"]], sc["wv"], sc["fx"], sc["fy"], H, W)
            assert np.array_equal(r2["face_id"], sc["raster"]["face_id"]) and np.array_equal(_bits(r2["depth"]), _bits(sc["raster"]["depth"]))
            _CACHE["sphere raster permuted"] = True
        return sc
    return _once(f"sphere {Cn}", make)


@pytest.mark.parametrize("with_alpha", [False, True])
@pytest.mark.parametrize("mode", ["blend", "best"])
@pytest.mark.parametrize("with_normals", [False, True])
@pytest.mark.parametrize("Cn", [1, 3, 8])
def test_noisy_icosphere_under_the_orbit(gpu_device, Cn, with_normals, mode, with_alpha):
    sc = _sphere(Cn)
    r = sc["raster"]
    normals, alpha = sc["normals"] if with_normals else None, sc["alpha"] if with_alpha else None
    kw = dict(alpha=alpha, mode=mode)
    want = _once(f"sphere {Cn} {with_normals} {mode} {with_alpha}", lambda: B.bake(
        sc["P"], normals, sc["wv"], sc["fx"], sc["fy"], sc["images"], r["face_id"], r["depth"], depth_tol=DEPTH_TOL, cos_min=COS_MIN, **kw))
    n = dict(zip(B.COUNT_NAMES, want["counts"]))
    assert n["used"] > 0 and n["occluded"] > 0 and n["uncovered"] > 0 and n["masked"] > 0 and (n["grazing"] > 0) == with_normals
    assert (want["n_used"] > 1).any() and (want["n_used"] == 0).any()
    runs = []
    for _ in range(2):
        rc, got, hc = _raw(gpu_device, sc["P"], normals, sc["wv"], sc["fx"], sc["fy"], sc["images"], r["face_id"], r["depth"], **kw)
        _compare(f"icosphere 162, C = {Cn}, normals {with_normals}, {mode}, alpha {with_alpha}", rc, got, hc, want)
        runs.append(got)
    assert all(runs[1][k].tobytes() == runs[0][k].tobytes() for k in runs[0])          # a second run: identical bytes
    perm = sc["perm"]                                                                  # permuted vertices: the permuted outputs
    rc, got, hc = _raw(gpu_device, sc["P"][perm], None if normals is None else normals[perm], sc["wv"], sc["fx"], sc["fy"], sc["images"],
                       r["face_id"], r["depth"], **kw)
    assert rc == _lib.OK and hc == want["counts"]
    assert all(got[k].tobytes() == runs[0][k][perm].tobytes() for k in got)


def test_plane_scenes(gpu_device):
    for shift in (0, 128):
        P, faces, inner, (iu, iv) = B.pixel_plane(7, 9, shift)
        img = B.dyadic_image(1, 3, 7, 9, 1)
        want, r = _once(f"plane {shift}", lambda: B.bake_mesh(P, faces, None, R.identity_view(), B.FX, B.FX, img, depth_tol=0.01))
        rc, got, hc = _raw(gpu_device, P, None, R.identity_view(), B.FX, B.FX, img, r["face_id"], r["depth"], depth_tol=0.01)
        _compare(f"plane on the pixel lattice, shift {shift} / 256", rc, got, hc, want)
        i, j = iu[inner], iv[inner]
        if shift == 0:
            exact = img[0][:, j, i].T
        else:
            exact = ((img[0][:, j, i].astype(np.float64) + img[0][:, j, i + 1] + img[0][:, j + 1, i] + img[0][:, j + 1, i + 1]) / 4.0).T
        assert np.array_equal(got["colors"][inner].astype(np.float64), exact.astype(np.float64)) and (got["n_used"][inner] == 1).all()
    P, faces, expected = B.two_planes_scene()
    img = B.dyadic_image(1, 2, 8, 8, 3)
    want, r = _once("two planes", lambda: B.bake_mesh(P, faces, None, R.identity_view(), B.FX, B.FX, img, depth_tol=0.5))
    rc, got, hc = _raw(gpu_device, P, None, R.identity_view(), B.FX, B.FX, img, r["face_id"], r["depth"], depth_tol=0.5)
    _compare("two planes, a sliver, vertices off the image, at z_near and NaN", rc, got, hc, want)
    assert hc == expected


def test_more_views_than_the_table_holds(gpu_device):
    V, h, w = 130, 4, 5
    P, faces = S.icosphere(0)
    P = (P / np.linalg.norm(P, axis=1, keepdims=True) * 0.5 + B.CENTRE).astype(np.float32)
    assert len(P) == 12 and V > _lib.TSDF_MAX_VIEWS
    wv, fx, fy = B.orbit(V, h, w)
    img = np.random.default_rng(0).uniform(0, 1, (V, 2, h, w)).astype(np.float32)
    for mode in ("blend", "best"):
        want, r = _once(f"130 views {mode}", lambda: B.bake_mesh(P, faces, None, wv, fx, fy, img, depth_tol=DEPTH_TOL, mode=mode))
        used = want["cls"] == B.USED
        both = used[:128].any(axis=0) & used[128:].any(axis=0)             # views before and after a table of 128 both contribute
        print(f"130 views, {mode}: used per vertex before / after view 128: {used[:128].sum(axis=0).tolist()} / {used[128:].sum(axis=0).tolist()}")
        assert both.any()
        rc, got, hc = _raw(gpu_device, P, None, wv, fx, fy, img, r["face_id"], r["depth"], mode=mode)
        _compare(f"12 vertices under 130 views, {mode}", rc, got, hc, want)


def test_edge_sizes(gpu_device):
    img = B.dyadic_image(2, 3, 8, 8, 5)
    cover = lambda V, h, w: (np.zeros((V, h, w), np.int32), np.full((V, h, w), 4.0, np.float32))       # a z-buffer that covers everything at z = 4
    one = R.lattice_to_world(np.array([768]), np.array([640]), 8, 8, B.FX, 4.0)                        # u = 3, v = 2.5
    wv2 = np.concatenate([R.identity_view(), R.identity_view()])
    for name, P, wv, im in (("N = 1, V = 2", one, wv2, img), ("N = 1, V = 1", one, R.identity_view(), img[:1]),
                            ("V = 1", B.two_planes_scene()[0], R.identity_view(), img[:1])):
        f, d = cover(len(wv), 8, 8)
        want = B.bake(P, None, wv, B.FX, B.FX, im, f, d, depth_tol=0.01)
        rc, got, hc = _raw(gpu_device, P, None, wv, B.FX, B.FX, im, f, d, depth_tol=0.01)
        _compare(name, rc, got, hc, want)
    assert hc[B.USED] > 0
    # a 1 x 1 image: only u = v = 0 is inside
    P = np.array([[0, 0, 4], [0.125, 0, 4], [0, -0.125, 4], [0, 0, 2]], np.float32)
    im = B.dyadic_image(1, 3, 1, 1, 6)
    f, d = cover(1, 1, 1)
    want = B.bake(P, None, R.identity_view(), B.FX, B.FX, im, f, d, depth_tol=0.01)
    rc, got, hc = _raw(gpu_device, P, None, R.identity_view(), B.FX, B.FX, im, f, d, depth_tol=0.01)
    _compare("a 1 x 1 image", rc, got, hc, want)
    assert hc[:7] == [0, 2, 0, 0, 0, 0, 2] and np.array_equal(got["colors"][0], im[0, :, 0, 0]) and np.array_equal(got["colors"][3], im[0, :, 0, 0])
    # vertices exactly on the last column and the last row: the clamped tap has weight 0
    P = R.lattice_to_world(np.array([7 * 256, 7 * 256, 640]), np.array([640, 7 * 256, 7 * 256]), 8, 8, B.FX, 4.0)
    f, d = cover(1, 8, 8)
    want = B.bake(P, None, R.identity_view(), B.FX, B.FX, img[:1], f, d, depth_tol=0.01)
    rc, got, hc = _raw(gpu_device, P, None, R.identity_view(), B.FX, B.FX, img[:1], f, d, depth_tol=0.01)
    _compare("u = W - 1 and v = H - 1", rc, got, hc, want)
    assert hc[B.USED] == 3 and np.array_equal(got["colors"][1], img[0, :, 7, 7])
    assert np.array_equal(got["colors"][0].astype(np.float64), (img[0, :, 2, 7].astype(np.float64) + img[0, :, 3, 7]) / 2)


def test_a_refused_call_leaves_every_sentinel(gpu_device):
    sc = _sphere(3)
    r = sc["raster"]
    for kw in (dict(mode=2), dict(mode=-1), dict(cos_min=1.5), dict(depth_tol=-1.0)):
        rc, got, hc = _raw(gpu_device, sc["P"], sc["normals"], sc["wv"], sc["fx"], sc["fy"], sc["images"], r["face_id"], r["depth"], **kw)
        print(f"{kw}: rc {rc}, h_counts {hc}")
        assert rc == _lib.ERR_BAD_ARG and hc == [-7] * 8
        assert (got["n_used"] == SENT_I).all() and (got["best_view"] == SENT_I).all()
        assert (got["colors"] == np.float32(SENT_F)).all() and (got["weight"] == np.float32(SENT_F)).all()


def test_the_python_face(gpu_device):
    sc = _sphere(3)
    r = sc["raster"]
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(gpu_device)
    fov = float(synthetic.orbit_cameras(3, resolution=32)["cfg"]["model"]["fov"])
    for mode in ("blend", "best"):
        rc, raw, hc = _raw(gpu_device, sc["P"], sc["normals"], sc["wv"], sc["fx"], sc["fy"], sc["images"], r["face_id"], r["depth"], alpha=sc["alpha"], mode=mode)
        assert rc == _lib.OK
        args = (t(sc["P"]), t(sc["faces"]), t(sc["images"]), t(sc["wv"]), (sc["fx"], sc["fy"]))
        kw = dict(vertex_normals=t(sc["normals"]), alpha=t(sc["alpha"]), depth_tol=DEPTH_TOL, cos_min=COS_MIN, mode=mode)
        b = mesh.bake_vertex_colors(*args, **kw)
        assert np.array_equal(b["visibility"]["face_id"].cpu().numpy(), r["face_id"])
        for k, name in (("colors", "vertex_colors"), ("weight", "weight"), ("n_used", "n_used"), ("best_view", "best_view")):
            assert b[name].cpu().numpy().tobytes() == raw[k].tobytes(), (mode, name)
        assert [b["counts"][k] for k in _lib.BAKE_COUNTS] == hc
        again = mesh.bake_vertex_colors(*args, visibility=b["visibility"], **kw)                # a reused visibility
        assert again["visibility"] is b["visibility"]
        assert all(torch.equal(again[k], b[k]) for k in ("vertex_colors", "weight", "n_used", "best_view")) and again["counts"] == b["counts"]
        by_fov = mesh.bake_vertex_colors(args[0], args[1], args[2], args[3], fov, alpha=t(sc["alpha"])[:, None], mode=mode)     # fov in degrees, [V,1,H,W], the default tolerance
        assert by_fov["vertex_colors"].shape == (162, 3) and sum(by_fov["counts"][k] for k in B.CLASSES) == 3 * 162
    # convex weights: every channel of a used vertex lies within the range of the images (finite pixels)
    img = np.random.default_rng(3).uniform(0.25, 0.75, sc["images"].shape).astype(np.float32)
    b = mesh.bake_vertex_colors(t(sc["P"]), t(sc["faces"]), t(img), t(sc["wv"]), (sc["fx"], sc["fy"]), vertex_normals=t(sc["normals"]), depth_tol=DEPTH_TOL)
    seen = (b["n_used"] > 0).cpu().numpy()
    c = b["vertex_colors"].cpu().numpy()
    print(f"used vertices {int(seen.sum())}: colours in [{c[seen].min()}, {c[seen].max()}], images in [{img.min()}, {img.max()}]")
    assert seen.any() and c[seen].min() >= img.min() and c[seen].max() <= img.max() and not c[~seen].any()
    with pytest.raises(ValueError, match="mode"):
        mesh.bake_vertex_colors(t(sc["P"]), t(sc["faces"]), t(img), t(sc["wv"]), fov, mode="mean")
    with pytest.raises(ValueError, match="camera per image"):
        mesh.bake_vertex_colors(t(sc["P"]), t(sc["faces"]), t(img), t(sc["wv"])[:2], fov)


def _blob(dev):
    """The synthetic blob of test_mesh_raster_gpu.py: 4,096 opaque Gaussians in a ball of radius 0.4, 8 orbit cameras of 64^2."""
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
    return (pc, 0, cams["viewmatrix"], cams["projmatrix"], cams["campos"], torch.zeros(3, device=dev), cams["cfg"]), cams


def test_extract_mesh_tsdf_colours_from_the_views(f3d, gpu_device, tmp_path):
    from f3dgaus_amd.gaussian_renderer import render_views
    args, cams = _blob(gpu_device)
    kw = dict(resolution=32, smooth_iterations=2, vertex_normals=True)
    plain = mesh.extract_mesh_tsdf(*args, **kw)
    off = mesh.extract_mesh_tsdf(*args, color_from_views=False, **kw)
    same = lambda a, b: (torch.equal(a, b) if torch.is_tensor(a) else a == b)
    assert list(off) == list(plain) and all(same(off[k], plain[k]) for k in plain if k != "components")
    m = mesh.extract_mesh_tsdf(*args, color_from_views=True, **kw)
    assert set(m) == set(plain) | {"vertex_colors_tsdf", "color_views"}
    assert all(same(m[k], plain[k]) for k in plain if k not in ("vertex_colors", "components"))
    assert torch.equal(m["vertex_colors_tsdf"], plain["vertex_colors"])
    out = render_views(*args, channels="rgb_depth_alpha", epilogue=False)
    b = mesh.bake_vertex_colors(m["vertices"], m["faces"], out["render"].contiguous(), cams["viewmatrix"], cams["cfg"]["model"]["fov"],
                                vertex_normals=m["vertex_normals"], alpha=out["rendered_alpha"], depth_tol=_tsdf_tolerance(args, 32))
    seen = m["color_views"] > 0
    n_seen = int(seen.sum())
    print(f"blob at 32^3: {m['vertices'].shape[0]} vertices, {n_seen} coloured from the views, at most {int(m['color_views'].max())} views; "
          f"counts {b['counts']}")
    assert torch.equal(m["color_views"], b["n_used"]) and m["color_views"].dtype == torch.int32 and int(m["color_views"].max()) <= 8 and n_seen > 0
    assert torch.equal(m["vertex_colors"][seen], b["vertex_colors"][seen]) and torch.equal(m["vertex_colors"][~seen], plain["vertex_colors"][~seen])
    p = str(tmp_path / "coloured.ply")
    f3d.ply.save_mesh_ply(p, m["vertices"], m["faces"], (m["vertex_colors"].clamp(0, 1) * 255).round().to(torch.uint8), vertex_normals=m["vertex_normals"])
    v, f, c = f3d.ply.read_mesh_ply(p)
    assert np.array_equal(v, m["vertices"].cpu().numpy()) and np.array_equal(c, (m["vertex_colors"].clamp(0, 1) * 255).round().to(torch.uint8).cpu().numpy())


def _tsdf_tolerance(args, resolution):
    """depth_tol of extract_mesh_tsdf with its default bounds and truncation: two voxels of longest / (resolution - 9)."""
    xyz = args[0]["xyz"][args[1]]
    box = torch.stack([xyz.min(dim=0)[0], xyz.max(dim=0)[0]]).double().cpu()
    longest = max(b - a for a, b in zip(box[0].tolist(), box[1].tolist()))
    return 2 * (longest / (resolution - 9))


def test_extract_mesh_colours_from_the_views(f3d, gpu_device, tmp_path):
    """The tetrahedral fixture of test_mesh_extract_gpu.py: 300 Gaussians, a 9^3 Kuhn grid, 3 cameras of 64^2."""
    import mesh_truth
    from f3dgaus_amd import cameras
    from test_mesh_extract_gpu import CENTRE, _scene
    dev = gpu_device
    scene = _scene()
    d = lambda t: t.to(dev)
    cfg = cameras.default_cfg(resolution=64)
    cfg["model"]["max_sh_degree"] = scene["sh_degree"]
    pc = {"xyz": d(scene["means3D"])[None], "opacity": d(scene["opacities"])[None], "scaling": d(scene["scales"])[None],
          "rotation": d(scene["rotations"])[None], "features_dc": d(scene["shs"])[None, :, :1], "features_rest": d(scene["shs"])[None, :, 1:]}
    pts, tets = mesh_truth.kuhn_grid(9)
    pts = torch.from_numpy(((pts - 0.5) * 1.2 + np.array(CENTRE, dtype=np.float32)).astype(np.float32)).to(dev)
    args = (pc, 0, pts, torch.full((len(pts), 1), 0.04, device=dev), torch.from_numpy(tets).to(dev), d(scene["viewmatrix"]), d(scene["projmatrix"]),
            d(scene["campos"]), d(scene["bg"]), cfg)
    plain = mesh.extract_mesh(*args, n_binary_steps=2)
    off = mesh.extract_mesh(*args, n_binary_steps=2, color_from_views=False)
    assert list(off) == list(plain) and all(torch.equal(off[k], plain[k]) for k in plain)
    m = mesh.extract_mesh(*args, n_binary_steps=2, color_from_views=True)
    assert set(m) == set(plain) | {"vertex_colors", "color_views"} and all(torch.equal(m[k], plain[k]) for k in plain)
    n = m["vertices_filtered"].shape[0]
    print(f"tetrahedral route: {n} filtered vertices, {int((m['color_views'] > 0).sum())} coloured from the views")
    assert n > 0 and m["vertex_colors"].shape == (n, 3) and m["color_views"].shape == (n,) and int(m["color_views"].max()) <= 3
    assert (m["color_views"] > 0).any() and not m["vertex_colors"][m["color_views"] == 0].any()
    full = mesh.extract_mesh(*args, n_binary_steps=2, keep_largest=1, smooth_iterations=1, vertex_normals=True, color_from_views=True)
    assert full["vertex_colors"].shape == full["vertices_smooth"].shape == full["vertices_clean"].shape
    p = str(tmp_path / "mesh_binary_search.ply")
    colors = (m["vertex_colors"].clamp(0, 1) * 255).round().to(torch.uint8)
    f3d.ply.save_mesh_ply(p, m["vertices_filtered"], m["faces_filtered"], colors)
    v, f, c = f3d.ply.read_mesh_ply(p)
    assert np.array_equal(v, m["vertices_filtered"].cpu().numpy()) and np.array_equal(c, colors.cpu().numpy())
