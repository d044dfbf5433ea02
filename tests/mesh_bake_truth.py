"""The vertex colour baking of include/f3dg.h (f3dg_mesh_bake_colors) restated in float64 numpy, in the definition's operation order: one
view at a time over all vertices, the views in ascending order, so that every vertex's sums are formed in the order the definition
fixes. face_id and depth come from mesh_raster_truth.raster (or from the rasteriser itself: they are inputs here). numpy's + - * /,
rint and floor on float64 are IEEE operations, the ones the kernel executes. The scenes the baking tests share follow."""
import numpy as np

import mesh_raster_truth as rt

CLASSES = ("near", "outside", "uncovered", "occluded", "grazing", "masked", "used")
COUNT_NAMES = CLASSES + ("vertices_seen",)
NEAR, OUTSIDE, UNCOVERED, OCCLUDED, GRAZING, MASKED, USED = range(7)
MODES = {"blend": 0, "best": 1}


def classify_view(P, normals, m, fx, fy, H, W, image, face_id, depth, alpha, alpha_min, depth_tol, cm2, z_near):
    """All vertices under ONE view: (cls [N] int, w [N] float64, s [N,C] float64); w and s mean something where cls == USED."""
    N, C = len(P), image.shape[0]
    m64 = np.asarray(m, np.float32).astype(np.float64)
    cls = np.full(N, -1, np.int64)
    w, s = np.ones(N), np.zeros((N, C))
    with np.errstate(all="ignore"):
        x, y, z, u, v = rt.project(P, m, fx, fy, H, W)
        fin = np.isfinite
        near = ~(fin(x) & fin(y) & fin(z) & fin(u) & fin(v) & (z > z_near))
        cls[near] = NEAR
        outside = (cls < 0) & ~((0.0 <= u) & (u <= np.float64(W - 1)) & (0.0 <= v) & (v <= np.float64(H - 1)))
        cls[outside] = OUTSIDE
        live = cls < 0
        us, vs = np.where(live, u, 0.0), np.where(live, v, 0.0)            # inside the image from here on
        i, j = np.rint(us).astype(np.int64), np.rint(vs).astype(np.int64)  # ties to even
        cls[live & (face_id[j, i] < 0)] = UNCOVERED
        live = cls < 0
        cls[live & ~(z - depth[j, i].astype(np.float64) <= np.float64(depth_tol))] = OCCLUDED
        live = cls < 0
        if normals is not None:
            n = np.asarray(normals, np.float32).astype(np.float64)
            nx, ny, nz = n[:, 0], n[:, 1], n[:, 2]
            nc = [(nx * m64[0, c] + ny * m64[1, c]) + nz * m64[2, c] for c in range(3)]
            g = -((nc[0] * x + nc[1] * y) + nc[2] * z)
            nn = (nc[0] * nc[0] + nc[1] * nc[1]) + nc[2] * nc[2]
            pp = (x * x + y * y) + z * z
            grazing = ~fin(nn) | ~(nn > 0.0) | ~(g > 0.0) | ~(g * g >= cm2 * (nn * pp))
            cls[live & grazing] = GRAZING
            w = (g * g) / (nn * pp)
            live = cls < 0
        i0, j0 = np.floor(us).astype(np.int64), np.floor(vs).astype(np.int64)
        i1, j1 = np.minimum(i0 + 1, W - 1), np.minimum(j0 + 1, H - 1)
        ok = np.ones(N, bool)
        if alpha is not None:
            for jj, ii in ((j0, i0), (j0, i1), (j1, i0), (j1, i1)):
                ok &= alpha[jj, ii].astype(np.float64) >= np.float64(alpha_min)
        a, b = us - i0.astype(np.float64), vs - j0.astype(np.float64)
        for c in range(C):
            img = image[c].astype(np.float64)
            c00, c10, c01, c11 = img[j0, i0], img[j0, i1], img[j1, i0], img[j1, i1]
            ok &= fin(c00) & fin(c10) & fin(c01) & fin(c11)
            top = c00 + a * (c10 - c00)
            bot = c01 + a * (c11 - c01)
            s[:, c] = top + b * (bot - top)
        cls[live & ~ok] = MASKED
        cls[cls < 0] = USED
    return cls, w, s


def bake(vertices, normals, world_views, fx, fy, images, face_id, depth, alpha=None, alpha_min=0.5, depth_tol=0.0, cos_min=0.1, mode="blend",
         z_near=0.01):
    """The whole call. Returns a dict: colors [N,C] float32, weight [N] float32, n_used [N] int32, best_view [N] int32, counts (list of 8,
    h_counts' order), and the per-pair cls [V,N], w [V,N] and s [V,N,C] in float64."""
    P = np.asarray(vertices, np.float32)
    wv = np.asarray(world_views, np.float32).reshape(-1, 4, 4)
    images = np.asarray(images, np.float32)
    V, C, H, W = images.shape
    N = len(P)
    assert len(wv) == V and face_id.shape == (V, H, W) and depth.shape == (V, H, W) and mode in MODES
    cm2 = np.float64(cos_min) * np.float64(cos_min)
    Sw, bw, acc = np.zeros(N), np.zeros(N), np.zeros((N, C))
    n_used, best_view = np.zeros(N, np.int32), np.full(N, -1, np.int32)
    all_cls, all_w, all_s = np.zeros((V, N), np.int64), np.zeros((V, N)), np.zeros((V, N, C))
    for view in range(V):                                                   # ascending: the order of every vertex's sums
        cls, w, s = classify_view(P, normals, wv[view], fx, fy, H, W, images[view], face_id[view], depth[view],
                                  None if alpha is None else np.asarray(alpha, np.float32)[view], alpha_min, depth_tol, cm2, z_near)
        used = cls == USED
        with np.errstate(all="ignore"):
            better = used & ((n_used == 0) | (w > bw))                      # the first used sample, then only a strictly larger w
            bw = np.where(better, w, bw)
            best_view = np.where(better, view, best_view).astype(np.int32)
            if mode == "blend":
                Sw = np.where(used, Sw + w, Sw)
                acc = np.where(used[:, None], acc + w[:, None] * s, acc)
            else:
                acc = np.where(better[:, None], s, acc)
        n_used = n_used + used.astype(np.int32)
        all_cls[view], all_w[view], all_s[view] = cls, w, s
    seen = n_used > 0
    with np.errstate(all="ignore"):
        colors = (acc / Sw[:, None]) if mode == "blend" else acc
        weight = Sw if mode == "blend" else bw
    colors = np.where(seen[:, None], colors, 0.0).astype(np.float32)
    weight = np.where(seen, weight, 0.0).astype(np.float32)
    counts = [int((all_cls == k).sum()) for k in range(7)] + [int(seen.sum())]
    return {"colors": colors, "weight": weight, "n_used": n_used, "best_view": best_view, "counts": counts, "cls": all_cls, "w": all_w, "s": all_s}


def bake_mesh(vertices, faces, normals, world_views, fx, fy, images, z_near=0.01, cull="none", **kw):
    """raster (mesh_raster_truth) then bake: what bake_vertex_colors does without a reused visibility. Returns (bake dict, raster dict)."""
    V, C, H, W = np.asarray(images).shape
    r = rt.raster(vertices, faces, world_views, fx, fy, H, W, z_near=z_near, cull=cull)
    return bake(vertices, normals, world_views, fx, fy, images, r["face_id"], r["depth"], z_near=z_near, **kw), r


# ------------------------------------------------------------------------------------------------ the shared scenes
FX, Z = 16.0, 4.0                   # powers of two: lattice_to_world is exact


def dyadic_image(V, C, H, W, seed):
    """Random multiples of 1/256 in [0, 1): sums and means of a few of them are exact in float64 and float32."""
    return (np.random.default_rng(seed).integers(0, 256, (V, C, H, W)) / 256.0).astype(np.float32)


def lattice_grid(us, vs, H, W, Zp, fx=FX):
    """A fronto-parallel grid under identity_view() whose vertices project EXACTLY onto the lattice points (us[k], vs[l]) (1/256 px,
    multiples of 128), two triangles per cell, row-major vertices (index l * len(us) + k). Returns (P [n,3] float32, faces int64)."""
    gu, gv = np.meshgrid(np.asarray(us), np.asarray(vs), indexing="xy")
    P = rt.lattice_to_world(gu.reshape(-1), gv.reshape(-1), H, W, fx, Zp)
    n = len(us)
    faces = []
    for l in range(len(vs) - 1):
        for k in range(n - 1):
            a, b, c, d = l * n + k, l * n + k + 1, (l + 1) * n + k + 1, (l + 1) * n + k
            faces += [(a, b, c), (a, c, d)]
    return P, np.array(faces, np.int64).reshape(-1, 3)


def pixel_plane(H, W, shift=0, Zp=Z):
    """The plane of the exact-sample tests: vertices on u = i + shift / 256 for i = 1 .. W - 2 (rows likewise), inside an outline half a
    pixel further out (u = 0.5 + shift / 256 and W - 1.5 + shift / 256), so that the pixel nearest to every INNER vertex is strictly
    inside the mesh and covered whatever the tie rule of the outline. shift = 0: the inner vertices sit on pixel centres; shift = 128: in
    the middle of four. Returns (P, faces, inner [n] bool, (iu [n], iv [n]): floor(u), floor(v) of every vertex)."""
    us = np.array([128] + [256 * i for i in range(1, W - 1)] + [256 * (W - 1) - 128]) + shift
    vs = np.array([128] + [256 * j for j in range(1, H - 1)] + [256 * (H - 1) - 128]) + shift
    P, faces = lattice_grid(us, vs, H, W, Zp)
    gu, gv = np.meshgrid(us, vs, indexing="xy")
    ku, kv = np.meshgrid(np.arange(len(us)), np.arange(len(vs)), indexing="xy")
    inner = ((ku > 0) & (ku < len(us) - 1) & (kv > 0) & (kv < len(vs) - 1)).reshape(-1)
    return P, faces, inner, (gu.reshape(-1) // 256, gv.reshape(-1) // 256)


def two_planes_scene():
    """The class-count scene: H x W = 8 x 8 under identity_view(), fx = fy = 16, depth_tol = 0.5, z_near = 0.01, no normals, no alpha.
      front   one quad at z = 4 with corners at u, v in {1.5, 4.5}: it covers the pixel centres 2 .. 4 squared. Its 4 vertices round
              (ties to even) to the pixels (2 | 4, 2 | 4), which it covers itself at its own depth: 4 USED.
      back    a grid at z = 8 on u, v in {0.5, 1, 2, 3, 4, 5, 5.5} (49 vertices, 72 faces): it covers the centres 1 .. 5 squared.
              Of the 25 vertices on pixel centres, the 9 on 2 .. 4 squared lie behind the front quad (z - depth = 4 > 0.5): OCCLUDED;
              the 16 past its silhouette: USED. The 24 outline vertices round to row / column 0 or 6, which nothing covers: UNCOVERED.
      sliver  a face at z = 4 inside the cell between the pixel centres 6 and 7: it wins no centre, and the pixels its three vertices
              round to, (6, 6), (7, 6) and (6, 7), are empty: 3 UNCOVERED.
      off     2 vertices without a face that project off the image (u = -1 and u = 8): OUTSIDE.
      bad     a vertex at z = 0.01 (= z_near, not beyond it) and a NaN vertex: NEAR.
    Returns (P, faces, the hand-written counts [8])."""
    H = W = 8
    Pf, Ff = lattice_grid([384, 1152], [384, 1152], H, W, 4.0)
    back = [128, 256, 512, 768, 1024, 1280, 1408]
    Pb, Fb = lattice_grid(back, back, H, W, 8.0)
    sliver = rt.lattice_to_world(np.array([1664, 1792, 1664]), np.array([1664, 1664, 1792]), H, W, FX, 4.0)
    off = rt.lattice_to_world(np.array([-256, 8 * 256]), np.array([3 * 256, 3 * 256]), H, W, FX, 4.0)
    bad = np.array([[0.0, 0.0, 0.01], [np.nan, 0.0, 4.0]], np.float32)
    P = np.concatenate([Pf, Pb, sliver, off, bad]).astype(np.float32)
    n0 = len(Pf) + len(Pb)
    faces = np.concatenate([Ff, Fb + len(Pf), np.array([[n0, n0 + 1, n0 + 2]], np.int64)])
    #          near outside uncovered occluded grazing masked used seen
    expected = [2, 2, 24 + 3, 9, 0, 0, 4 + 16, 4 + 16]
    return P, faces, expected


CENTRE = np.array([0.0, 0.0, 7.667])           # what the orbit cameras of f3dgaus_amd.synthetic look at


def orbit(n, H, W):
    """(world_views [n,4,4] float32, fx, fy) of the n-view orbit at H x W."""
    from f3dgaus_amd import synthetic
    cams = synthetic.orbit_cameras(n, resolution=32)
    fx, fy = rt.focal(float(cams["cfg"]["model"]["fov"]), H, W)
    return cams["viewmatrix"].numpy().astype(np.float32), fx, fy


def sphere_scene(level, n_views, H, W, C, seed, radius=0.5):
    """A noisy icosphere at the orbit's centre with its area-weighted normals, random images with four NaN pixels, and an alpha plane
    that masks the left third of every image. Returns a dict of numpy arrays."""
    import mesh_smooth_truth as st
    P, faces = st.icosphere(level, noise=0.02, seed=seed)
    P = (P * radius + CENTRE).astype(np.float32)
    faces = np.asarray(faces, np.int64)
    normals = st.normals(P, faces, len(P))
    wv, fx, fy = orbit(n_views, H, W)
    rng = np.random.default_rng(seed + 100)
    images = rng.uniform(0, 1, (n_views, C, H, W)).astype(np.float32)
    images[:, 0, H // 2:H // 2 + 2, W // 2:W // 2 + 2] = np.nan
    alpha = np.ones((n_views, H, W), np.float32)
    alpha[:, :, :W // 2 - 2] = 0.25
    return {"P": P, "faces": faces, "normals": normals, "wv": wv, "fx": fx, "fy": fy, "images": images, "alpha": alpha}


def probe_scene(tx=(0.0, 4.0)):
    """One probe vertex (index 4, no face of its own) at (0, 0, 4) on a quad at z = 4 that fills the view, seen by len(tx) cameras that
    differ by a shift of tx[k] along x; H x W = 8 x 16, fx = fy = 4. Under shift t the probe sits at camera (t, 0, 4): u = 7.5 + t,
    v = 3.5 (the middle of four pixels) and, with the normal (0, 0, -1), g = 4, nn = 1, pp = t t + 16: w = 16 / (t t + 16), which is 1
    for t = 0 and 1/2 for t = 4. Returns (P, faces, normals, world_views, fx, H, W)."""
    P = np.array([[-7, -3, 4], [7, -3, 4], [7, 3, 4], [-7, 3, 4], [0, 0, 4]], np.float32)
    faces = np.array([[0, 1, 2], [0, 2, 3]], np.int64)
    normals = np.tile(np.array([[0, 0, -1]], np.float32), (5, 1))
    wv = np.tile(np.eye(4, dtype=np.float32), (len(tx), 1, 1))
    wv[:, 3, 0] = tx
    return P, faces, normals, wv, 4.0, 8, 16
