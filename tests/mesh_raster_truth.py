"""The mesh rasteriser of include/f3dg.h (f3dg_mesh_raster) restated in float64 numpy, in the definition's operation order, plus an
independent route that pins the restatement (coverage by the three integer edge tests over ALL pixels with the orientation applied as
a sign instead of a swap; depth and weights by fractions.Fraction), and the meshes the raster tests share. numpy's + - * / and rint on
float64 are IEEE operations, the ones the kernels execute."""
from fractions import Fraction

import numpy as np

CULL = {"none": 0, "back": 1, "front": 2}
GUARD = 16384.0
SMALL, WAVE = 64, 512               # centres of a box one thread walks / one wave walks
COUNT_NAMES = ("rasterised", "near", "guard", "degenerate", "culled", "large", "covered")
EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)


def focal(fov_degrees, H, W):
    """fx, fy as TSDFVolume.integrate forms them."""
    import math
    FoV = float(fov_degrees) * math.pi / 180
    return W / (2 * math.tan(FoV / 2.)), H / (2 * math.tan(FoV / 2.))


def project(vertices, m, fx, fy, H, W):
    """All vertices under one world_view m [4,4] (row-vector convention): x, y, z, u, v in float64, the definition's order."""
    P = np.asarray(vertices, np.float32).astype(np.float64)
    m = np.asarray(m, np.float32).astype(np.float64)
    X, Y, Z = P[:, 0], P[:, 1], P[:, 2]
    with np.errstate(all="ignore"):
        x = ((X * m[0, 0] + Y * m[1, 0]) + Z * m[2, 0]) + m[3, 0]
        y = ((X * m[0, 1] + Y * m[1, 1]) + Z * m[2, 1]) + m[3, 1]
        z = ((X * m[0, 2] + Y * m[1, 2]) + Z * m[2, 2]) + m[3, 2]
        u = ((np.float64(fx) * x) / z + np.float64(W) / 2.0) - 0.5
        v = ((np.float64(fy) * y) / z + np.float64(H) / 2.0) - 0.5
    return x, y, z, u, v


def classify(ids, x, y, z, u, v, z_near, cull):
    """The class of one pair ("rasterised", "near", "guard", "degenerate", "culled") and, when rasterised, (U [3], V [3], area)."""
    a, b, c = (int(i) for i in ids)
    if a == b or b == c or a == c:
        return "degenerate", None
    k = [a, b, c]
    fin = np.isfinite
    if any(not (fin(x[i]) and fin(y[i]) and fin(z[i]) and z[i] > z_near and fin(u[i]) and fin(v[i])) for i in k):
        return "near", None
    if any(not (abs(u[i]) <= GUARD and abs(v[i]) <= GUARD) for i in k):
        return "guard", None
    U = [int(np.rint(256.0 * u[i])) for i in k]
    V = [int(np.rint(256.0 * v[i])) for i in k]
    area = (U[1] - U[0]) * (V[2] - V[0]) - (V[1] - V[0]) * (U[2] - U[0])
    if area == 0:
        return "degenerate", None
    if (cull == "back" and area > 0) or (cull == "front" and area < 0):
        return "culled", None
    return "rasterised", (U, V, area)


def box_of(U, V, H, W):
    """(i0, i1, j0, j1) of the pixel centres inside the snapped corners' box, cut to the image; empty when i1 < i0 or j1 < j0."""
    i0, i1 = max(-((-min(U)) // 256), 0), min(max(U) // 256, W - 1)
    j0, j1 = max(-((-min(V)) // 256), 0), min(max(V) // 256, H - 1)
    return i0, i1, j0, j1


def edge_values(U, V, area, ii, jj):
    """For pixel centres (ii, jj) (int64 arrays): the coverage mask and the edge values w [3] opposite the face's OWN corners, after the
    swap of corners 1 and 2 where area < 0 -- the definition's route."""
    o = (0, 2, 1) if area < 0 else (0, 1, 2)
    Px, Py = 256 * ii.astype(np.int64), 256 * jj.astype(np.int64)
    E, inside = [], np.ones(ii.shape, bool)
    for e in range(3):
        a, b = o[e], o[(e + 1) % 3]
        du, dv = U[b] - U[a], V[b] - V[a]
        Ee = du * (Py - V[a]) - dv * (Px - U[a])
        inside &= (Ee > 0) | ((Ee == 0) & bool(dv > 0 or (dv == 0 and du < 0)))
        E.append(Ee)
    w = [None] * 3
    w[o[0]], w[o[1]], w[o[2]] = E[1], E[2], E[0]          # oriented corner 0 / 1 / 2 is opposite edge 1 / 2 / 0
    return inside, w


def weights(w, area, zc):
    """float64 D-normalised weights beta [3] and depth 1 / D of the definition, BEFORE the rounding to float32."""
    absA = np.float64(abs(area))
    q = [np.float64(1.0) / np.float64(zk) for zk in zc]
    t = [(w[k].astype(np.float64) / absA) * q[k] for k in range(3)]
    D = (t[0] + t[1]) + t[2]
    return [t[k] / D for k in range(3)], np.float64(1.0) / D


def raster(vertices, faces, world_views, fx, fy, H, W, z_near=0.01, cull="none", attrs=None, keep64=False):
    """The whole call. Returns a dict: face_id [V,H,W] int32, depth [V,H,W] float32, bary [V,3,H,W] float32, attrs_out [V,C,H,W] float32 or
    None, counts (list of 7, h_counts' order), boxes (centres of every rasterised pair's box, in pair order), and with keep64 the
    float64 depth64 / beta64 before rounding. An id out of range raises ValueError."""
    P = np.asarray(vertices, np.float32)
    faces = np.asarray(faces).reshape(-1, 3).astype(np.int64)
    wv = np.asarray(world_views, np.float32).reshape(-1, 4, 4)
    N, F, NV = len(P), len(faces), len(wv)
    if F and (faces.min() < 0 or faces.max() >= N):
        raise ValueError("an id outside [0, N)")
    A = None if attrs is None else np.asarray(attrs, np.float32).astype(np.float64)
    keys = np.full((NV, H, W), EMPTY, np.uint64)
    bary = np.zeros((NV, 3, H, W), np.float32)
    out = None if A is None else np.zeros((NV, A.shape[1], H, W), np.float32)
    d64, b64 = np.zeros((NV, H, W)), np.zeros((NV, 3, H, W))
    n = dict.fromkeys(COUNT_NAMES, 0)
    boxes = []
    for view in range(NV):
        x, y, z, u, v = project(P, wv[view], fx, fy, H, W)
        for f in range(F):
            cls, tri = classify(faces[f], x, y, z, u, v, z_near, cull)
            n[cls] += 1
            if tri is None:
                continue
            U, V, area = tri
            i0, i1, j0, j1 = box_of(U, V, H, W)
            size = 0 if (i1 < i0 or j1 < j0) else (i1 - i0 + 1) * (j1 - j0 + 1)
            boxes.append(size)
            n["large"] += size > SMALL
            if size == 0:
                continue
            jj, ii = np.meshgrid(np.arange(j0, j1 + 1), np.arange(i0, i1 + 1), indexing="ij")
            inside, w = edge_values(U, V, area, ii, jj)
            if not inside.any():
                continue
            with np.errstate(all="ignore"):
                beta, depth = weights(w, area, z[faces[f]])
            d32 = depth.astype(np.float32)
            key = (d32.view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.uint64(f)
            sub = keys[view, j0:j1 + 1, i0:i1 + 1]
            win = inside & (key < sub)
            sub[win] = key[win]
            for k in range(3):
                bary[view, k, j0:j1 + 1, i0:i1 + 1][win] = beta[k].astype(np.float32)[win]
                b64[view, k, j0:j1 + 1, i0:i1 + 1][win] = beta[k][win]
            d64[view, j0:j1 + 1, i0:i1 + 1][win] = depth[win]
            if A is not None:
                a = A[faces[f]]
                for c in range(A.shape[1]):
                    val = ((a[0, c] * beta[0] + a[1, c] * beta[1]) + a[2, c] * beta[2]).astype(np.float32)
                    out[view, c, j0:j1 + 1, i0:i1 + 1][win] = val[win]
    hit = keys != EMPTY
    face_id = np.where(hit, (keys & np.uint64(0xFFFFFFFF)).astype(np.int64), -1).astype(np.int32)
    depth = np.where(hit, (keys >> np.uint64(32)).astype(np.uint32), 0).astype(np.uint32).view(np.float32)
    n["covered"] = int(hit.sum())
    r = {"face_id": face_id, "depth": depth, "bary": bary, "attrs_out": out, "counts": [int(n[k]) for k in COUNT_NAMES], "boxes": boxes}
    if keep64:
        r.update(depth64=d64, beta64=b64)
    return r


# ------------------------------------------------------------------------------------------------ the independent route
def cover_all_pixels(U, V, H, W):
    """Coverage of one snapped triangle over ALL pixels of the image, with the orientation applied as a sign to the face's own edges
    0 -> 1, 1 -> 2, 2 -> 0 instead of a swap: [H,W] bool, and the signed edge values s E [3] (s E_e is opposite own corner (e + 2) % 3)."""
    area = (U[1] - U[0]) * (V[2] - V[0]) - (V[1] - V[0]) * (U[2] - U[0])
    if area == 0:
        return np.zeros((H, W), bool), None
    s = 1 if area > 0 else -1
    Py, Px = np.meshgrid(256 * np.arange(H, dtype=np.int64), 256 * np.arange(W, dtype=np.int64), indexing="ij")
    inside, sE = np.ones((H, W), bool), []
    for e in range(3):
        a, b = e, (e + 1) % 3
        du, dv = s * (U[b] - U[a]), s * (V[b] - V[a])               # the edge as the oriented triangle runs it
        Ee = du * (Py - V[a]) - dv * (Px - U[a])
        inside &= (Ee > 0) | ((Ee == 0) & bool(dv > 0 or (dv == 0 and du < 0)))
        sE.append(Ee)
    return inside, sE


def exact_pixel(U, V, zc, i, j):
    """fractions.Fraction on the snapped integers and the float64 z: (depth, beta [3]) of pixel (i, j), exactly."""
    area = (U[1] - U[0]) * (V[2] - V[0]) - (V[1] - V[0]) * (U[2] - U[0])
    Px, Py = 256 * i, 256 * j
    w = []
    for k in range(3):                                            # the sub-triangle opposite corner k, over the whole
        a, b = (k + 1) % 3, (k + 2) % 3
        w.append(Fraction((U[b] - U[a]) * (Py - V[a]) - (V[b] - V[a]) * (Px - U[a]), area))
    q = [1 / Fraction(float(zk)) for zk in zc]
    D = sum(w[k] * q[k] for k in range(3))
    return 1 / D, [w[k] * q[k] / D for k in range(3)]


def ulp64_apart(x, exact):
    """|x - exact| in units of the last place of float64 x."""
    x = float(x)
    return float(abs(Fraction(x) - exact) / Fraction(np.spacing(abs(x)) if x else np.spacing(0.0)))


# ------------------------------------------------------------------------------------------------ the shared meshes
def jittered_grid(nx, ny, seed, spacing=5):
    """A grid of nx x ny quads whose corners sit on the HALF-PIXEL lattice: spacing pixels apart, every inner corner moved by up to one
    pixel in steps of half a pixel (a quad of side >= 3 px whose corners move by <= 1 px stays convex, so either diagonal splits it into
    two proper triangles), the outline fixed on a rectangle whose sides pass half-way between pixel centres. Random diagonals and random
    windings. Returns (U, V) int arrays in 1/256 px, faces [2 nx ny, 3], and the pixel rectangle (i0, i1, j0, j1) of the interior centres."""
    rng = np.random.default_rng(seed)
    gx, gy = np.meshgrid(np.arange(nx + 1), np.arange(ny + 1), indexing="xy")
    hx = (2 * spacing * gx + 1).astype(np.int64)                   # half pixels: the outline at 0.5, 0.5 + spacing nx
    hy = (2 * spacing * gy + 1).astype(np.int64)
    inner = (gx > 0) & (gx < nx) & (gy > 0) & (gy < ny)
    hx = hx + np.where(inner, rng.integers(-2, 3, gx.shape), 0)
    hy = hy + np.where(inner, rng.integers(-2, 3, gx.shape), 0)
    idx = lambda ix, iy: iy * (nx + 1) + ix
    faces = []
    for iy in range(ny):
        for ix in range(nx):
            a, b, c, d = idx(ix, iy), idx(ix + 1, iy), idx(ix + 1, iy + 1), idx(ix, iy + 1)
            for t in ([(a, b, c), (a, c, d)] if rng.integers(2) else [(a, b, d), (b, c, d)]):
                faces.append(t if rng.integers(2) else (t[0], t[2], t[1]))
    return 128 * hx.reshape(-1), 128 * hy.reshape(-1), np.array(faces, np.int64), (1, spacing * nx, 1, spacing * ny)


def lattice_to_world(U, V, H, W, fx, Z):
    """Vertices on the plane z = Z of an identity camera that project EXACTLY onto the snapped coordinates (U, V): fx = fy a power of
    two, Z a power of two, U and V multiples of 128 (every product and quotient is exact in float32 and float64)."""
    X = (U / 256.0 - (W / 2.0 - 0.5)) * Z / fx
    Y = (V / 256.0 - (H / 2.0 - 0.5)) * Z / fx
    P = np.stack([X, Y, np.full(len(U), float(Z))], axis=1).astype(np.float32)
    assert np.array_equal(P.astype(np.float64)[:, 0], X) and np.array_equal(P.astype(np.float64)[:, 1], Y)
    return P


def identity_view():
    return np.eye(4, dtype=np.float32)[None]


def plane_grid(nx, ny, centre, half, seed=None):
    """(nx + 1) x (ny + 1) vertices on the plane z = centre[2] (``seed``: each moved along z by up to 0.05), nx x ny quads of two
    triangles, all of one winding."""
    gx, gy = np.meshgrid(np.linspace(-half, half, nx + 1), np.linspace(-half, half, ny + 1), indexing="xy")
    P = np.stack([gx.reshape(-1) + centre[0], gy.reshape(-1) + centre[1], np.full(gx.size, centre[2])], axis=1).astype(np.float32)
    if seed is not None:
        P[:, 2] += np.random.default_rng(seed).uniform(-0.05, 0.05, len(P)).astype(np.float32)
    idx = lambda ix, iy: iy * (nx + 1) + ix
    faces = []
    for iy in range(ny):
        for ix in range(nx):
            a, b, c, d = idx(ix, iy), idx(ix + 1, iy), idx(ix + 1, iy + 1), idx(ix, iy + 1)
            faces += [(a, b, c), (a, c, d)]
    return P, np.array(faces, np.int64)


def big_and_small(centre, seed=3):
    """Two triangles that fill the frame of a camera at the origin looking down +z at ``centre``, BEHIND 20 triangles of assorted sizes:
    boxes on both sides of the one-thread limit and of the wave limit."""
    rng = np.random.default_rng(seed)
    cx, cy, cz = centre
    P = [(cx - 9, cy - 9, cz + 1), (cx + 9, cy - 9, cz + 1), (cx + 9, cy + 9, cz + 1), (cx - 9, cy + 9, cz + 1.5)]
    faces = [(0, 1, 2), (0, 2, 3)]
    for k in range(20):
        size = (0.1, 0.5, 1.2, 2.5)[k % 4]
        c = np.array([cx + rng.uniform(-2.5, 2.5), cy + rng.uniform(-2.5, 2.5), cz + rng.uniform(-0.3, 0.3)])
        tri = c + rng.uniform(-size, size, (3, 3)) * np.array([1, 1, 0.2])
        faces.append((len(P), len(P) + 1, len(P) + 2))
        P += [tuple(t) for t in tri]
    return np.array(P, np.float32), np.array(faces, np.int64)
