"""Truth for the TSDF mesh route (f3dg_tsdf_integrate / _cells_count / _cells_emit / _vertices, f3dgaus_amd.tsdf): a numpy restatement of
the definition in include/f3dg.h in float64, with a float32 mode for E_ref, the fixtures the tests share, the fragile-voxel rule and mesh
checks. The reference holds no TSDF code: this restatement IS the definition's second statement, not a port.

Definition (voxel (x, y, z), id (z ny + y) nx + x, centre p = origin + voxel (x, y, z); per view v, everything in ``dtype`` on the float32
inputs):
    camera    (X, Y, Z) = p wv[:3,:3] + wv[3,:3];  live iff Z > z_near
    pixel     u = fx X / Z + W/2, w = fy Y / Z + H/2;  live iff 0 <= u < W and 0 <= w < H (as floats; NaN fails);  i = floor(u), j = floor(w)
    depth     d = depth[v,j,i];  live iff d finite and d > 0, and alpha[v,j,i] >= alpha_min when alpha is given
    sample    sdf = d - Z;  dropped iff sdf < -trunc;  t = min(1, sdf / trunc);  a colour sample iff |sdf| <= trunc
    call      S = sum t, n = count, Cs = sum colour, nc = count over the views in ascending order;
              tsdf <- (tsdf weight + S) / (weight + n), weight <- weight + n where n > 0;  color / color_weight likewise with Cs, nc
    cells     cell (x, y, z) (id (z (ny-1) + y)(nx-1) + x) is active iff its eight corners have weight >= min_weight and a finite tsdf and
              do not all agree on tsdf < 0;  six Kuhn tetrahedra per active cell, the axis orders in lexicographic order (xyz, xzy, yxz,
              yzx, zxy, zyx), the two middle vertices of the even orders swapped: (v0 - v3) . ((v1 - v3) x (v2 - v3)) > 0 for all six
    vertices  edge (lo, hi): o = the end with tsdf < 0 (lo if both), f = the other;  w = t_f / (t_f - t_o) where that divisor is > 0, else 0;
              vertex = p_f + (p_o - p_f) w;  colour likewise where both ends have color_weight > 0, the one that has otherwise, else 0

Fragile voxels. The definition is discontinuous where the floor, Z > z_near or a band test flips. A voxel is fragile if for any view
fx X / Z + W/2 or its y twin lies within MARGIN (1e-4) of an integer (for a sample with Z > 0 that lands within one pixel of the image),
|Z - z_near| < MARGIN, or, for a sample that reads a live pixel, |sdf + trunc| < MARGIN trunc or ||sdf| - trunc| < MARGIN trunc. At most
FRAGILE_CAP (1 %) of a case's observed voxels may be fragile (``fragile`` asserts nothing; the tests do).

Tolerance. Outside the fragile set a kernel's weight and color_weight are exact, and tsdf weight and color color_weight lie within
4 E_ref + 1e-6 max|.| of the float64 restatement: E_ref the float32 restatement's own error on that case and quantity (DESIGN.md section 4:
measured, not chosen, margin 4)."""
import itertools

import numpy as np

MARGIN = 1e-4
FRAGILE_CAP = 0.01
Z_NEAR = 0.05
ALPHA_MIN = 0.5

# the six axis orders of the Kuhn split and the corner offsets (dx, dy, dz) of their four vertices
KUHN_ORDERS = list(itertools.permutations(range(3)))


def _odd(perm):
    return sum(1 for a in range(3) for b in range(a + 1, 3) if perm[a] > perm[b]) % 2 == 1


def kuhn_corners():
    """[6,4,3] int: the corner offsets of the six tetrahedra, in the header's order."""
    out = []
    for perm in KUHN_ORDERS:
        c = np.zeros(3, dtype=np.int64)
        path = [c.copy()]
        for axis in perm:
            c[axis] += 1
            path.append(c.copy())
        if not _odd(perm):
            path[1], path[2] = path[2], path[1]
        out.append(np.stack(path))
    return np.stack(out)


def look_at(eye, target, up=(0.0, 1.0, 0.0)):
    """world_view [4,4] float64, row-vector convention (p_cam = [p_world, 1] @ world_view), +z forward."""
    eye, target = np.asarray(eye, dtype=np.float64), np.asarray(target, dtype=np.float64)
    fwd = target - eye
    fwd = fwd / np.linalg.norm(fwd)
    right = np.cross(np.asarray(up, dtype=np.float64), fwd)
    right = right / np.linalg.norm(right)
    upv = np.cross(fwd, right)
    m = np.eye(4)
    m[:3, 0], m[:3, 1], m[:3, 2] = right, upv, fwd
    m[3, :3] = -(eye @ m[:3, :3])
    return m


def sphere_depth(world_view, spheres, H, W, fx, fy):
    """Analytic z-depth [H,W] float32 of the nearest of ``spheres`` ((centre, radius), world space) along the ray through every pixel
    centre; 0 where the ray hits nothing."""
    jj, ii = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    d = np.stack([(ii + 0.5 - W / 2.0) / fx, (jj + 0.5 - H / 2.0) / fy, np.ones_like(ii)], -1)       # camera point = t d, z-depth = t
    best = np.full((H, W), np.inf)
    for centre, radius in spheres:
        c = np.append(np.asarray(centre, dtype=np.float64), 1.0) @ world_view[:, :3]
        a, b, cc = (d * d).sum(-1), (d * c).sum(-1), (c * c).sum() - radius * radius
        disc = b * b - a * cc
        with np.errstate(invalid="ignore"):
            t = (b - np.sqrt(disc)) / a
        hit = (disc > 0) & (t > 0)
        best = np.where(hit & (t < best), t, best)
    return np.where(np.isfinite(best), best, 0.0).astype(np.float32)


def facing_ratio(world_view, centre, radius, depth, fx, fy):
    """[H,W] float32: the cosine between a sphere's normal at the point a pixel sees (``depth`` from ``sphere_depth``) and the ray back to
    the camera; 0 where the pixel sees nothing."""
    H, W = depth.shape
    jj, ii = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    d = np.stack([(ii + 0.5 - W / 2.0) / fx, (jj + 0.5 - H / 2.0) / fy, np.ones_like(ii)], -1)
    c = np.append(np.asarray(centre, dtype=np.float64), 1.0) @ world_view[:, :3]
    normal = (d * depth[..., None].astype(np.float64) - c) / radius
    ray = d / np.linalg.norm(d, axis=-1, keepdims=True)
    return np.where(depth > 0, -(normal * ray).sum(-1), 0.0).astype(np.float32)


def empty_state(dims):
    nx, ny, nz = dims
    return {"tsdf": np.zeros((nz, ny, nx), np.float32), "weight": np.zeros((nz, ny, nx), np.float32),
            "color": np.zeros((3, nz, ny, nx), np.float32), "color_weight": np.zeros((nz, ny, nx), np.float32)}


def voxel_centres(origin, voxel, dims, dtype):
    """[N,3] in ``dtype``: origin + voxel (x, y, z) on the float32 origin and voxel, x fastest."""
    nx, ny, nz = dims
    o = np.asarray(origin, dtype=np.float32).astype(dtype)
    s = dtype(np.float32(voxel))
    z, y, x = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    return np.stack([o[0] + s * x.reshape(-1).astype(dtype), o[1] + s * y.reshape(-1).astype(dtype), o[2] + s * z.reshape(-1).astype(dtype)], 1)


def _samples(p, wv, fx, fy, H, W, depth, alpha, trunc, z_near, alpha_min, dtype):
    """One view's samples at the points p [N,3]: dict of X, Y, Z, u, w, the pixel index, `pix_live` (the sample reads a live pixel),
    `live` (it is a sample), `col` (it is a colour sample), sdf and t; all in ``dtype``."""
    T = dtype
    M = wv.astype(np.float32).astype(T)
    with np.errstate(all="ignore"):
        X = p[:, 0] * M[0, 0] + p[:, 1] * M[1, 0] + p[:, 2] * M[2, 0] + M[3, 0]
        Y = p[:, 0] * M[0, 1] + p[:, 1] * M[1, 1] + p[:, 2] * M[2, 1] + M[3, 1]
        Z = p[:, 0] * M[0, 2] + p[:, 1] * M[1, 2] + p[:, 2] * M[2, 2] + M[3, 2]
        front = Z > T(z_near)
        Zs = np.where(front, Z, T(1))
        u = T(fx) * X / Zs + T(W / 2.0)
        w = T(fy) * Y / Zs + T(H / 2.0)
        inside = front & (u >= 0) & (u < W) & (w >= 0) & (w < H)
        i = np.where(inside, np.floor(np.where(inside, u, 0)), 0).astype(np.int64)
        j = np.where(inside, np.floor(np.where(inside, w, 0)), 0).astype(np.int64)
        pix = j * W + i
        d = depth.reshape(-1)[pix]
        pix_live = inside & np.isfinite(d) & (d > 0)
        if alpha is not None:
            pix_live &= alpha.reshape(-1)[pix] >= np.float32(alpha_min)          # (NaN fails)
        ds = np.where(pix_live, d, np.float32(1)).astype(T)
        sdf = ds - Z
        live = pix_live & ~(sdf < -T(trunc))
        t = np.minimum(T(1), sdf / T(trunc))
        col = live & (np.abs(sdf) <= T(trunc))
    return {"X": X, "Y": Y, "Z": Z, "u": u, "w": w, "front": front, "pix": pix, "pix_live": pix_live, "live": live, "col": col, "sdf": sdf, "t": t}


def integrate(state, origin, voxel, dims, trunc, depth, world_view, fx, fy, color=None, alpha=None, alpha_min=ALPHA_MIN, z_near=Z_NEAR,
              dtype=np.float64):
    """One call of the definition in ``dtype``: returns the new state (arrays in ``dtype``, shaped as the inputs; the input is untouched).
    ``state`` holds float32 arrays or a state this function returned in the same dtype (chained calls stay in ``dtype``)."""
    T = dtype
    nx, ny, nz = dims
    N = nx * ny * nz
    V, H, W = depth.shape
    p = voxel_centres(origin, voxel, dims, T)
    S, n = np.zeros(N, T), np.zeros(N, T)
    Cs, nc = np.zeros((3, N), T), np.zeros(N, T)
    for v in range(V):
        s = _samples(p, world_view[v].reshape(4, 4), np.float32(fx), np.float32(fy), H, W, depth[v], None if alpha is None else alpha[v],
                     np.float32(trunc), np.float32(z_near), alpha_min, T)
        S += np.where(s["live"], s["t"], T(0))
        n += s["live"]
        if color is not None:
            c = color[v].reshape(3, -1)[:, s["pix"]]
            Cs += np.where(s["col"][None], np.where(s["col"][None], c, np.float32(0)).astype(T), T(0))
            nc += s["col"]
    out = {}
    w0, t0 = state["weight"].reshape(-1).astype(T), state["tsdf"].reshape(-1).astype(T)
    wn = w0 + n
    seen = (n > 0) & (wn > 0)
    out["tsdf"] = np.where(seen, (t0 * w0 + S) / np.where(seen, wn, T(1)), t0).reshape(nz, ny, nx)
    out["weight"] = np.where(seen, wn, w0).reshape(nz, ny, nx)
    cw0, c0 = state["color_weight"].reshape(-1).astype(T), state["color"].reshape(3, -1).astype(T)
    cwn = cw0 + nc
    cseen = (nc > 0) & (cwn > 0)
    out["color"] = np.where(cseen[None], (c0 * cw0[None] + Cs) / np.where(cseen, cwn, T(1))[None], c0).reshape(3, nz, ny, nx)
    out["color_weight"] = np.where(cseen, cwn, cw0).reshape(nz, ny, nx)
    return out


def fragile(origin, voxel, dims, trunc, depth, world_view, fx, fy, alpha=None, alpha_min=ALPHA_MIN, z_near=Z_NEAR):
    """[nz,ny,nx] bool: the fragile voxels of a call (float64)."""
    nx, ny, nz = dims
    V, H, W = depth.shape
    p = voxel_centres(origin, voxel, dims, np.float64)
    tr = float(np.float32(trunc))
    out = np.zeros(nx * ny * nz, dtype=bool)
    for v in range(V):
        s = _samples(p, world_view[v].reshape(4, 4), np.float32(fx), np.float32(fy), H, W, depth[v], None if alpha is None else alpha[v],
                     np.float32(trunc), np.float32(z_near), alpha_min, np.float64)
        with np.errstate(all="ignore"):
            out |= np.abs(s["Z"] - float(np.float32(z_near))) < MARGIN
            near_image = s["front"] & (s["u"] > -1) & (s["u"] < W + 1) & (s["w"] > -1) & (s["w"] < H + 1)
            out |= near_image & ((np.abs(s["u"] - np.round(s["u"])) < MARGIN) | (np.abs(s["w"] - np.round(s["w"])) < MARGIN))
            out |= s["pix_live"] & ((np.abs(s["sdf"] + tr) < MARGIN * tr) | (np.abs(np.abs(s["sdf"]) - tr) < MARGIN * tr))
    return out.reshape(nz, ny, nx)


def cells_tets(tsdf, weight, min_weight=1.0):
    """(n_active, tets [6 n_active, 4] int32, active [nz-1,ny-1,nx-1] bool) of a volume's float32 tsdf and weight [nz,ny,nx]."""
    nz, ny, nx = tsdf.shape
    with np.errstate(invalid="ignore"):
        ok = (weight >= np.float32(min_weight)) & np.isfinite(tsdf)
        neg = tsdf < 0
    all_ok = np.ones((nz - 1, ny - 1, nx - 1), dtype=bool)
    n_neg = np.zeros((nz - 1, ny - 1, nx - 1), dtype=np.int64)
    for dz, dy, dx in itertools.product((0, 1), repeat=3):
        sl = (slice(dz, nz - 1 + dz), slice(dy, ny - 1 + dy), slice(dx, nx - 1 + dx))
        all_ok &= ok[sl]
        n_neg += neg[sl]
    active = all_ok & (n_neg > 0) & (n_neg < 8)
    cz, cy, cx = np.nonzero(active)                          # C order: ascending cell id
    base = (cz * ny + cy) * nx + cx
    corners = kuhn_corners()                                 # [6,4,3]
    off = corners[..., 0] + corners[..., 1] * nx + corners[..., 2] * nx * ny
    tets = (base[:, None, None] + off[None]).reshape(-1, 4).astype(np.int32)
    return int(active.sum()), tets, active


def vertices(interp_v, tsdf, origin, voxel, dims, color=None, color_weight=None, dtype=np.float64):
    """(vertices [E,3], vertex_colors [E,3] or None) in ``dtype``, in the header's operation order."""
    T = dtype
    nx, ny, nz = dims
    t = tsdf.reshape(-1).astype(np.float32)
    lo, hi = interp_v[:, 0], interp_v[:, 1]
    with np.errstate(invalid="ignore"):
        lo_occ = t[lo] < 0
    f, o = np.where(lo_occ, hi, lo), np.where(lo_occ, lo, hi)
    tf, to = t[f].astype(T), t[o].astype(T)
    with np.errstate(all="ignore"):
        den = tf - to
        w = np.where(den > 0, tf / np.where(den > 0, den, T(1)), T(0))
    org, s = np.asarray(origin, np.float32).astype(T), T(np.float32(voxel))

    def pos(ids):
        x, y, z = ids % nx, (ids // nx) % ny, ids // (nx * ny)
        return np.stack([org[0] + s * x.astype(T), org[1] + s * y.astype(T), org[2] + s * z.astype(T)], 1)
    pf, po = pos(f), pos(o)
    verts = pf + (po - pf) * w[:, None]
    cols = None
    if color is not None:
        c = color.reshape(3, -1).astype(np.float32).astype(T)
        cw = color_weight.reshape(-1)
        hf, ho = cw[f] > 0, cw[o] > 0
        cf, co = c[:, f].T, c[:, o].T
        both = cf + (co - cf) * w[:, None]
        cols = np.where((hf & ho)[:, None], both, np.where(hf[:, None], cf, np.where(ho[:, None], co, T(0))))
    return verts, cols


# ------------------------------------------------------------------------------------------------ mesh checks
def mesh_stats(verts, faces, centre):
    """dict: closed (every edge in exactly two faces, once per direction), euler (V - E + F over the used vertices), signed volume about
    ``centre``, and the signs of normal . (centroid - centre) per face."""
    faces = np.asarray(faces, dtype=np.int64)
    v = np.asarray(verts, dtype=np.float64) - np.asarray(centre, dtype=np.float64)
    a, b, c = v[faces[:, 0]], v[faces[:, 1]], v[faces[:, 2]]
    normal = np.cross(b - a, c - a)
    out_sign = np.sign((normal * (a + b + c)).sum(1))
    volume = float((a * np.cross(b, c)).sum() / 6.0)
    directed = np.concatenate([faces[:, [0, 1]], faces[:, [1, 2]], faces[:, [2, 0]]])
    n = int(faces.max()) + 1 if len(faces) else 1
    key_d = directed[:, 0] * n + directed[:, 1]
    und = np.sort(directed, 1)
    key_u, cnt = np.unique(und[:, 0] * n + und[:, 1], return_counts=True)
    closed = bool(len(faces) > 0 and (cnt == 2).all() and len(np.unique(key_d)) == len(key_d))
    used = len(np.unique(faces))
    return {"closed": closed, "euler": used - len(key_u) + len(faces), "volume": volume, "out_sign": out_sign,
            "radius": np.linalg.norm(v[np.unique(faces)], axis=1) if len(faces) else np.zeros(0)}


def analytic_sphere_volume(dims, voxel, radius, trunc):
    """A fully observed volume of the sphere's own signed distance: origin, tsdf = clamp((|p| - r) / trunc, -1, 1) float32, weight 1."""
    nx, ny, nz = dims
    origin = (-0.5 * voxel * (nx - 1) + 0.0137, -0.5 * voxel * (ny - 1) - 0.0071, -0.5 * voxel * (nz - 1) + 0.0043)     # off the lattice
    p = voxel_centres(origin, voxel, dims, np.float64)
    t = np.clip((np.linalg.norm(p, axis=1) - radius) / trunc, -1, 1).astype(np.float32).reshape(nz, ny, nx)
    return origin, t, np.ones((nz, ny, nx), np.float32)


# ------------------------------------------------------------------------------------------------ the shared cases
INTEG = dict(dims=(40, 33, 27), voxel=0.05, H=40, W=48, fx=66.0, fy=58.0, seed=3)
SPHERES = (((-0.2, 0.02, 0.0), 0.45), ((0.27, 0.1, 0.06), 0.38))
_CASES = {}


def integration_case():
    """The GPU integration fixture: a 40 x 33 x 27 volume around two overlapping spheres and five 48 x 40 views with fx != fy --
    0, 1 regular; 2 inside the volume (voxels behind z_near); 3 looking away (a constant depth: only the projection rejects);
    4 a world_view with 1e30 and NaN entries. The depth maps hold NaN / 0 / negative / +Inf pixels, alpha is below the threshold on a
    patch, the colours of dead pixels are NaN. Everything float32."""
    if "integ" in _CASES:
        return _CASES["integ"]
    g = INTEG
    nx, ny, nz = g["dims"]
    H, W, fx, fy = g["H"], g["W"], g["fx"], g["fy"]
    rng = np.random.default_rng(g["seed"])
    origin = tuple(np.float32(v) for v in (-0.5 * g["voxel"] * (nx - 1) + 0.011, -0.5 * g["voxel"] * (ny - 1) + 0.007, -0.5 * g["voxel"] * (nz - 1) - 0.013))
    wv = np.stack([look_at((0.3, 0.2, -3.1), (0.0, 0.0, 0.0)), look_at((2.4, -0.5, -1.9), (0.05, 0.0, 0.0)),
                   look_at((-0.85, 0.55, -0.5), (0.2, 0.0, 0.1)), look_at((0.0, 0.0, -2.0), (0.0, 0.0, -6.0)), np.eye(4)])
    wv[4, 3, 0], wv[4, 0, 1], wv[4, 3, 2] = 1e30, np.nan, 2.0
    wv = wv.astype(np.float32)
    depth = np.stack([sphere_depth(wv[v].astype(np.float64), SPHERES, H, W, fx, fy) for v in range(3)] + [np.full((H, W), 2.0, np.float32)] * 2)
    color = rng.random((5, 3, H, W)).astype(np.float32)
    alpha = np.where(depth > 0, 0.9 + 0.1 * rng.random((5, H, W)), 0.1 * rng.random((5, H, W))).astype(np.float32)
    for v in range(3):                                       # special pixels on the spheres
        hit = np.argwhere(depth[v] > 0)
        pick = hit[rng.permutation(len(hit))[:16]]
        for k, (r, c) in enumerate(pick):
            depth[v, r, c] = (np.nan, 0.0, -1.5, np.inf)[k % 4]
            color[v, :, r, c] = np.nan
        r0, c0 = hit[len(hit) // 2]
        alpha[v, r0:r0 + 5, c0:c0 + 6] = 0.3                  # a patch below the threshold
    color[np.broadcast_to((depth[:, None] > 0) & np.isfinite(depth[:, None]), color.shape) == False] = np.nan  # noqa: E712
    c = {"dims": g["dims"], "voxel": np.float32(g["voxel"]), "trunc": np.float32(4 * g["voxel"]), "origin": origin, "H": H, "W": W,
         "fx": np.float32(fx), "fy": np.float32(fy), "world_view": np.ascontiguousarray(wv.reshape(5, 16)), "depth": depth,
         "color": color, "alpha": alpha}
    _CASES["integ"] = c
    return c


def run_case(c, views, use_color=True, use_alpha=True, state=None, dtype=np.float64):
    """``integrate`` of the case's views [list or slice] on ``state`` (empty when None)."""
    state = empty_state(c["dims"]) if state is None else state
    return integrate(state, c["origin"], c["voxel"], c["dims"], c["trunc"], c["depth"][views], c["world_view"][views].reshape(-1, 4, 4), c["fx"], c["fy"],
                     color=c["color"][views] if use_color else None, alpha=c["alpha"][views] if use_alpha else None, dtype=dtype)


def case_truth(c, use_color=True, use_alpha=True):
    """The float64 and float32 restatements of all five views at once, the fragile set, its share of the observed voxels and E_ref of
    tsdf weight and color color_weight outside it; computed once, shared, never modified."""
    key = ("truth", use_color, use_alpha)
    if key in _CASES:
        return _CASES[key]
    views = slice(0, 5)
    s64 = run_case(c, views, use_color, use_alpha)
    s32 = run_case(c, views, use_color, use_alpha, dtype=np.float32)
    frag = fragile(c["origin"], c["voxel"], c["dims"], c["trunc"], c["depth"], c["world_view"].reshape(-1, 4, 4), c["fx"], c["fy"],
                   alpha=c["alpha"] if use_alpha else None)
    observed = s64["weight"] > 0
    keep = ~frag
    e_t = float(np.abs((s32["tsdf"].astype(np.float64) * s32["weight"] - s64["tsdf"] * s64["weight"]) * keep).max())
    e_c = float(np.abs((s32["color"].astype(np.float64) * s32["color_weight"][None] - s64["color"] * s64["color_weight"][None]) * keep[None]).max())
    t = {"s64": s64, "s32": s32, "fragile": frag, "share": float((frag & observed).sum()) / max(1, int(observed.sum())),
         "observed": int(observed.sum()), "e_ref": {"tsdf": e_t, "color": e_c}}
    _CASES[key] = t
    return t


def check_state(got, want64, frag, e_ref, label="", use_color=True):
    """``got``: dict of float32 arrays (tsdf, weight, color, color_weight). Prints every figure, then asserts: finite; weights exact
    outside the fragile set; tsdf weight and color color_weight within 4 E_ref + 1e-6 max|.| of the float64 state there."""
    keep = ~frag
    g = {k: np.asarray(v, dtype=np.float64) for k, v in got.items()}
    names = ("tsdf", "weight") + (("color", "color_weight") if use_color else ())
    for k in names:
        assert np.isfinite(g[k]).all(), (label, k, "non-finite")
    wrong_w = int(((g["weight"] != want64["weight"]) & keep).sum())
    a, b = g["tsdf"] * g["weight"], want64["tsdf"] * want64["weight"]
    err_t, bound_t = float(np.abs((a - b) * keep).max()), 4 * e_ref["tsdf"] + 1e-6 * float(np.abs(b).max())
    print(f"{label} weight: {wrong_w} wrong of {int(keep.sum())} compared;  tsdf weight: E_ref {e_ref['tsdf']:.3e} kernel err {err_t:.3e} bound {bound_t:.3e}")
    assert wrong_w == 0, (label, "weight", wrong_w)
    assert err_t <= bound_t, (label, "tsdf weight", err_t, bound_t)
    if use_color:
        wrong_c = int(((g["color_weight"] != want64["color_weight"]) & keep).sum())
        a, b = g["color"] * g["color_weight"][None], want64["color"] * want64["color_weight"][None]
        err_c, bound_c = float(np.abs((a - b) * keep[None]).max()), 4 * e_ref["color"] + 1e-6 * float(np.abs(b).max())
        print(f"{label} color_weight: {wrong_c} wrong;  color color_weight: E_ref {e_ref['color']:.3e} kernel err {err_c:.3e} bound {bound_c:.3e}")
        assert wrong_c == 0, (label, "color_weight", wrong_c)
        assert err_c <= bound_c, (label, "color color_weight", err_c, bound_c)


E2E = dict(dims=(48, 48, 48), voxel=0.03, radius=0.5, H=128, W=128, f=1200.0, distance=20.0, alpha_min=0.3)


def e2e_case():
    """Six cameras on the axes, 20 away, around an analytic sphere of radius 0.5 at the origin, a 48^3 volume of 0.03 voxels: origin,
    depth [6,H,W], alpha (the facing ratio, the cosine between the surface normal and the ray back to the camera: with alpha_min = 0.3 a
    camera contributes where it sees the surface at less than 72.5 degrees, so the nearest-pixel depth of a grazing ray moves no vertex),
    colour (a function of the pixel), world_view [6,16], and the float64 restatement's volume and mesh. The geometry was chosen on the
    CPU: with it the restatement's mesh is closed, of genus 0 and star-shaped about the centre (tests/test_tsdf_truth.py)."""
    if "e2e" in _CASES:
        return _CASES["e2e"]
    g = E2E
    n = g["dims"][0]
    origin = tuple(np.float32(-0.5 * g["voxel"] * (n - 1) + o) for o in (0.0041, -0.0067, 0.0023))
    D = g["distance"]
    eyes = [(D, 0, 0), (-D, 0, 0), (0, D, 0), (0, -D, 0), (0, 0, D), (0, 0, -D)]
    ups = [(0, 1, 0), (0, 1, 0), (0, 0, 1), (0, 0, 1), (0, 1, 0), (0, 1, 0)]
    wv = np.stack([look_at(e, (0, 0, 0), u) for e, u in zip(eyes, ups)]).astype(np.float32)
    H, W = g["H"], g["W"]
    depth = np.stack([sphere_depth(wv[v].astype(np.float64), (((0, 0, 0), g["radius"]),), H, W, g["f"], g["f"]) for v in range(6)])
    jj, ii = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    color = np.stack([np.stack([(ii + v) % 7 / 7.0, (jj + 2 * v) % 5 / 5.0, np.full((H, W), v / 6.0)]) for v in range(6)]).astype(np.float32)
    alpha = np.stack([facing_ratio(wv[v].astype(np.float64), (0, 0, 0), g["radius"], depth[v], g["f"], g["f"]) for v in range(6)])
    c = {"dims": g["dims"], "voxel": np.float32(g["voxel"]), "trunc": np.float32(4 * g["voxel"]), "origin": origin, "H": H, "W": W,
         "fx": np.float32(g["f"]), "fy": np.float32(g["f"]), "world_view": np.ascontiguousarray(wv.reshape(6, 16)), "depth": depth, "color": color,
         "alpha": alpha, "alpha_min": g["alpha_min"]}
    s64 = integrate(empty_state(c["dims"]), origin, c["voxel"], c["dims"], c["trunc"], depth, wv, c["fx"], c["fy"], color=color, alpha=alpha,
                    alpha_min=g["alpha_min"])
    c["state32"] = {k: v.astype(np.float32) for k, v in s64.items()}
    c["mesh"] = mesh_of(c["state32"], origin, c["voxel"], c["dims"])
    frag = fragile(origin, c["voxel"], c["dims"], c["trunc"], depth, wv, c["fx"], c["fy"], alpha=alpha, alpha_min=g["alpha_min"])
    observed = s64["weight"] > 0
    c["fragile_share"] = float((frag & observed).sum()) / max(1, int(observed.sum()))
    _CASES["e2e"] = c
    return c


def mesh_of(state32, origin, voxel, dims, min_weight=1.0, dtype=np.float64):
    """The restatement's mesh of a float32 state: dict of n_active, tets, interp_v, faces, vertices, vertex_colors."""
    import mesh_truth
    n_active, tets, _ = cells_tets(state32["tsdf"], state32["weight"], min_weight)
    interp_v, faces, _ = mesh_truth.marching_tets(-state32["tsdf"].reshape(-1), tets)
    verts, cols = vertices(interp_v, state32["tsdf"], origin, voxel, dims, state32.get("color"), state32.get("color_weight"), dtype=dtype)
    return {"n_active": n_active, "tets": tets, "interp_v": interp_v, "faces": faces, "vertices": verts, "vertex_colors": cols}
