"""Float64 truth of the point integration (csrc/f3dg_integrate.hip: the per-pixel pass and the point stage) ON ITS OWN INPUTS, and the
bars that hold a kernel to it. Test infrastructure only (numpy); the pattern of tests/compositing_truth.py, whose constants and K it reuses.

Inputs are what the kernels read: the records (view2gaussian, opacity * coef, rgb), the sorted list, the tile ranges, the background, the
view matrix, the points.

pass1_truth, per pixel, five rays (centre and four corners, forward.cu:864-905 = oracle/gof_oracle.c integrate_pass1):
    float32, the reference's order, no FMA -- INPUTS:  the rays; n0, n1, n2; AA; bhalf; BB = 2 bhalf; q = fl(BB / AA); t = fl(-0.5 q)
    float64 from there:  min_value = -q (BB / 4) + CC, power (clamped at 0), exp, alpha, test_T, every sum; the float32 literals (0.2f,
    0.99f, 1.0f / 255.0f, 0.0001f) at their own values
  with the decision sequence of the reference: skip when t <= 0.2f, skip when alpha < 1/255, skip -- NOT stop -- when test_T < 0.0001f, the
  pixel stops at 1,024 contributors. A pixel whose entries come within the margins of a decision (|t / 0.2 - 1|, |alpha / ALPHA_MIN - 1| >=
  M_ALPHA; |test_T / T_STOP - 1| >= M_STOP; minimum over its five rays and all entries) is left out; entries after a ray is certainly finished
  (T (1 - 1/255) < T_STOP (1 - M_STOP): every later entry is skipped whatever its alpha) no longer count.

points_truth, per point: projection and pixel as project_point (the float32 view transform in the kernel's order, ix / iy the double sum
cast to float; vz <= 0.2f and the image bounds decide); the point's float32 ray, then in float32 AA, BB, t = fl(-BB / fl(2 AA)) clamped to
the depth and power = fl(-0.5f fl(fl(fl(fl(AA t) t) + fl(BB t)) + CC)) -- all of it +, -, x, / in a fixed order, an INPUT: the polynomial
cancels about 1e3 x, so counting it as part of the blend would need a margin that keeps 1-40 % of the points. Float64 from `power` on:
raw = opac exp(power), alpha = min(0.99f, raw), skipped when alpha < 1/255, acc += alpha T, T *= 1 - alpha; A = sum alpha T. The contributors
are walked as the second loop of integrateCUDA walks them, INCLUDING the 16-bit wrap of the stored positions: ids are taken modulo 65,536,
the walk ends at the first id <= the previous one or > the last contributor, an accepted id addresses the list at THAT position. A point is
kept when its pixel is kept and min |raw / ALPHA_MIN - 1| >= M_ALPHA over its contributors."""
import functools

import numpy as np

from compositing_truth import ALPHA_MAX, ALPHA_MIN, M_ALPHA, M_STOP, T_STOP, k_stats

f32 = np.float32
NEAR = float(f32(0.2))                         # t <= 0.2f, vz <= 0.2f: float32 literals in this code
MAX_CONTRIB = 1024
CHUNK = 256
GROUPS = ("rgb", "alpha", "final_T", "alpha_integrated")


def focal(W, H, tanfovx, tanfovy):
    return f32(W) / (f32(2.0) * f32(tanfovx)), f32(H) / (f32(2.0) * f32(tanfovy))


def _quad32(v, rx, ry):
    """AA, BB of records v [m,10] at rays rx, ry [r] in float32, the reference's order: [m,r] each."""
    c = lambda k: v[:, k, None]
    n0 = (c(0) * rx + c(1) * ry) + c(2)
    n1 = (c(1) * rx + c(3) * ry) + c(4)
    n2 = (c(2) * rx + c(4) * ry) + c(5)
    AA = (rx * n0 + ry * n1) + n2
    BB = f32(2.0) * ((c(6) * rx + c(7) * ry) + c(8))
    return AA, BB


def pass1_truth(records, point_list, ranges, W, H, tanfovx, tanfovy, bg):
    """records: dict(view2gaussian [P,10], opac [P], rgb [P,3]) float32; point_list [R]; ranges [tiles,2] (positions into point_list).
    Returns out [9,H,W] (rgb + T bg, 0, 0, 0, max t over the five rays, alpha, 0), A_out [9,H,W], final_T / A_T [H,W], last [H,W] uint32,
    contrib (list per pixel id: the 1-based positions any ray used, in list order), keep [H,W], m_alpha / m_stop [H,W]."""
    v2g = np.ascontiguousarray(records["view2gaussian"], dtype=f32)
    opac = np.asarray(records["opac"], dtype=f32).reshape(-1).astype(np.float64)
    rgb = np.asarray(records["rgb"], dtype=f32).astype(np.float64)
    point_list = np.asarray(point_list).astype(np.int64)
    ranges = np.asarray(ranges).astype(np.int64).reshape(-1, 2)
    bg = np.asarray(bg, dtype=f32).astype(np.float64).reshape(3)
    fx, fy = focal(W, H, tanfovx, tanfovy)
    gx, gy = (W + 15) // 16, (H + 15) // 16
    assert ranges.shape[0] == gx * gy
    out, A_out = np.zeros((9, H, W)), np.zeros((9, H, W))
    final_T = np.ones((H, W))
    last = np.zeros((H, W), np.uint32)
    m_alpha, m_stop = np.full((H, W), np.inf), np.full((H, W), np.inf)
    contrib = [np.zeros(0, np.int64)] * (H * W)
    offs = np.array([(0, 0), (-.5, -.5), (.5, -.5), (-.5, .5), (.5, .5)], f32)
    with np.errstate(all="ignore"):
        for tile in range(gx * gy):
            x0, y0 = (tile % gx) * 16, (tile // gx) * 16
            ys, xs = np.meshgrid(np.arange(y0, min(y0 + 16, H)), np.arange(x0, min(x0 + 16, W)), indexing="ij")
            ys, xs = ys.ravel(), xs.ravel()
            n = xs.size
            # ray k of pixel p is element k * n + p
            pxf = ((xs.astype(f32) + f32(0.5))[None, :] + offs[:, 0:1]).ravel()
            pyf = ((ys.astype(f32) + f32(0.5))[None, :] + offs[:, 1:2]).ravel()
            rx = ((pxf.astype(np.float64) - W / 2.) / np.float64(fx)).astype(f32)
            ry = ((pyf.astype(np.float64) - H / 2.) / np.float64(fy)).astype(f32)
            pix_of = np.tile(np.arange(n), 5)
            T = np.ones(5 * n)
            fin = np.zeros(5 * n, bool)                      # certainly finished rays
            done = np.zeros(n, bool)                         # pixels at 1,024 contributors
            C, CA = np.zeros((3, n)), np.zeros((3, n))
            C6, C7 = np.zeros(n), np.zeros(n)
            ma, ms = np.full(n, np.inf), np.full(n, np.inf)
            lastc, nloc = np.zeros(n, np.uint32), np.zeros(n, np.int64)
            hits_pix, hits_pos = [], []
            a, b = ranges[tile]
            for c0 in range(int(a), int(b), CHUNK):
                if (fin | done[pix_of]).all():
                    break
                g = point_list[c0:min(c0 + CHUNK, int(b))]
                v = v2g[g]
                AA, BB = _quad32(v, rx, ry)                  # float32 [m, 5n]
                q = BB / AA
                t = (f32(-0.5) * q).astype(np.float64)
                p1 = ~(t <= NEAR)
                power = np.minimum(-0.5 * (-q.astype(np.float64) * (BB.astype(np.float64) / 4.0) + v[:, 9, None].astype(np.float64)), 0.0)
                alpha = np.fmin(ALPHA_MAX, opac[g][:, None] * np.exp(power))
                p2 = p1 & ~(alpha < ALPHA_MIN)
                marg = np.minimum(np.abs(t / NEAR - 1.0), np.where(p1, np.abs(alpha / ALPHA_MIN - 1.0), np.inf))
                prev = 0
                # only an entry some ray can use changes the state; the margins of the ones in between count under the state before them
                for e in list(np.flatnonzero(p2.any(1))) + [len(g)]:
                    live = ~(fin | done[pix_of])
                    hi = min(e + 1, len(g))                   # entries prev .. e: the skipped ones and e itself
                    if hi > prev:
                        seg = np.where(live, marg[prev:hi].min(0), np.inf)
                        ma = np.minimum(ma, seg.reshape(5, n).min(0))
                    prev = hi
                    if e == len(g):
                        break
                    idx = np.flatnonzero(p2[e] & live)
                    if idx.size == 0:
                        continue
                    al, Tc = alpha[e, idx], T[idx]
                    tt = Tc * (1.0 - al)
                    np.minimum.at(ms, pix_of[idx], np.abs(tt / T_STOP - 1.0))
                    use = ~(tt < T_STOP)
                    iu = idx[use]
                    if iu.size == 0:
                        continue
                    cen = iu < n                              # the centre ray carries colour and alpha
                    w = al[use][cen] * Tc[use][cen]
                    pc = iu[cen]
                    for ch in range(3):
                        C[ch, pc] += rgb[g[e], ch] * w
                        CA[ch, pc] += abs(rgb[g[e], ch]) * w
                    C7[pc] += w
                    np.maximum.at(C6, pix_of[iu], t[e, iu])
                    T[iu] = tt[use]
                    fin[iu] = T[iu] * (1.0 - ALPHA_MIN) < T_STOP * (1.0 - M_STOP)
                    pu = np.unique(pix_of[iu])
                    lastc[pu] = c0 - a + e + 1
                    nloc[pu] += 1
                    done[pu] = nloc[pu] >= MAX_CONTRIB
                    hits_pix.append(pu)
                    hits_pos.append(np.full(pu.size, c0 - a + e + 1, np.int64))
            T0 = T[:n]
            out[:3, ys, xs] = C + T0[None] * bg[:, None]
            A_out[:3, ys, xs] = CA + T0[None] * np.abs(bg)[:, None]
            out[6, ys, xs] = C6; A_out[6, ys, xs] = np.abs(C6)
            out[7, ys, xs] = C7; A_out[7, ys, xs] = C7
            final_T[ys, xs] = T0
            last[ys, xs] = lastc
            m_alpha[ys, xs] = ma; m_stop[ys, xs] = ms
            if hits_pix:
                hp, hq = np.concatenate(hits_pix), np.concatenate(hits_pos)
                order = np.argsort(hp, kind="stable")
                hp, hq = hp[order], hq[order]
                cuts = np.searchsorted(hp, np.arange(n + 1))
                for p in range(n):
                    contrib[int(ys[p]) * W + int(xs[p])] = hq[cuts[p]:cuts[p + 1]]
    keep = (m_alpha >= M_ALPHA) & (m_stop >= M_STOP)
    return dict(out=out, A_out=A_out, final_T=final_T, A_T=final_T.copy(), last=last, contrib=contrib, keep=keep, m_alpha=m_alpha, m_stop=m_stop)


def project_points(pts, viewmatrix, W, H, tanfovx, tanfovy):
    """project_point of every point: ok [PN], pixel x / y (int, valid where ok), float32 ix, iy, depth."""
    fx, fy = focal(W, H, tanfovx, tanfovy)
    view = np.asarray(viewmatrix, dtype=f32).reshape(16)
    p = np.asarray(pts, dtype=f32)
    with np.errstate(all="ignore"):
        vx = ((view[0] * p[:, 0] + view[4] * p[:, 1]) + view[8] * p[:, 2]) + view[12]
        vy = ((view[1] * p[:, 0] + view[5] * p[:, 1]) + view[9] * p[:, 2]) + view[13]
        vz = ((view[2] * p[:, 0] + view[6] * p[:, 1]) + view[10] * p[:, 2]) + view[14]
        ix = ((fx * vx / (vz + f32(0.0000001))).astype(np.float64) + W / 2.).astype(f32)
        iy = ((fy * vy / (vz + f32(0.0000001))).astype(np.float64) + H / 2.).astype(f32)
        ok = ~(vz <= f32(0.2)) & ~((ix < 0) | (ix >= W) | (iy < 0) | (iy >= H))
        px, py = np.where(ok, ix, 0).astype(np.int64), np.where(ok, iy, 0).astype(np.int64)
    return ok, px, py, ix, iy, vz


def walk(pos, last):
    """The second loop's walk through a pixel's stored positions (full 1-based positions `pos`, stored modulo 65,536): returns the accepted
    16-bit ids, whether the walk stops at a wrapped id before the list's end, and whether it accepts an id that is not the position stored."""
    ids = pos & 0xFFFF
    bad = (ids <= np.concatenate([[0], ids[:-1]])) | (ids > last)
    stop = int(np.argmax(bad)) if bad.any() else len(ids)
    return ids[:stop], bool(stop < len(ids)), bool((pos[:stop] > 0xFFFF).any())


def wrap_census(p1):
    """Per pixel [H,W]: the walk stops at a wrapped id / accepts an aliased id."""
    H, W = p1["last"].shape
    stops, aliased = np.zeros(H * W, bool), np.zeros(H * W, bool)
    for i, pos in enumerate(p1["contrib"]):
        _, stops[i], aliased[i] = walk(pos, int(p1["last"].ravel()[i]))
    return stops.reshape(H, W), aliased.reshape(H, W)


def kept_points_per_pixel(p1, pt):
    """[H,W]: how many kept in-image points each pixel holds."""
    n = np.zeros(p1["keep"].size, np.int64)
    np.add.at(n, pt["pix"][pt["keep"] & pt["ok"]], 1)
    return n.reshape(p1["keep"].shape)


def points_truth(records, point_list, ranges, p1, pts, viewmatrix, W, H, tanfovx, tanfovy, wrap=True):
    """Returns ok [PN] (in the image), pix [PN] (pixel id, -1 where not ok), ai [PN] (1.0 where not ok), A [PN], keep [PN]. wrap=False: what
    an implementation that stored full positions would compute (every contributor at its own position) -- NOT the reference; for the test
    that shows the wrap scenes tell the two apart."""
    v2g = np.ascontiguousarray(records["view2gaussian"], dtype=f32)
    opac = np.asarray(records["opac"], dtype=f32).reshape(-1).astype(np.float64)
    point_list = np.asarray(point_list).astype(np.int64)
    ranges = np.asarray(ranges).astype(np.int64).reshape(-1, 2)
    fx, fy = focal(W, H, tanfovx, tanfovy)
    ok, px, py, ix, iy, vz = project_points(pts, viewmatrix, W, H, tanfovx, tanfovy)
    pix = np.where(ok, py * W + px, -1)
    ai, A, keep = np.ones(len(pts)), np.zeros(len(pts)), np.zeros(len(pts), bool)
    gx = (W + 15) // 16
    sel = np.flatnonzero(ok)
    sel = sel[np.argsort(pix[sel], kind="stable")]
    cuts = np.flatnonzero(np.diff(pix[sel])) + 1
    with np.errstate(all="ignore"):
        for grp in np.split(sel, cuts) if sel.size else []:
            pid = int(pix[grp[0]])
            y, x = divmod(pid, W)
            ids = walk(p1["contrib"][pid], int(p1["last"][y, x]))[0] if wrap else p1["contrib"][pid]
            pk = bool(p1["keep"][y, x])
            if ids.size == 0:
                ai[grp] = 0.0
                keep[grp] = pk
                continue
            tile = (y // 16) * gx + x // 16
            g = point_list[ranges[tile, 0] + ids - 1]
            rx = ((ix[grp].astype(np.float64) - W / 2.) / np.float64(fx)).astype(f32)
            ry = ((iy[grp].astype(np.float64) - H / 2.) / np.float64(fy)).astype(f32)
            v = v2g[g]
            AA, BB = _quad32(v, rx, ry)                       # [m, k]
            t = -BB / (f32(2.0) * AA)
            depth = vz[grp][None, :]
            t = np.where(t > depth, depth, t).astype(f32)
            power = (f32(-0.5) * (((AA * t) * t + BB * t) + v[:, 9, None])).astype(np.float64)
            raw = opac[g][:, None] * np.exp(power)
            alpha = np.fmin(ALPHA_MAX, raw)
            a = np.where(alpha < ALPHA_MIN, 0.0, alpha)
            Tb = np.cumprod(1.0 - a, axis=0)                  # T after each contributor, in list order
            Tb = np.concatenate([np.ones((1, len(grp))), Tb[:-1]], 0)
            ai[grp] = A[grp] = (a * Tb).sum(0)
            keep[grp] = pk & (np.abs(raw / ALPHA_MIN - 1.0).min(0) >= M_ALPHA)
    return dict(ok=ok, pix=pix, ai=ai, A=A, keep=keep)


def figures(p1, pt, out, final_T, ai):
    """K (median, p99, max) per group of an image [9,H,W], a final_T plane [H,W] and alpha_integrated [PN] over what the truth keeps."""
    k = p1["keep"]
    return {"rgb": k_stats(out[:3], p1["out"][:3], p1["A_out"][:3], k), "alpha": k_stats(out[7], p1["out"][7], p1["A_out"][7], k),
            "final_T": k_stats(final_T, p1["final_T"], p1["A_T"], k), "alpha_integrated": k_stats(ai, pt["ai"], pt["A"], pt["keep"])}


def check_bars(label, p1, pt, fig, fig_oracle, m, failures, out, final_T, ai, groups=GROUPS, show=True):
    """Every K statistic <= m x the oracle's for the same scene, group and statistic (no floor); exact zeros where A = 0. Appends (label,
    group, what, got, bar) to `failures`; prints kernel and oracle side by side."""
    for g in groups:
        for s, (kh, ko) in zip(("median", "p99", "max"), zip(fig[g], fig_oracle[g])):
            if not kh <= m * ko:
                failures.append((label, g, "K " + s, kh, m * ko))
        if show:
            print("%s %-16s K med / p99 / max  kernel %.2f / %.2f / %.1f   oracle %.2f / %.2f / %.1f" % ((label, g) + tuple(fig[g]) + tuple(fig_oracle[g])))
    k = p1["keep"]
    for g, x, t, a, kp in (("rgb", out[:3], p1["out"][:3], p1["A_out"][:3], k), ("alpha", out[7], p1["out"][7], p1["A_out"][7], k),
                           ("final_T", final_T, p1["final_T"], p1["A_T"], k), ("alpha_integrated", ai, pt["ai"], pt["A"], pt["keep"])):
        if g not in groups:
            continue
        z = (a == 0) & np.broadcast_to(kp, a.shape)
        if not np.array_equal(np.asarray(x, np.float64)[z], t[z]):
            failures.append((label, g, "exact zeros", int((np.asarray(x, np.float64)[z] != t[z]).sum()), 0))


# ---- the scenes -------------------------------------------------------------------------------------------------------------------------------------

SCENES = {   # name: (helpers.make_scene arguments, points)
    "I1": (dict(P=2000, res=(64, 64), s0=0.05, view="canonical"), 20000),
    "I4": (dict(P=4000, res=(100, 72), s0=0.04, view="oblique", kernel_size=0.1), 30000),              # partial tiles
    "small_bg": (dict(P=1500, res=(33, 18), s0=0.01, view="oblique", bg=(0.2, 0.5, 0.7)), 8000),       # one column of a third tile
    "one_more": (dict(P=600, res=(17, 17), s0=0.05, view="canonical"), 4000),                          # a tile and one pixel more
    "aniso": (dict(P=3000, res=(96, 80), s0=0.3, aniso=True, view="oblique"), 10000),
}
WRAP_SCENES = ("wrap_stop", "wrap_alias")          # tile lists longer than 65,535 entries: the (u_int16_t) cast of forward.cu:969 wraps
SHORT_SCENES = tuple("short%d" % k for k in (1, 2, 3, 4)) + ("short0",)
N_POINTS = dict({k: v[1] for k, v in SCENES.items()}, wrap_stop=4000, wrap_alias=4000, **{k: 3000 for k in SHORT_SCENES})


def _alias_scene():
    """A list of 69,837 entries in one tile whose pixels both stop at a wrapped id and accept an aliased one: four large Gaussians in front
    (every pixel's first contributors, small ids), fillers confined to the tile's left half, 300 mid-sized ones behind everything."""
    import helpers
    import torch
    P, nA, nC = 72000, 4, 300
    sc = helpers.make_scene(P=P, res=(16, 16), s0=0.003, seed=61, view="canonical")
    m, s, op = sc["means3D"].clone(), sc["scales"].clone(), sc["opacities"].clone()
    B = slice(nA, P - nC)
    m[B, 0] = -m[B, 0].abs() - 0.15 * m[B, 2] / 7.0
    gen = torch.Generator().manual_seed(61)
    m[:nA] = torch.tensor([0.0, 0.0, 5.0]) + 0.05 * torch.randn(nA, 3, generator=gen); s[:nA] = 1.0; op[:nA] = 0.3
    m[P - nC:, 2] = 10.0 + torch.rand(nC, generator=gen); m[P - nC:, :2] *= 1.2; s[P - nC:] = 0.4; op[P - nC:] = 0.4
    sc["means3D"], sc["scales"], sc["opacities"] = m.contiguous(), s.contiguous(), op.contiguous()
    return sc


def _short_scene(k):
    """One 16 x 16 tile: k large Gaussians on the axis at distinct depths (every pixel's list holds all k) and one small one in a corner, so
    a pixel has k or k + 1 contributors; k = 0: the small one alone, most pixels have none."""
    import helpers
    import torch
    sc = helpers.make_scene(P=k + 1, res=(16, 16), s0=0.05, seed=7, view="canonical", bg=(0.1, 0.6, 0.3))
    m, s, op = sc["means3D"].clone(), sc["scales"].clone(), sc["opacities"].clone()
    for i in range(k):
        m[i] = torch.tensor([0.0, 0.0, 5.0 + 0.7 * i]); s[i] = 1.0; op[i] = 0.3
    m[k] = torch.tensor([-0.45, -0.45, 7.0]); s[k] = 0.06; op[k] = 0.8
    sc["means3D"], sc["scales"], sc["opacities"] = m.contiguous(), s.contiguous(), op.contiguous()
    return sc


@functools.lru_cache(maxsize=None)
def scene(name):
    import helpers
    if name in SCENES:
        return helpers.make_scene(**SCENES[name][0])
    if name == "wrap_stop":
        return helpers.make_scene(P=70000, res=(16, 16), s0=0.003, view="canonical")
    if name == "wrap_alias":
        return _alias_scene()
    return _short_scene(int(name[5:]))


@functools.lru_cache(maxsize=None)
def points(name):
    import helpers_integrate
    sc, n = scene(name), N_POINTS[name]

    def all_over_the_tile(n, z0, z1, seed):
        rng = np.random.default_rng(seed)
        z = rng.uniform(z0, z1, n)
        p = np.concatenate([rng.uniform(-1.05, 1.05, (n, 2)) * (z * sc["tanfovx"])[:, None], z[:, None]], 1)
        p[: n // 50, 2] = -1.0                        # behind the camera
        return np.ascontiguousarray(p, dtype=f32)

    if name in SHORT_SCENES:       # in front of, between and behind the Gaussians (make_points stays near the Gaussians: one pixel here)
        pts = all_over_the_tile(n, 4.0, 9.0, 3)
    elif name in WRAP_SCENES:      # (make_points follows the fillers into wrap_alias's left half, where no pixel accepts an aliased id, and stays
        # in front of most contributors past position 65,535: the other half lies all over the tile, down to behind every Gaussian)
        pts = np.concatenate([helpers_integrate.make_points(sc, n // 2), all_over_the_tile(n - n // 2, 4.0, 12.0, 4)])
    else:
        pts = helpers_integrate.make_points(sc, n)
    pts.setflags(write=False)
    return pts


@functools.lru_cache(maxsize=None)
def oracle(name):
    """The CPU oracle's integrate of a scene and its points: outputs and intermediates."""
    import helpers_integrate
    sc = scene(name)
    o = helpers_integrate.oracle_integrate(sc, points(name))
    it = o.pop("oracle").intermediates()
    if sc["colors_precomp"] is not None:
        it["rgb"] = sc["colors_precomp"].numpy().astype(f32)
    o.update(it)
    return o


def records_of(o):
    return dict(view2gaussian=o["view2gaussian"], opac=o["conic_opacity"][:, 3], rgb=o["rgb"])


@functools.lru_cache(maxsize=None)
def oracle_truth(name):
    """The truth on the ORACLE's records and lists, and the oracle's own figures against it: (pass 1, points, figures). A kernel whose exported
    records and lists are bit-equal to the oracle's on the Gaussians that are in a list has this very truth."""
    sc, o = scene(name), oracle(name)
    shape = (sc["W"], sc["H"], sc["tanfovx"], sc["tanfovy"])
    p1 = pass1_truth(records_of(o), o["point_list"], o["ranges"], *shape, sc["bg"].numpy())
    pt = points_truth(records_of(o), o["point_list"], o["ranges"], p1, points(name), sc["viewmatrix"][0].numpy(), *shape)
    return p1, pt, figures(p1, pt, o["out"], o["final_T"][0], o["ai"])
