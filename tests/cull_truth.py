"""Plain references for the projection's own conservative culling data (csrc/f3dg_preprocess.hip: pretest_constant, cull_conic,
conservative_ellipse, the tile rectangle after tile culling with its half-tile hints, the small path's chunk boxes). Test infrastructure
only (numpy; the scenes need torch and the oracle).

What the data promises: it drops only work whose alpha is certainly below 1/255. `reach` states "the reference can blend Gaussian g at this
position" on the reference's own float32 roundings; `ellipse_restated` restates the formulas of the ellipse in float64; `ellipse_value64`
and `delta` state what the consumers' float32 evaluation of an exported ellipse can differ from its float64 value; `box_of` / `tiles_of`
state the tile rectangle and the hints of an ellipse. Derivations and measured figures: DESIGN.md section 4b.

Coordinates: "pixel-index" -- pixel (i, j) has its centre AT (i, j), its corners at i -+ 0.5 -- as the ellipse records are."""
import functools
import math

import numpy as np

import compositing_truth as ct

U = 2.0 ** -24                                         # unit roundoff of float32
ALPHA_MIN = ct.ALPHA_MIN                               # the float32 number 1.0f / 255.0f
NEAR = ct.NEAR
BAND = 1e-5                                            # S- / S+: alpha >= ALPHA_MIN (1 +- BAND)
THR_SHIFT = 4e-6                                       # the hardware log2 behind thr: 8 * 2^-23 * ln 2 = 6.6e-7, rounded up
ELLIPSE, EVERYTHING, NEVER = 0, 1, 2
SKIP_LO, SKIP_HI, COORD = 0x8000, 0x80000000, 0x7FFF
BOX_REL, BOX_ABS = 1.0e-3, 4.0e-3                      # twice the kernel's 1.0005 / 2e-3 px inflation of the ellipse's box


# ---- reach: the positions where the reference can blend a Gaussian -----------------------------------------------------------------------------------

def rays_at(pos, S, tanfov):
    """The float32 ray of pixel-index positions `pos` along an axis of S pixels: (float)((pos + 0.5 - S / 2.) / focal), focal the float32
    S / (2 tanfov). At integer positions this is compositing_truth.rays (= gof_oracle.c:484-486); at the half-integer corners it is the ray
    of f3dg_integrate.hip: integrate_pass1_rays_kernel. pos + 0.5 is exact in float32 for every multiple of 1/4 below 2^21."""
    f = np.float32(S) / (np.float32(2.0) * np.float32(tanfov))
    p = (np.asarray(pos, np.float64) + 0.5).astype(np.float32).astype(np.float64)
    return ((p - S / 2.0) / np.float64(f)).astype(np.float32)


def lattice(S, step=4):
    """Pixel-index positions -0.5, -0.5 + 1/step, ..., S - 0.5: the closed image interval. Index k is position k / step - 0.5."""
    return np.arange(step * S + 1, dtype=np.float64) / step - 0.5


def reach(records, W, H, tanfovx, tanfovy, positions, windows=None, integrate=False):
    """Can the reference blend Gaussian g at a position?  records: dict(view2gaussian [P,10], opac [P]) float32. positions: (xs, ys), 1-D
    pixel-index coordinates of a separable grid. windows [P,4] (optional): index ranges ix0, ix1, iy0, iy1 (exclusive ends) into xs / ys
    that bound the evaluation of each Gaussian (the reference visits a Gaussian only in the tiles of its 3-sigma rectangle).
    normal[3], AA, BB in float32 in the reference's order without FMA (gof_oracle.c:499-505); t = (float)(-BB / (2 AA)) > 0.2;
    min_value in float64, power = (float)(-0.5 min_value) clamped at 0. integrate=True: f3dg_integrate.hip ray_eval's variant, q = BB / AA
    ONE float32 division, t = -0.5f q, min_value = -q (BB / 4.) + CC.
    Returns a list over Gaussians of (ix0, iy0, S_plus, S_minus, AA, bhalf): the window's origin, the two boolean sets [ny, nx]
       S+ : t > 0.2 and opac exp(power) >= ALPHA_MIN (1 - 1e-5)        S- : the same with (1 + 1e-5)
    and the float32 AA and B / 2 of the window (the operands of the kernels' pre-test). exp is monotone, so the tests are made on power:
    opac exp(power) >= c  <=>  power >= ln(c / opac) (float64; its 1e-16 is nothing against the band).
    Why 1e-5: a faithful expf is within 2 ulp (2.4e-7), the product adds 6e-8, so every faithful implementation's pass set lies between S-
    and S+; the kernel leaves 1e-4 on thr, so S+ is still well inside what it promises to cover."""
    v2g = np.asarray(records["view2gaussian"], np.float32).reshape(-1, 10)
    opac = np.asarray(records["opac"], np.float32).reshape(-1)
    xs, ys = positions
    rx_all, ry_all = rays_at(xs, W, tanfovx), rays_at(ys, H, tanfovy)
    out = []
    two = np.float32(2.0)
    with np.errstate(all="ignore"):
        for g in range(v2g.shape[0]):
            ix0, ix1, iy0, iy1 = (0, len(xs), 0, len(ys)) if windows is None else [int(w) for w in windows[g]]
            if ix1 <= ix0 or iy1 <= iy0 or not opac[g] > 0:
                out.append((ix0, iy0, np.zeros((0, 0), bool), np.zeros((0, 0), bool), np.zeros((0, 0), np.float32), np.zeros((0, 0), np.float32)))
                continue
            v = v2g[g]
            rx, ry = rx_all[None, ix0:ix1], ry_all[iy0:iy1, None]
            n0 = (v[0] * rx + v[1] * ry) + v[2]
            n1 = (v[1] * rx + v[3] * ry) + v[4]
            n2 = (v[2] * rx + v[4] * ry) + v[5]
            AA = (rx * n0 + ry * n1) + n2
            bh = (v[6] * rx + v[7] * ry) + v[8]
            BB = two * bh
            A64, B64, CC = AA.astype(np.float64), BB.astype(np.float64), float(v[9])
            if integrate:
                q = (BB / AA).astype(np.float32)
                t = np.float32(-0.5) * q
                mv = -q.astype(np.float64) * (B64 / 4.0) + CC
            else:
                t = (-B64 / (2.0 * A64)).astype(np.float32)
                mv = -(B64 / A64) * (B64 / 4.0) + CC
            power = np.minimum((-0.5 * mv).astype(np.float32), np.float32(0.0)).astype(np.float64)
            front = t.astype(np.float64) > NEAR
            o = float(opac[g])
            sp = front & (power >= math.log(ALPHA_MIN * (1.0 - BAND) / o))
            sm = front & (power >= math.log(ALPHA_MIN * (1.0 + BAND) / o))
            out.append((ix0, iy0, sp, sm, AA, bh))
    return out


def reference_rect(means2D, radii, W, H):
    """The oracle's 3-sigma tile rectangle (auxiliary.h getRect; float32): rminx, rmaxx, rminy, rmaxy [P] (exclusive maxima)."""
    gx, gy = (W + 15) // 16, (H + 15) // 16
    m = np.asarray(means2D, np.float32).reshape(-1, 2)
    r = np.asarray(radii).astype(np.float32)
    t = np.float32(16.0)
    with np.errstate(all="ignore"):
        lo = lambda p, g: np.clip(np.nan_to_num(np.trunc((p - r) / t), nan=0.0, posinf=1e9, neginf=-1e9), 0, g).astype(np.int64)
        hi = lambda p, g: np.clip(np.nan_to_num(np.trunc((p + r + np.float32(15.0)) / t), nan=0.0, posinf=1e9, neginf=-1e9), 0, g).astype(np.int64)
        return lo(m[:, 0], gx), hi(m[:, 0], gx), lo(m[:, 1], gy), hi(m[:, 1], gy)


def windows_of(rect, W, H, step):
    """Index windows into lattice(W, step) / lattice(H, step) of the closed pixel range of a tile rectangle: tiles rmin .. rmax - 1 hold the
    positions 16 rmin - 0.5 .. 16 rmax - 0.5 (clipped to the image), corners included."""
    x0, x1, y0, y1 = rect
    ix0, ix1 = 16 * x0 * step, np.minimum(16 * x1, W) * step + 1
    iy0, iy1 = 16 * y0 * step, np.minimum(16 * y1, H) * step + 1
    empty = (x1 <= x0) | (y1 <= y0)
    return np.stack([ix0, np.where(empty, ix0, ix1), iy0, np.where(empty, iy0, iy1)], 1)


# ---- the ellipse, restated in float64 ------------------------------------------------------------------------------------------------------------------

def thr_of(opac, thr_shift=0.0):
    """thr = ln(1 / (255 opac)) - 1e-4 in float64 (+inf for opac <= 0, NaN for NaN), the kernel's value up to its hardware log2."""
    o = np.asarray(opac, np.float32).astype(np.float64)
    with np.errstate(all="ignore"):
        return np.where(o > 0, -np.log(255.0 * np.where(o > 0, o, 1.0)) - 1e-4 + thr_shift, np.where(o <= 0, np.inf, np.nan))


def conic_restated(vg, thr, X, Y, k_extra=2e-3, d_scale=1.0):
    """cull_conic in float64: the widened level set r^T M r <= 0 in ray space. Returns (m00, m01, m02, m11, m12, m22, ok). Shared with
    tests/tools/ellipse_margin_model.py (k_extra, d_scale: that tool's knobs; the kernel's values are the defaults)."""
    vg = np.asarray(vg, np.float64)
    with np.errstate(all="ignore"):
        C = vg[:, 9]
        cK = C - (-2.0 * thr + k_extra)
        X = np.broadcast_to(np.asarray(X, np.float64), C.shape); Y = np.broadcast_to(np.asarray(Y, np.float64), C.shape)
        A = np.abs(vg[:, 0]) * X * X + 2 * np.abs(vg[:, 1]) * X * Y + 2 * np.abs(vg[:, 2]) * X + np.abs(vg[:, 3]) * Y * Y + 2 * np.abs(vg[:, 4]) * Y + np.abs(vg[:, 5])
        Bn = np.abs(vg[:, 6]) * X + np.abs(vg[:, 7]) * Y + np.abs(vg[:, 8])
        D = d_scale * 1.1 * U * (6.0 * cK * A + 7.0 * Bn * Bn)
        B0, B1, B2 = vg[:, 6], vg[:, 7], vg[:, 8]
        return (cK * vg[:, 0] - B0 * B0, cK * vg[:, 1] - B0 * B1, cK * vg[:, 2] - B0 * B2, cK * vg[:, 3] - B1 * B1, cK * vg[:, 4] - B1 * B2,
                cK * vg[:, 5] - B2 * B2 - D, cK > 0)


def ellipse_restated(v2g, opac, W, H, tanfovx, tanfovy, thr_shift=0.0, have_scale=True):
    """Float64 restatement of cull_conic + conservative_ellipse for pairs (view2gaussian [n,10], opacity * coef [n], float32 values): true
    divisions and float64 square roots where the kernel multiplies by hardware reciprocals and takes float32 roots; the deliberate
    round-ups stay (x 1.000001 on the two roots, x (1 - 1e-7) on 1 / s^2), and so does the fattening of ellipses flatter than
    sqrt(1000) = 31.6 to that aspect. Returns dict(cls [n]: ELLIPSE / EVERYTHING / NEVER, cx, cy (pixel-index), a, b, c, fat [n] bool,
    ratio [n]: lmax^2 / (1000 det) = (aspect / 31.6)^2 of a fattened pair's form before the fattening, 1 otherwise)."""
    vg = np.asarray(v2g, np.float32).astype(np.float64).reshape(-1, 10)
    n = vg.shape[0]
    fx = float(np.float32(W) / (np.float32(2.0) * np.float32(tanfovx)))
    fy = float(np.float32(H) / (np.float32(2.0) * np.float32(tanfovy)))
    X, Y = float(np.float32(tanfovx)), float(np.float32(tanfovy))
    thr = thr_of(opac, thr_shift)
    cls = np.full(n, EVERYTHING, np.int64)
    fat = np.zeros(n, bool)
    with np.errstate(all="ignore"):
        never0 = np.isposinf(thr)
        m00, m01, m02, m11, m12, m22, ok = conic_restated(vg, np.where(np.isfinite(thr), thr, 0.0), X, Y)
        live = ok & np.isfinite(thr) & have_scale
        D22 = m00 * m11 - m01 * m01
        live &= (m00 > 0) & (m11 > 0) & (D22 > 1e-9 * np.abs(m00 * m11))
        cx, cy = (m01 * m12 - m02 * m11) / D22, (m01 * m02 - m00 * m12) / D22
        Qc = m22 + m02 * cx + m12 * cy
        live &= np.isfinite(Qc) & np.isfinite(cx) & np.isfinite(cy)
        empty = live & (Qc > 0) & (Qc < 1e300)
        live &= Qc < 0
        k = -1.0 / Qc
        a, b, c = m00 * k / (fx * fx), 2.0 * m01 * k / (fx * fy), m11 * k / (fy * fy)
        det, tr = a * c - 0.25 * b * b, a + c
        live &= (det > 0) & (tr < 1e300)
        disc = np.sqrt(np.maximum(0.25 * tr * tr - det, 0.0)) * 1.000001
        lmax = 0.5 * tr + disc
        live &= (lmax > 0) & (lmax < 1e300)
        flat = live & (lmax * lmax > 1000.0 * det)
        ratio = lmax * lmax / (1000.0 * det)             # (aspect / 31.6)^2 of the form before the fattening
        lmin = det / lmax
        vx, vy = 0.5 * b, lmax - a
        alt = (np.abs(vx) + np.abs(vy) < 1e-300 * lmax) | (a > c)
        vx, vy = np.where(alt, lmax - c, vx), np.where(alt, 0.5 * b, vy)
        n2 = vx * vx + vy * vy
        d = (lmax - 1000.0 * lmin) / n2
        a2, b2, c2 = a - d * vx * vx, b - 2.0 * d * vx * vy, c - d * vy * vy
        okflat = (lmin > 0) & (n2 > 0) & (a2 > 0) & (c2 > 0) & (a2 * c2 - 0.25 * b2 * b2 > 0)
        live &= ~flat | okflat
        a, b, c = np.where(flat, a2, a), np.where(flat, b2, b), np.where(flat, c2, c)
        lmax = np.where(flat, 1000.0 * lmin, lmax)
        s = 1.001 + 0.05 * (np.sqrt(lmax) * 1.000001)
        px, py = cx * fx + W / 2.0 - 0.5, cy * fy + H / 2.0 - 0.5
        live &= (np.abs(px) < 8192.0) & (np.abs(py) < 8192.0)
        is2 = 1.0 / (s * s) * (1.0 - 1e-7)
        a, b, c = a * is2, b * is2, c * is2
        live &= (a > 1e-30) & (c > 1e-30) & (a < 1e30) & (c < 1e30)
    cls[live] = ELLIPSE
    cls[empty & ~never0] = NEVER
    cls[never0] = NEVER
    fat = flat & live
    z = lambda x: np.where(live, x, 0.0)
    return dict(cls=cls, cx=z(px), cy=z(py), a=z(a), b=z(b), c=z(c), fat=fat, ratio=np.where(fat, ratio, 1.0))


def well_conditioned(v2g, opac, W, H, tanfovx, tanfovy, have_scale=True):
    """The restatement at thr, and per pair whether it is well conditioned: under thr -+ THR_SHIFT (what the hardware log2 behind the kernel's
    thr can differ from the float64 one) the outcome class stays and a, b, c move by less than 1e-6 relative (b: of b_scale).
    Pairs with opacity * coef near 1/255 (C - k near 0) and pairs with Qc near 0 fail it. The restatement also carries "centre_move" [n]:
    how far (px) the centre moves under that shift -- thr's last bits move the centre of a long ellipse seen in perspective."""
    r0 = ellipse_restated(v2g, opac, W, H, tanfovx, tanfovy, 0.0, have_scale)
    good = np.ones(r0["cls"].shape, bool)
    move = np.zeros(r0["cls"].shape)
    with np.errstate(all="ignore"):
        for sh in (-THR_SHIFT, THR_SHIFT):
            r = ellipse_restated(v2g, opac, W, H, tanfovx, tanfovy, sh, have_scale)
            good &= r["cls"] == r0["cls"]
            e = r0["cls"] == ELLIPSE
            mv = np.maximum(np.maximum(np.abs(r["a"] - r0["a"]) / r0["a"], np.abs(r["c"] - r0["c"]) / r0["c"]), np.abs(r["b"] - r0["b"]) / b_scale(r0))
            good &= ~e | (mv < 1e-6)
            move = np.maximum(move, np.where(e & (r["cls"] == ELLIPSE), np.maximum(np.abs(r["cx"] - r0["cx"]), np.abs(r["cy"] - r0["cy"])), 0.0))
    r0["centre_move"] = move
    return r0, good


def b_scale(r):
    """The magnitude b is measured against: its own, but not less than sqrt(a c) (b may vanish; |b| < 2 sqrt(a c) for an ellipse). A uniform
    scaling of the form by (1 + e) -- what thr, 1 / Qc and 1 / s^2 do -- moves b by e |b|, up to 2 e sqrt(a c)."""
    with np.errstate(all="ignore"):
        return np.maximum(np.abs(r["b"]), np.sqrt(r["a"] * r["c"]))


# Relative tolerance of the kernel's a, b (of b_scale), c against the restatement on well-conditioned pairs (derivation: DESIGN.md):
#   v_rcp_f64 (1 / Qc, 1 / s^2; the Newton-refined 1 / D22 is exact to 1e-16)      2 x 1e-8
#   the two float32 roots, rounded up, through s^2                                 2.3e-6
#   narrowing a, b, c to float32                                                   6e-8
#   the thr of a well-conditioned pair                                             1e-6 (the definition of well_conditioned)
COEF_RTOL = 2e-8 + 2.3e-6 + 6e-8 + 1e-6                # = 3.4e-6
# A FATTENED pair adds: the kernel's lmax is a float32 root of a float32-narrowed argument times 1.000001f, the restatement's a float64 root
# times 1.000001 -- they differ by ROOT_RHO = u / 2 (argument) + u (root) + u (product) + 4.7e-8 (1.000001f is 1 + 8 * 2^-23 = 1.00000095) <
# 2e-7 relative. The fattened form is Q - (lmax - 1000 lmin) v v^T: its larger eigenvalue 1000 lmin inherits that difference ABSOLUTELY,
# ROOT_RHO lmax, i.e. ROOT_RHO * ratio relative to itself, ratio = lmax^2 / (1000 det) = (aspect / 31.6)^2 (ellipse_restated returns it), once
# through lmax and once through lmin = det / lmax. So a fattened pair's tolerance is COEF_RTOL + 2 ROOT_RHO ratio.
ROOT_RHO = 2e-7


def coef_rtol(restated):
    return COEF_RTOL + np.where(restated["fat"], 2.0 * ROOT_RHO * restated["ratio"], 0.0)


# ---- the consumers' float32 evaluation of an exported ellipse ------------------------------------------------------------------------------------------

def ellipse_value64(cull, c, x, y):
    """E = a dx^2 + b dx dy + c dy^2 in float64 at pixel-index positions (x, y), of the exported float32 ellipse cull = (cx, cy, a, b), c."""
    cx, cy, a, b = (float(np.float32(v)) for v in cull)
    dx, dy = np.asarray(x, np.float64) - cx, np.asarray(y, np.float64) - cy
    return a * dx * dx + b * dx * dy + float(np.float32(c)) * dy * dy


def delta(cull, c, x, y):
    """Bound on |E^ - E| between the kernels' float32 evaluation E^ and ellipse_value64, by forward error analysis of exactly their order
    (f3dg_quad.h, f3dg_render4.hip, f3dg_integrate.hip, f3dg_contribution.hip), u = 2^-24:
        u0 = fl(qx0 - cx), dx^ = fl(u0 + q)                 2 roundings; 0 <= q <= 7 so |u0| <= |dx^| + 7: |dx^ - dx| <= u (2 |dx| + 8) =: ex
        dy^ likewise                                       2 roundings: ey = u (2 |dy| + 8)      (the origins qx0, q are exact integers or
                                                           halves below 2^22 at any image size; cx, cy are the stored float32 values)
        adx = fl(a dx^)                                    1 rounding
        in  = fma(b, dy^, adx)                             1 rounding
        cdy = fl(fl(c dy^) dy^)                            2 roundings (1 if the compiler contracted a product away: the larger count is taken)
        E^  = fma(dx^, in, cdy)                            1 rounding
    9 roundings in all. The term a dx^2 carries 3 of them (adx, in, E^), b dx dy 2, c dy^2 3:
        |E^ - E| <= g3 (a dx^2 + |b dx dy| + c dy^2) + (1 + g3) [(2 a |dx| + |b dy|) ex + (|b dx| + 2 c |dy|) ey + a ex^2 + |b| ex ey + c ey^2],
    g3 = 3u / (1 - 3u). A formula in u and the pair's own magnitudes at the position; nothing in it is fitted."""
    cx, cy, a, b = (float(np.float32(v)) for v in cull)
    c = float(np.float32(c))
    dx, dy = np.abs(np.asarray(x, np.float64) - cx), np.abs(np.asarray(y, np.float64) - cy)
    ex, ey = U * (2.0 * dx + 8.0), U * (2.0 * dy + 8.0)
    g3 = 3.0 * U / (1.0 - 3.0 * U)
    ab = abs(b)
    return g3 * (a * dx * dx + ab * dx * dy + c * dy * dy) + (1.0 + g3) * ((2.0 * a * dx + ab * dy) * ex + (ab * dx + 2.0 * c * dy) * ey
                                                                         + a * ex * ex + ab * ex * ey + c * ey * ey)


def classify(cull, c):
    """Outcome class of exported planes cull [n,4], c [n]: a = b = c = 0 is "everything", the far-away tiny ellipse is "never"."""
    cull = np.asarray(cull, np.float32).reshape(-1, 4)
    c = np.asarray(c, np.float32).reshape(-1)
    cls = np.full(c.shape, ELLIPSE, np.int64)
    cls[(cull[:, 2] == 0) & (cull[:, 3] == 0) & (c == 0)] = EVERYTHING
    cls[(cull[:, 0] == np.float32(-1.0e9)) & (cull[:, 1] == np.float32(-1.0e9)) & (cull[:, 2] == np.float32(1.0e30)) & (c == np.float32(1.0e30))] = NEVER
    return cls


def box_of(cull, c):
    """Axis-aligned half extents (hx, hy) [n] in float64 of a x^2 + b x y + c y^2 <= 1: sqrt(c / det), sqrt(a / det), det = a c - b^2 / 4.
    inf where det <= 0 ("everything")."""
    cull = np.asarray(cull, np.float32).astype(np.float64).reshape(-1, 4)
    c = np.asarray(c, np.float32).astype(np.float64).reshape(-1)
    a, b = cull[:, 2], cull[:, 3]
    det = a * c - 0.25 * b * b
    with np.errstate(all="ignore"):
        return np.where(det > 0, np.sqrt(c / det), np.inf), np.where(det > 0, np.sqrt(a / det), np.inf)


def tiles_of(centre, half, slack, grid, within=None):
    """Tile range [lo, hi) along one axis of the interval centre -+ (half (1 + slack[0]) + slack[1]) -- tile t holds the pixel centres
    16 t .. 16 t + 15 --, clamped to 0 .. grid and intersected with `within` = (lo, hi) when given; lo = hi = 0 when empty. With the half-tile
    hints of that range: skip_lo: the interval begins beyond 16 lo + 7 (it misses the first half of the first tile), skip_hi: it ends before
    16 (hi - 1) + 8. Returns lo, hi, skip_lo, skip_hi [n]."""
    centre = np.asarray(centre, np.float64)
    h = np.asarray(half, np.float64) * (1.0 + slack[0]) + slack[1]
    with np.errstate(all="ignore"):
        x0, x1 = centre - h, centre + h
        lo = np.clip(np.nan_to_num(np.ceil((x0 - 15.0) / 16.0), nan=0.0, posinf=1e9, neginf=-1e9), 0, grid).astype(np.int64)
        hi = np.clip(np.nan_to_num(np.floor(x1 / 16.0) + 1.0, nan=1e9, posinf=1e9, neginf=-1e9), 0, grid).astype(np.int64)
        if within is not None:
            lo, hi = np.maximum(lo, within[0]), np.minimum(hi, within[1])
        empty = hi <= lo
        lo, hi = np.where(empty, 0, lo), np.where(empty, 0, hi)
        return lo, hi, ~empty & (x0 > 16.0 * lo + 7.0), ~empty & (x1 < 16.0 * (hi - 1) + 8.0)


def pretest_k0(v2g, opac):
    """K0 = C + 2 thr with a float64 thr (+inf for opacity <= 0, NaN for NaN opacity)."""
    vg = np.asarray(v2g, np.float32).astype(np.float64).reshape(-1, 10)
    return vg[:, 9] + 2.0 * thr_of(opac)


# ---- the scenes --------------------------------------------------------------------------------------------------------------------------------------

EDGE_OPACITIES = (0.0, -0.1, float("nan"), 1.0, 1.5, 0.99, 0.0039,
                  ALPHA_MIN * (1 + 2.0 ** -20), ALPHA_MIN * (1 - 2.0 ** -20), ALPHA_MIN * (1 + 2.0 ** -10), ALPHA_MIN * (1 - 2.0 ** -10))

SCENE_NAMES = ("mixed", "filter", "needles", "close", "opacity_edges", "strip")


@functools.lru_cache(maxsize=None)
def scene(name):
    import torch
    import helpers
    def opacities(sc, lo, hi, seed):
        # The comparison with the restatement needs pairs whose ellipse does not move with the last bits of thr (well_conditioned): the
        # level set's size goes with k = 2 ln(255 opacity coef), so thr -+ 4e-6 moves a, b, c by 8e-6 / k -- below 1e-6 only for
        # opacity * coef > e^4 / 255 = 0.214. Faint Gaussians are the business of `opacity_edges`, which is exempt from the cap.
        gen = torch.Generator().manual_seed(seed)
        sc["opacities"] = (torch.rand(sc["P"], 1, generator=gen) * (hi - lo) + lo).contiguous()
        return sc

    if name in ("mixed", "precomp"):
        sc = opacities(helpers.make_scene(P=1500, res=(72, 56), s0=0.05, seed=3, view=(3, 5), aniso=True, behind_fraction=0.05), 0.35, 0.95, 4)
        if name == "precomp":
            o = [helpers.run_oracle(sc, view=v) for v in range(2)]
            sc = dict(sc)
            sc["cov3Ds_precomp"] = torch.from_numpy(o[0]["cov3D"].copy())
            sc["view2gaussian_precomp"] = torch.from_numpy(np.stack([x["view2gaussian"] for x in o]).copy())
        return sc
    if name == "filter":
        # (opacity * coef is what counts: the 2D filter's coef is 0.5 .. 0.8 at these sizes)
        return opacities(helpers.make_scene(P=800, res=(48, 40), s0=0.1, seed=5, view="oblique", kernel_size=0.3, scale_modifier=0.5), 0.7, 1.0, 6)
    if name == "needles":
        # Seen from 3 .. 5 units a needle is 50 .. 80 px long, 1.5 .. 2.5 px wide once fattened, and well conditioned -- but then s = 1.001 +
        # 0.05 px / semi-minor axis keeps every position of S+ below E = 0.9. Every 21st needle is therefore moved to 0.5 .. 1 units: those are
        # hundreds of pixels long, s is close to 1.001 and their S+ reaches the ellipse's outer tenth; thr's last bits move them by more than
        # 1e-6 (they are the scene's ill-conditioned 2.5 %).
        sc = opacities(helpers.make_scene(P=400, res=(64, 64), s0=0.05, seed=7, view="canonical", depth_range=(3.0, 5.0)), 0.35, 0.95, 8)
        sc["scales"] = torch.tensor([0.3, 1e-3, 1e-3]).repeat(400, 1).contiguous()
        gen = torch.Generator().manual_seed(8)
        torch.rand(400, 1, generator=gen)
        m = sc["means3D"].clone()
        z = torch.rand(len(m[::21]), generator=gen) * 0.5 + 0.5
        m[::21] = m[::21] * (z / m[::21, 2]).unsqueeze(1)
        sc["means3D"] = m.contiguous()
        return sc
    if name == "close":
        sc = opacities(helpers.make_scene(P=300, res=(64, 64), s0=0.05, seed=9, view="canonical", depth_range=(0.2, 0.5)), 0.35, 0.95, 10)
        gen = torch.Generator().manual_seed(11)
        sc["scales"] = (torch.rand(300, 3, generator=gen) * 0.4 + 0.1).contiguous()
        sc["scales"][1::4] *= 0.1             # a quarter ten times smaller: close, but the camera is outside their level set (real ellipses)
        sc["opacities"][::30] = 0.003         # ten below 1/255: their level set is empty ("never") although the camera is inside their 3 sigma
        return sc
    if name == "opacity_edges":
        sc = helpers.make_scene(P=512, res=(64, 64), s0=0.05, seed=13, view="oblique")
        sc["opacities"] = torch.tensor([EDGE_OPACITIES[i % len(EDGE_OPACITIES)] for i in range(512)], dtype=torch.float32).reshape(512, 1)
        return sc
    if name == "strip":
        return opacities(helpers.make_scene(P=300, res=(2048, 16), s0=0.05, seed=15, view="oblique"), 0.35, 0.95, 16)
    if name.startswith("tiny_P"):
        return helpers.make_scene(P=int(name[6:]), res=(32, 32), s0=0.08, seed=17, view="oblique")
    raise KeyError(name)


def n_views(name):
    return scene(name)["viewmatrix"].shape[0]


@functools.lru_cache(maxsize=None)
def oracle(name, view=0):
    """The oracle's projection of one view of a scene: view2gaussian, opacity * coef, radii, means2D, rectangles, tiles_touched."""
    import helpers
    sc = scene(name)
    o = helpers.run_oracle(sc, view=view)
    o.pop("oracle")
    return dict(view2gaussian=o["view2gaussian"].copy(), opac=o["conic_opacity"][:, 3].copy(), radii=np.asarray(o["radii"]).copy(),
                means2D=o["means2D"].copy(), tiles_touched=o["tiles_touched"].copy(), num_rendered=int(o["num_rendered"]),
                rect=reference_rect(o["means2D"], o["radii"], sc["W"], sc["H"]))


STEP = 4


@functools.lru_cache(maxsize=None)
def truth(name, view=0):
    """The small per-view facts, computed ONCE from the oracle's records (the GPU module asserts that the call's own records are bit-equal to
    them on the visible pairs): vis [P]; restated, good (well_conditioned); centres [P,5]: xmin, xmax, ymin, ymax, count of the
    compositing variant's S+ at the PIXEL CENTRES inside the reference rectangle (what the tile rectangle and the hints must cover)."""
    sc, o = scene(name), oracle(name, view)
    W, H = sc["W"], sc["H"]
    vis = o["radii"] > 0
    x0, x1, y0, y1 = o["rect"]
    win = np.stack([16 * x0, np.minimum(16 * x1, W), 16 * y0, np.minimum(16 * y1, H)], 1)      # the pixel centres of the rectangle's tiles
    win[~vis] = 0
    xs, ys = np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64)
    rc = reach(dict(view2gaussian=o["view2gaussian"], opac=o["opac"]), W, H, sc["tanfovx"], sc["tanfovy"], (xs, ys), win)
    centres = np.zeros((len(vis), 5))
    for g in np.nonzero(vis)[0]:
        ix0, iy0, sp = rc[g][:3]
        if sp.any():
            iy, ix = np.nonzero(sp)
            centres[g] = (xs[ix0 + ix.min()], xs[ix0 + ix.max()], ys[iy0 + iy.min()], ys[iy0 + iy.max()], sp.sum())
    have_scale = "view2gaussian_precomp" not in sc
    restated, good = well_conditioned(o["view2gaussian"], o["opac"], W, H, sc["tanfovx"], sc["tanfovy"], have_scale)
    return dict(vis=vis, centres=centres, restated=restated, good=good)


def walk(name, view=0):
    """Per visible Gaussian of a view with a non-empty S+: (g, x, y, AA, bhalf) -- the positions of S+ on the quarter-pixel lattice over
    the closed image rectangle inside the Gaussian's reference rectangle, integrate's variant on the whole lattice (it holds every ray
    position of integrate_pass1_rays_kernel: the pixel centres and the corners i - 0.5, i = 0 .. S) united with the compositing variant at
    the pixel centres, and the float32 operands of the kernels' pre-test there. A generator: a close-up scene has 2e7 such positions."""
    sc, o = scene(name), oracle(name, view)
    W, H = sc["W"], sc["H"]
    vis = o["radii"] > 0
    xs, ys = lattice(W, STEP), lattice(H, STEP)
    win = windows_of(o["rect"], W, H, STEP)
    for g in np.nonzero(vis)[0]:
        rec = dict(view2gaussian=o["view2gaussian"][g:g + 1], opac=o["opac"][g:g + 1])
        ix0, iy0, spi, _, AA, bh = reach(rec, W, H, sc["tanfovx"], sc["tanfovy"], (xs, ys), win[g:g + 1], integrate=True)[0]
        if spi.size == 0:
            continue
        spc = reach(rec, W, H, sc["tanfovx"], sc["tanfovy"], (xs, ys), win[g:g + 1], integrate=False)[0][2]
        iy, ix = np.mgrid[iy0:iy0 + spi.shape[0], ix0:ix0 + spi.shape[1]]
        both = spi | (spc & (ix % STEP == 2) & (iy % STEP == 2))      # index k is position k / 4 - 0.5: the integers are k = 2 (mod 4)
        if both.any():
            yield int(g), xs[ix[both]], ys[iy[both]], AA[both], bh[both]


def pretest_skips(K, AA, bh):
    """The kernels' pre-test fl(b * b) < fl(K * a) in float32 (b = B / 2, a = AA: the reference's own float32 values)."""
    with np.errstate(all="ignore"):
        return (bh * bh) < (np.float32(K) * AA)


def first_uncovered(cull, c, pos):
    """The first position of `pos` (x, y, ...) that the exported ellipse does not certainly cover: E64 > 1 - delta. None when all are
    covered; also returns how many positions have E64 > 0.9 (the exercised edge)."""
    if float(np.float32(cull[2])) == 0.0 and float(np.float32(cull[3])) == 0.0 and float(np.float32(c)) == 0.0:
        return None, 0                                  # "everything"
    E = ellipse_value64(cull, c, pos[0], pos[1])
    bad = ~(E <= 1.0 - delta(cull, c, pos[0], pos[1]))
    near = int((E > 0.9).sum())
    if bad.any():
        i = int(np.nonzero(bad)[0][0])
        return (float(pos[0][i]), float(pos[1][i]), float(E[i])), near
    return None, near
