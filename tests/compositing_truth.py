"""Float64 truth of the compositing forward ON ITS OWN INPUTS, and the bars that hold a kernel to it. Test infrastructure only (numpy).

Every compositing mode of the library reproduces the reference's float32 evaluation of the ray quadratic (forward.cu:500-505 =
oracle/gof_oracle.c:499-505: normal[3], AA, BB in float32, no FMA): at sigma0 = 0.01 that rounding alone moves the image 0.6 % (median) away
from an all-float64 evaluation of the scene (fwd_truth.render_fp64), so a kernel can only be held to float64 if those roundings count as
INPUTS of the blend, as dL_dview2gaussian does for the per-Gaussian backward (tests/test_per_gaussian_backward_gpu.py).

blend_truth takes  (1) the records (view2gaussian, opacity * coef, rgb), the sorted list and the tile ranges,
                   (2) the float32 ray of each pixel,
                   (3) normal[3], AA, BB evaluated in float32 in the reference's order,
and does everything after that in float64: t, min_value, power, exp, alpha, test_T, mapped_max_t, the normal's length, every sum and
product, the final normalisation of the distortion -- with the decision sequence of gof_oracle.c:493-547 and the reference's literals at
their own values (0.99f, 1.0f / 255.0f, 0.0001f are float32 numbers; 0.2, 100.0, 0.5, 1e-7 are doubles). What is left between an
implementation and this truth is the rounding of its blend alone:  K = |x - truth| / (2^-24 A),  A = the sum of the magnitudes of the terms
of that pixel and channel. A pixel whose visited entries come within a few float32 ulp of a decision (alpha >= 1/255, t > 0.2,
test_T < 1e-4; T > 0.5 for the depth) may legitimately decide the other way: such pixels are left out, by margins stated here and capped by
tests/test_compositing_truth.py."""
import functools

import numpy as np

EPS = 2.0 ** -24
ALPHA_MAX = float(np.float32(0.99))                   # fminf(0.99f, ...)
ALPHA_MIN = float(np.float32(1.0) / np.float32(255.0))  # alpha < 1.0f / 255.0f
T_STOP = float(np.float32(0.0001))                    # test_T < 0.0001f
NEAR, FAR = 0.2, 100.0                                # auxiliary.h:27-28 (double literals)
M_ALPHA, M_STOP, M_HALF = 2.0 ** -18, 2.0 ** -14, 2.0 ** -14
NO_MEDIAN = np.uint32(0xFFFFFFFF)

# 2^-18 ~ 60 float32 ulp: an alpha carries an expf, a product and the rounding of power (|power| <= 5.6, so one ulp of power moves alpha by up
# to 5.6 ulp). A transmittance is a chain of up to ~1,600 products on these scenes: n 2^-24 ~ 1e-4 worst case (2^-14 = 6e-5), sqrt(n) typical.

GROUPS = ("rgb", "normal", "depth", "alpha", "distortion")
CHANNELS = {"rgb": slice(0, 3), "normal": slice(3, 6), "depth": slice(6, 7), "alpha": slice(7, 8), "distortion": slice(8, 9)}
PLANES = ("T", "dist1", "dist2", "dist_raw")


def _f32(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32))


def rays(W, H, tanfovx, tanfovy):
    """The float32 ray of every pixel column / row (gof_oracle.c:484-486; focal as rasterizer_impl.cu:274-275)."""
    fx = np.float32(W) / (np.float32(2.0) * np.float32(tanfovx))
    fy = np.float32(H) / (np.float32(2.0) * np.float32(tanfovy))
    pixx = (np.arange(W, dtype=np.float32) + np.float32(0.5)).astype(np.float64)
    pixy = (np.arange(H, dtype=np.float32) + np.float32(0.5)).astype(np.float64)
    return ((pixx - W / 2.0) / np.float64(fx)).astype(np.float32), ((pixy - H / 2.0) / np.float64(fy)).astype(np.float32)


def blend_truth(records, point_list, ranges, W, H, tanfovx, tanfovy, bg):
    """records: dict(view2gaussian [P,10], opac [P], rgb [P,3]) float32; point_list [R]; ranges [tiles, 2] (positions into point_list).
    Returns a dict: out [9,H,W], final_T [4,H,W] (T, dist1, dist2, un-normalised distortion), n_contrib [2,H,W] uint32 (last and median
    contributor, 1-based positions in the tile's list; 0 / 0xFFFFFFFF: none), A_out [9,H,W], A_T [4,H,W], m_alpha / m_stop / m_half [H,W],
    last_rgb [3,H,W] (the rgb term of the last blended entry), keep / keep_depth [H,W] (the pixels the comparison covers)."""
    v2g, opac, rgb = _f32(records["view2gaussian"]), _f32(records["opac"]).reshape(-1), _f32(records["rgb"])
    point_list = np.asarray(point_list).astype(np.int64)
    ranges = np.asarray(ranges).astype(np.int64).reshape(-1, 2)
    bg = np.asarray(bg, dtype=np.float32).astype(np.float64).reshape(3)
    gx, gy = (W + 15) // 16, (H + 15) // 16
    assert ranges.shape[0] == gx * gy
    rx_all, ry_all = rays(W, H, tanfovx, tanfovy)
    out, A_out = np.zeros((9, H, W)), np.zeros((9, H, W))
    fT, A_T = np.zeros((4, H, W)), np.zeros((4, H, W))
    ncon = np.zeros((2, H, W), np.uint32)
    marg = np.full((3, H, W), np.inf)
    last_rgb = np.zeros((3, H, W))
    two = np.float32(2.0)
    with np.errstate(all="ignore"):
        for tile in range(gx * gy):
            x0, y0 = (tile % gx) * 16, (tile // gx) * 16
            ys, xs = np.meshgrid(np.arange(y0, min(y0 + 16, H)), np.arange(x0, min(x0 + 16, W)), indexing="ij")
            ys, xs = ys.ravel(), xs.ravel()
            n = xs.size
            rx, ry = rx_all[xs], ry_all[ys]
            T = np.ones(n); C = np.zeros((8, n)); CA = np.zeros((8, n))
            d1 = np.zeros(n); d2 = np.zeros(n); dist = np.zeros(n); d1A = np.zeros(n); distA = np.zeros(n)
            done = np.zeros(n, bool)
            last = np.zeros(n, np.uint32); med = np.full(n, NO_MEDIAN, np.uint32)
            m_alpha = np.full(n, np.inf); m_stop = np.full(n, np.inf); m_half = np.full(n, np.inf)
            lrgb = np.zeros((3, n))
            a, b = ranges[tile]
            for j, g in enumerate(point_list[a:b]):
                if done.all():
                    break
                v = v2g[g]
                # float32, the reference's order, no FMA
                n0 = (v[0] * rx + v[1] * ry) + v[2]
                n1 = (v[1] * rx + v[3] * ry) + v[4]
                n2 = (v[2] * rx + v[4] * ry) + v[5]
                AA = ((rx * n0 + ry * n1) + n2).astype(np.float64)
                BB = (two * ((v[6] * rx + v[7] * ry) + v[8])).astype(np.float64)
                CC = float(v[9])
                # float64 from here
                live = ~done
                t = -BB / (2.0 * AA)
                m_alpha = np.where(live, np.minimum(m_alpha, np.abs(t / NEAR - 1.0)), m_alpha)
                p1 = live & ~(t <= NEAR)
                power = np.minimum(-0.5 * (-(BB / AA) * (BB / 4.0) + CC), 0.0)
                alpha = np.minimum(ALPHA_MAX, float(opac[g]) * np.exp(power))
                m_alpha = np.where(p1, np.minimum(m_alpha, np.abs(alpha / ALPHA_MIN - 1.0)), m_alpha)
                p2 = p1 & ~(alpha < ALPHA_MIN)
                test_T = T * (1.0 - alpha)
                m_stop = np.where(p2, np.minimum(m_stop, np.abs(test_T / T_STOP - 1.0)), m_stop)
                stop = p2 & (test_T < T_STOP)
                done |= stop
                bl = p2 & ~stop
                if not bl.any():
                    continue
                m_half = np.where(bl, np.minimum(m_half, np.abs(T / 0.5 - 1.0)), m_half)
                w = np.where(bl, alpha * T, 0.0)
                mp = np.where(bl, (FAR * t - FAR * NEAR) / ((FAR - NEAR) * t), 0.0)
                f0, f1, f2 = n0.astype(np.float64), n1.astype(np.float64), n2.astype(np.float64)
                ln = np.sqrt(f0 * f0 + f1 * f1 + f2 * f2 + 1e-7)
                dist += (mp * mp * (1.0 - T) + d2 - 2.0 * mp * d1) * w
                distA += (mp * mp * (1.0 - T) + d2 + 2.0 * np.abs(mp) * d1A) * w
                d1 += mp * w; d1A += np.abs(mp) * w; d2 += mp * mp * w
                for ch in range(3):
                    term = float(rgb[g, ch]) * w
                    C[ch] += term; CA[ch] += np.abs(term)
                    lrgb[ch] = np.where(bl, term, lrgb[ch])
                for ch, f in ((3, f0), (4, f1), (5, f2)):
                    term = -f / ln * w
                    C[ch] += term; CA[ch] += np.abs(term)
                half = bl & (T > 0.5)
                C[6] = np.where(half, t, C[6])
                med = np.where(half, np.uint32(j + 1), med)
                C[7] += w
                T = np.where(bl, test_T, T)
                last = np.where(bl, np.uint32(j + 1), last)
            CA[6], CA[7] = np.abs(C[6]), C[7]
            C[:3] += T[None] * bg[:, None]; CA[:3] += T[None] * np.abs(bg)[:, None]
            norm = (1.0 - T) * (1.0 - T) + 1e-7
            out[:8, ys, xs] = C; A_out[:8, ys, xs] = CA
            out[8, ys, xs] = dist / norm; A_out[8, ys, xs] = distA / norm
            fT[:, ys, xs] = np.stack([T, d1, d2, dist]); A_T[:, ys, xs] = np.stack([T, d1A, d2, distA])
            ncon[0, ys, xs] = last; ncon[1, ys, xs] = med
            marg[:, ys, xs] = np.stack([m_alpha, m_stop, m_half])
            last_rgb[:, ys, xs] = lrgb
    keep = (marg[0] >= M_ALPHA) & (marg[1] >= M_STOP)
    return dict(out=out, final_T=fT, n_contrib=ncon, A_out=A_out, A_T=A_T, m_alpha=marg[0], m_stop=marg[1], m_half=marg[2],
                last_rgb=last_rgb, keep=keep, keep_depth=keep & (marg[2] >= M_HALF))


def k_stats(x, truth, A, keep):
    """(median, 99th percentile, maximum) over `keep` of K = |x - truth| / (2^-24 A); K = 0 where A = 0 and x = truth, inf where A = 0 and
    x != truth. `keep` [H,W] is broadcast over leading channel dimensions."""
    x, truth, A = np.asarray(x, np.float64), np.asarray(truth, np.float64), np.asarray(A, np.float64)
    keep = np.broadcast_to(keep, x.shape)
    err = np.abs(x - truth)[keep]
    a = A[keep]
    with np.errstate(all="ignore"):
        K = np.where(a > 0, err / (EPS * a), np.where(err == 0, 0.0, np.inf))
    if K.size == 0:
        return (0.0, 0.0, 0.0)
    return float(np.median(K)), float(np.percentile(K, 99)), float(K.max())


def _keep_of(truth, group):
    return truth["keep_depth"] if group == "depth" else truth["keep"]


def figures(truth, out, final_T=None):
    """K (median, p99, max) per group of an image [9,H,W] (and per final_T plane of [4,H,W]) over the truth's kept pixels."""
    fig = {g: k_stats(out[CHANNELS[g]], truth["out"][CHANNELS[g]], truth["A_out"][CHANNELS[g]], _keep_of(truth, g)) for g in GROUPS}
    if final_T is not None:
        for i, p in enumerate(PLANES):
            fig[p] = k_stats(final_T[i], truth["final_T"][i], truth["A_T"][i], truth["keep"])
    return fig


def check_bars(label, truth, fig, fig_oracle, m, failures, out, final_T=None, n_contrib=None, groups=None, show=True):
    """Section-4 bars of an output against the truth: every K statistic <= m x the oracle's for the same scene, group and statistic (no
    floor); exact zeros where A = 0; with n_contrib, the last contributor on every kept pixel and the median contributor on every pixel kept
    for depth. Appends (label, what, got, bar) to `failures`; prints kernel and oracle side by side."""
    for g in (groups or fig):
        for s, (kh, ko) in zip(("median", "p99", "max"), zip(fig[g], fig_oracle[g])):
            if not kh <= m * ko:
                failures.append((label, g, "K " + s, kh, m * ko))
        if show:
            print("%s %-10s K med / p99 / max  kernel %.2f / %.2f / %.1f   oracle %.2f / %.2f / %.1f" % ((label, g) + tuple(fig[g]) + tuple(fig_oracle[g])))
    pairs = [(g, out[CHANNELS[g]], truth["out"][CHANNELS[g]], truth["A_out"][CHANNELS[g]]) for g in GROUPS if groups is None or g in groups]
    if final_T is not None:
        pairs += [(p, final_T[i], truth["final_T"][i], truth["A_T"][i]) for i, p in enumerate(PLANES)]
    for g, x, t, a in pairs:
        z = (a == 0) & np.broadcast_to(_keep_of(truth, g), a.shape)
        if not np.array_equal(np.asarray(x, np.float64)[z], t[z]):
            failures.append((label, g, "exact zeros", int((np.asarray(x, np.float64)[z] != t[z]).sum()), 0))
    if n_contrib is not None:
        bad = int((n_contrib[0] != truth["n_contrib"][0])[truth["keep"]].sum())
        if bad:
            failures.append((label, "last contributor", "pixels that differ", bad, 0))
        bad = int((n_contrib[1] != truth["n_contrib"][1])[truth["keep_depth"]].sum())
        if bad:
            failures.append((label, "median contributor", "pixels that differ", bad, 0))


# ---- the scenes (the smallest at which each mechanism runs) ----------------------------------------------------------------------------------------

SCENES = {
    "tiny": dict(P=2000, res=(64, 64), s0=0.05, view="canonical"),                                           # F1
    "odd": dict(P=4000, res=(100, 72), s0=0.04, view="oblique"),                                             # partial tiles and quadrants
    "small_splats": dict(P=8000, res=(64, 64), s0=0.01, view="oblique"),                                     # the fragile regime
    "aniso_bg": dict(P=3000, res=(64, 48), s0=0.02, view="oblique", aniso=True, behind_fraction=0.05, bg=(0.2, 0.5, 0.7)),
    "filter_precomp": dict(P=3000, res=(96, 96), s0=0.05, view="oblique", kernel_size=0.1, scale_modifier=0.5, colors_precomp=True,
                           bg=(0.3, 0.1, 0.6)),
    "pixel_ordered": dict(P=4096, res=(64, 64), s0=0.01, view="oblique", pixel_ordered=True),
    "depth_spread": dict(P=800, res=(64, 64), s0=0.3, view="canonical", depth_range=(1.0, 30.0)),            # distortion up to 6e-4
    # (canonical: make_scene spreads the depths along world z, which is the view depth of the canonical camera only -- from the oblique camera
    # the same Gaussians give a channel that peaks at 9.5e-5; here 4,018 pixels exceed 1e-4, up to 2.9e-3, with lists of at most 202 entries)
    "deep": dict(P=600, res=(64, 64), s0=0.05, view="canonical", depth_range=(1.5, 20.0)),
    "wall": "wall", "mixed": "mixed",             # helpers.make_run_scene: lists of 876 / 1,358 entries, every run length of the scans
    "odd3": "odd",                                # make_run_scene("odd"): 73 x 41, three views in one call
    "thin": dict(P=6000, res=(73, 41), s0=0.03, view="oblique", seed=7),                                     # opacities x 0.04: 1,600-entry chains
}


@functools.lru_cache(maxsize=None)
def scene(name):
    import helpers
    kw = SCENES[name]
    if isinstance(kw, str):
        return helpers.make_run_scene(kw)
    sc = helpers.make_scene(**kw)
    if name == "thin":
        sc["opacities"] = sc["opacities"] * 0.04      # nothing saturates
    return sc


def n_views(name):
    return scene(name)["viewmatrix"].shape[0]


@functools.lru_cache(maxsize=None)
def oracle(name, view=0):
    """The CPU oracle's run of one view: its outputs and intermediates (helpers.run_oracle), rgb filled in when colours are given."""
    import helpers
    sc = scene(name)
    o = helpers.run_oracle(sc, view=view)
    o.pop("oracle")
    if sc["colors_precomp"] is not None:
        o["rgb"] = sc["colors_precomp"].numpy().astype(np.float32)
    return o


def truth_of(name, records, point_list, ranges):
    sc = scene(name)
    return blend_truth(records, point_list, ranges, sc["W"], sc["H"], sc["tanfovx"], sc["tanfovy"], sc["bg"].numpy())


@functools.lru_cache(maxsize=None)
def oracle_truth(name, view=0):
    """The truth on the ORACLE's records and lists, and the oracle's own figures against it. A kernel whose exported records and lists are
    bit-equal to the oracle's on the visible Gaussians (asserted by the GPU module) has this very truth."""
    o = oracle(name, view)
    t = truth_of(name, dict(view2gaussian=o["view2gaussian"], opac=o["conic_opacity"][:, 3], rgb=o["rgb"]), o["point_list"], o["ranges"])
    return t, figures(t, o["out_color"], o["final_T"])


def assert_inputs_are_the_oracles(label, h, oracles):
    """Records, list and ranges exported from a call (helpers.run_hip / export_workspace), bit for bit the oracle's of every view (`oracles`:
    helpers.run_oracle's results, one per view) on the visible Gaussians: the truth of the oracle's records is then this call's truth."""
    total = 0
    for v, o in enumerate(oracles):
        vis = o["radii"] > 0
        assert np.array_equal(h["radii"][v] > 0, vis), (label, v)
        for k, a, b in (("view2gaussian", h["view2gaussian"][v], o["view2gaussian"]), ("opacity*coef", h["opac"][v], o["conic_opacity"][:, 3]),
                        ("rgb", h["rgb"][v], o["rgb"])):
            assert np.array_equal(np.ascontiguousarray(a[vis]).view(np.uint32), np.ascontiguousarray(b[vis]).view(np.uint32)), (label, v, k)
        R = o["num_rendered"]
        assert np.array_equal(h["point_list"][total:total + R], o["point_list"]), (label, v, "point list")
        r = h["ranges"][v].astype(np.int64)
        assert np.array_equal(r - total * (r.sum(1, keepdims=True) > 0), o["ranges"].astype(np.int64)), (label, v, "ranges")
        total += R
    assert total == h["num_rendered"], label
