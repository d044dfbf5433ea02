"""Float64 truth of the per-Gaussian contribution statistics ON THE COMPOSITING INPUTS, and the float32 yardstick beside it. Test
infrastructure only (numpy), in the style of compositing_truth.blend_truth, whose constants and inputs these are.

For a pair (pixel, entry g of the pixel's tile list), walked in list order from T = 1:
    skipped   the pixel is done, or t <= 0.2, or alpha < 1/255;
    stopper   not skipped and T (1 - alpha) < 0.0001f: the pixel is done, stops[g] += 1;
    blended   otherwise: w = alpha T, blended[g] += 1, max_w[g] = max(., w), sum_w[g] += w, T = T (1 - alpha).

contribution_truth  normal[3], AA, BB in float32 in the reference's order (they count as inputs, as in blend_truth), everything after in
                    float64. A float32 implementation may decide a pair the other way when it comes within a few ulp of a test, and from
                    then on that pixel's T, and so every later decision of the pixel, may differ. So a pixel becomes DIRTY at the first
                    entry (of a pixel the truth has not finished) that comes within M_ALPHA of the t or the alpha test or within M_STOP
                    of the stop; that pair and every later pair of the pixel that could pass the stateless tests
                    (t > 0.2 (1 - M_ALPHA) and alpha >= (1/255) (1 - M_ALPHA)) is UNCERTAIN, whether the truth has finished the pixel
                    or not. blended / stops / max_w / sum_w count the CERTAIN pairs only, uncertain[g] the others: an implementation's
                    counter lies in [certain, certain + uncertain], and a Gaussian with uncertain == 0 is CLEAN: its statistics are
                    the truth's.
contribution_replay the same walk in float32 in the reference's operation order (gof_oracle.c:493-547: no FMA, the double island
                    -BB / (2 AA), min_value in float64), expf as the correctly rounded float32 of the float64 exponential. It plays the
                    part the CPU oracle plays for images. Its sum is the fixed-point one of the library: round(w 2^32) per pair in a
                    64-bit integer."""
import functools

import numpy as np

import compositing_truth as CT

FIXED = 4294967296.0


def _inputs(records, point_list, ranges, W, H, tanfovx, tanfovy):
    v2g, opac = CT._f32(records["view2gaussian"]), CT._f32(records["opac"]).reshape(-1)
    point_list = np.asarray(point_list).astype(np.int64)
    ranges = np.asarray(ranges).astype(np.int64).reshape(-1, 2)
    gx, gy = (W + 15) // 16, (H + 15) // 16
    assert ranges.shape[0] == gx * gy
    rx_all, ry_all = CT.rays(W, H, tanfovx, tanfovy)
    return v2g, opac, point_list, ranges, gx, gy, rx_all, ry_all


def _tile_pixels(tile, gx, W, H):
    x0, y0 = (tile % gx) * 16, (tile // gx) * 16
    ys, xs = np.meshgrid(np.arange(y0, min(y0 + 16, H)), np.arange(x0, min(x0 + 16, W)), indexing="ij")
    return ys.ravel(), xs.ravel()


def _quadratic_f32(v, rx, ry):
    """normal[3], AA, BB of forward.cu:500-509 in float32, the reference's order, no FMA."""
    n0 = (v[0] * rx + v[1] * ry) + v[2]
    n1 = (v[1] * rx + v[3] * ry) + v[4]
    n2 = (v[2] * rx + v[4] * ry) + v[5]
    AA = (rx * n0 + ry * n1) + n2
    BB = np.float32(2.0) * ((v[6] * rx + v[7] * ry) + v[8])
    return AA, BB


def contribution_truth(records, point_list, ranges, W, H, tanfovx, tanfovy):
    """records: dict(view2gaussian [P,10], opac [P]) float32; point_list [R]; ranges [tiles,2]. Returns per Gaussian (arrays [P]):
    blended, stops (int64, certain pairs), max_w, sum_w (float64, certain pairs), uncertain (int64); and final_T [H,W] float64,
    n_last [H,W] (1-based position of the last blended entry, 0: none), dirty [H,W] bool."""
    v2g, opac, point_list, ranges, gx, gy, rx_all, ry_all = _inputs(records, point_list, ranges, W, H, tanfovx, tanfovy)
    P = v2g.shape[0]
    blended, stops, uncertain = np.zeros(P, np.int64), np.zeros(P, np.int64), np.zeros(P, np.int64)
    max_w, sum_w = np.zeros(P), np.zeros(P)
    final_T, n_last, dirty_map = np.ones((H, W)), np.zeros((H, W), np.int64), np.zeros((H, W), bool)
    with np.errstate(all="ignore"):
        for tile in range(gx * gy):
            ys, xs = _tile_pixels(tile, gx, W, H)
            rx, ry = rx_all[xs], ry_all[ys]
            n = xs.size
            T = np.ones(n); done = np.zeros(n, bool); dirty = np.zeros(n, bool); last = np.zeros(n, np.int64)
            a, b = ranges[tile]
            for j, g in enumerate(point_list[a:b]):
                if (done & ~dirty).all():
                    break
                AA32, BB32 = _quadratic_f32(v2g[g], rx, ry)
                AA, BB = AA32.astype(np.float64), BB32.astype(np.float64)
                t = -BB / (2.0 * AA)
                power = np.minimum(-0.5 * (-(BB / AA) * (BB / 4.0) + float(v2g[g][9])), 0.0)
                alpha = np.minimum(CT.ALPHA_MAX, float(opac[g]) * np.exp(power))
                live = ~done
                p1 = live & ~(t <= CT.NEAR)
                p2 = p1 & ~(alpha < CT.ALPHA_MIN)
                test_T = T * (1.0 - alpha)
                near = live & (np.abs(t / CT.NEAR - 1.0) < CT.M_ALPHA)
                near |= p1 & (np.abs(alpha / CT.ALPHA_MIN - 1.0) < CT.M_ALPHA)
                near |= p2 & (np.abs(test_T / CT.T_STOP - 1.0) < CT.M_STOP)
                dirty |= near
                could = (t > CT.NEAR * (1.0 - CT.M_ALPHA)) & (alpha >= CT.ALPHA_MIN * (1.0 - CT.M_ALPHA))
                uncertain[g] += int((dirty & could).sum())
                stop = p2 & (test_T < CT.T_STOP)
                bl = p2 & ~stop
                sure = ~dirty
                stops[g] += int((stop & sure).sum())
                cb = bl & sure
                if cb.any():
                    w = alpha[cb] * T[cb]
                    blended[g] += int(cb.sum())
                    max_w[g] = max(max_w[g], float(w.max()))
                    sum_w[g] += float(w.sum())
                done |= stop
                T = np.where(bl, test_T, T)
                last = np.where(bl, j + 1, last)
            final_T[ys, xs] = T; n_last[ys, xs] = last; dirty_map[ys, xs] = dirty
    return dict(blended=blended, stops=stops, max_w=max_w, sum_w=sum_w, uncertain=uncertain, final_T=final_T, n_last=n_last, dirty=dirty_map)


def contribution_replay(records, point_list, ranges, W, H, tanfovx, tanfovy):
    """The float32 walk in the reference's operation order. Returns per Gaussian blended, stops (int64), max_w (float32), sum_fixed
    (uint64: sum of round(w 2^32)), sum_w (float64 = sum_fixed / 2^32); final_T [H,W] float32."""
    v2g, opac, point_list, ranges, gx, gy, rx_all, ry_all = _inputs(records, point_list, ranges, W, H, tanfovx, tanfovy)
    P = v2g.shape[0]
    f32 = np.float32
    blended, stops = np.zeros(P, np.int64), np.zeros(P, np.int64)
    max_w, sum_fixed = np.zeros(P, f32), np.zeros(P, np.uint64)
    final_T = np.ones((H, W), f32)
    with np.errstate(all="ignore"):
        for tile in range(gx * gy):
            ys, xs = _tile_pixels(tile, gx, W, H)
            rx, ry = rx_all[xs], ry_all[ys]
            n = xs.size
            T = np.ones(n, f32); done = np.zeros(n, bool)
            a, b = ranges[tile]
            for g in point_list[a:b]:
                if done.all():
                    break
                AA32, BB32 = _quadratic_f32(v2g[g], rx, ry)
                AA, BB = AA32.astype(np.float64), BB32.astype(np.float64)
                t = (-BB / (2.0 * AA)).astype(f32)
                p1 = ~done & ~(t.astype(np.float64) <= CT.NEAR)
                min_value = -(BB / AA) * (BB / 4.0) + np.float64(v2g[g][9])
                power = (np.float64(f32(-0.5)) * min_value).astype(f32)
                power = np.where(power > f32(0.0), f32(0.0), power)
                alpha = np.minimum(f32(0.99), opac[g] * np.exp(power.astype(np.float64)).astype(f32))
                p2 = p1 & ~(alpha < f32(1.0) / f32(255.0))
                test_T = T * (f32(1.0) - alpha)
                stop = p2 & (test_T < f32(0.0001))
                bl = p2 & ~stop
                stops[g] += int(stop.sum())
                if bl.any():
                    w = alpha[bl] * T[bl]
                    assert w.dtype == f32
                    blended[g] += int(bl.sum())
                    max_w[g] = max(max_w[g], w.max())
                    sum_fixed[g] += np.rint(w.astype(np.float64) * FIXED).astype(np.uint64).sum(dtype=np.uint64)
                done |= stop
                T = np.where(bl, test_T, T)
            final_T[ys, xs] = T
    return dict(blended=blended, stops=stops, max_w=max_w, sum_fixed=sum_fixed, sum_w=sum_fixed.astype(np.float64) / FIXED, final_T=final_T)


def _records(o):
    return dict(view2gaussian=o["view2gaussian"], opac=o["conic_opacity"][:, 3])


@functools.lru_cache(maxsize=None)
def oracle_truth(name, view=0):
    """The truth on the oracle's records and lists of one view of a compositing_truth scene."""
    sc, o = CT.scene(name), CT.oracle(name, view)
    return contribution_truth(_records(o), o["point_list"], o["ranges"], sc["W"], sc["H"], sc["tanfovx"], sc["tanfovy"])


@functools.lru_cache(maxsize=None)
def oracle_replay(name, view=0):
    sc, o = CT.scene(name), CT.oracle(name, view)
    return contribution_replay(_records(o), o["point_list"], o["ranges"], sc["W"], sc["H"], sc["tanfovx"], sc["tanfovy"])


def replay_counts(name):
    """blended, stops of the replay summed over the scene's views."""
    rs = [oracle_replay(name, v) for v in range(CT.n_views(name))]
    return sum(r["blended"] for r in rs), sum(r["stops"] for r in rs)


def prune_scene(sc, keep):
    """The scene with the Gaussians of the boolean mask `keep` only, in their order."""
    import torch
    idx = torch.from_numpy(np.nonzero(keep)[0])
    out = dict(sc)
    for k in ("means3D", "opacities", "scales", "rotations", "shs", "colors_precomp"):
        if sc[k] is not None:
            out[k] = sc[k][idx].contiguous()
    out["P"] = int(idx.numel())
    return out


# ---- the bars of an implementation's max_weight / sum_weight against the truth --------------------------------------------------------
REL_FLOOR = 2.0 ** -23          # one float32 ulp, relative
FIXED_ULP = 2.0 ** -33          # half a unit of the fixed point per pair, absolute on the sum


def clean_touched(truth):
    """Gaussians whose statistics are the truth's (no uncertain pair) and that have a blended pair to compare."""
    return (truth["uncertain"] == 0) & (truth["blended"] > 0)


def rel_stats(x, ref, slack=None):
    """(median, 99th percentile, maximum) of max(|x - ref| - slack, 0) / ref."""
    x, ref = np.asarray(x, np.float64), np.asarray(ref, np.float64)
    if x.size == 0:
        return (0.0, 0.0, 0.0)
    err = np.abs(x - ref)
    if slack is not None:
        err = np.maximum(err - slack, 0.0)
    r = err / ref
    return float(np.median(r)), float(np.percentile(r, 99)), float(r.max())


def weight_figures(truth, max_w, sum_w):
    """Relative-error statistics of an implementation's max_weight and sum_weight [P] on the clean touched Gaussians; the sum's absolute
    error is first relieved of blended x 2^-33, the rounding of the fixed point."""
    m = clean_touched(truth)
    return dict(max_weight=rel_stats(np.asarray(max_w)[m], truth["max_w"][m]),
                sum_weight=rel_stats(np.asarray(sum_w)[m], truth["sum_w"][m], truth["blended"][m] * FIXED_ULP))
