"""Non-finite containment of the compositing kernels, forward and backward, against the CPU oracle.

In the reference a non-finite value reaches only what depends on it: an Inf / NaN colour of Gaussian g only the pixels g is blended
into, a NaN of dL_dpixels at pixel p only the gradients of the Gaussians blended at p. A kernel that multiplies a value it should have
skipped by a zero weight (Inf * 0 = NaN), or gates a scan step by multiplying with a 0 / 1 flag, leaks it into pixels or Gaussians the
reference leaves finite. Masking is not a fix: where the reference turns the value into Inf / NaN the kernel must too.

Forward cells and the kernel each one reaches (f3dg_debug_last_render_kernel, asserted per call):
    fast_general        fast, 3 views, general path, render_lowocc 0        render3s_fwd_kernel
    exact_aux_packed    exact + SAVE_AUX, default packing                   render4_fwd_kernel (rank-packed)
    fast_pack1          render_pack 1, fast                                 render4_fwd_kernel<FAST=true> (f3dg_pair_apply_flat trips)
    exact_pack0         render_pack 0, exact                                render3s_fwd_kernel<FAST=false>
    scan_th12 / _th64   F3DG_FLAG_SCAN, render_scan_th 12 / 64              render5_fwd_kernel
    one_view_fast       one view, fast, small-call path                     render3p_fwd_kernel
    one_view_exact      one view, exact, small-call path                    render3q_fwd_kernel
    two_views           two views, fast, small-call path                    render3p_fwd_kernel
    scan_small          render_scan 1, one view                             render5p_fwd_kernel
    lean_channels       SKIP_NORMAL | SKIP_DISTORTION, 3 views              render3s_fwd_kernel<NORMAL=false, DIST=false>
    fast_save_aux       FAST | SAVE_AUX, 3 views                            render3s_fwd_kernel<SAVE_AUX=true, FAST=true>
"""
import numpy as np
import pytest
import torch

import f3dgaus_amd as f3d
from f3dgaus_amd import _lib
from f3dgaus_amd.diff_gof_rasterization.backward import rasterize_backward_raw
from helpers import make_scene, run_oracle

pytestmark = pytest.mark.gpu

DEFAULTS = {"render_lowocc": 1, "render_pack": -1, "render_scan": -1, "render_scan_th": 12, "bwd_dense": 1, "small_path_aux": 1}


def _scene(V, seed=21):
    # 72 x 56: partial tiles and quadrants on the right and bottom edges
    return make_scene(P=3000, res=(72, 56), s0=0.05, view="oblique", n_views=V, seed=seed, colors_precomp=True, bg=(0.2, 0.5, 0.1))


def _set(opts):
    L = _lib.lib()
    for k, v in opts.items():
        assert L.f3dg_set_option(k.encode(), v) == 0, k


def _reset(opts):
    L = _lib.lib()
    for k in opts:
        L.f3dg_set_option(k.encode(), DEFAULTS[k])


def _forward(scene, device, colors, kw, save_aux=False):
    dev = lambda t: None if t is None else t.to(device)
    V, H, W = scene["viewmatrix"].shape[0], scene["H"], scene["W"]
    out, radii, ws = f3d.rasterize_views(
        dev(scene["means3D"]), dev(scene["opacities"]), dev(scene["viewmatrix"]), dev(scene["projmatrix"]), dev(scene["campos"]),
        dev(scene["bg"]), image_height=H, image_width=W, tanfovx=scene["tanfovx"], tanfovy=scene["tanfovy"], sh=None,
        colors_precomp=colors.to(device), scales=dev(scene["scales"]), rotations=dev(scene["rotations"]), sh_degree=scene["sh_degree"],
        scale_modifier=scene["scale_modifier"], kernel_size=scene["kernel_size"], save_aux=save_aux,
        out=torch.zeros((V, 9, H, W), device=device), **kw)
    torch.cuda.synchronize()
    return out, radii, ws


def _pick_gaussians(scene):
    """One large footprint deep in its tiles, one centred on a quadrant's last column (x % 8 = 7), one near a tile corner; each the
    first of its candidates that the oracle blends somewhere."""
    o = run_oracle(scene, view=0)
    r, m, d = o["radii"], o["means2D"], o["depths"]
    W, H, V = scene["W"], scene["H"], scene["viewmatrix"].shape[0]
    vis = (r > 0) & (m[:, 0] >= 0) & (m[:, 0] < W) & (m[:, 1] >= 0) & (m[:, 1] < H)
    ids = np.nonzero(vis)[0]
    big = ids[r[ids] >= np.quantile(r[ids], 0.9)]
    q = ids[(np.floor(m[ids, 0]).astype(int) % 8 == 7) & (r[ids] >= 3)]
    corner = np.hypot(m[ids, 0] - 16 * np.round(m[ids, 0] / 16), m[ids, 1] - 16 * np.round(m[ids, 1] / 16))
    picks = []
    for cand in (big[np.argsort(-d[big])], q[np.argsort(r[q])], ids[np.argsort(corner)]):
        picks.append(next(int(g) for g in cand if _oracle_reached(scene, V, int(g)).any()))
    return picks


FWD_CELLS = {
    "fast_general": (3, dict(exact=False, small_path=False), {"render_lowocc": 0}, False, "render3s_fwd_kernel<SAVE_AUX=false, FAST=true"),
    "exact_aux_packed": (3, dict(exact=True, small_path=False), {"render_lowocc": 0}, True, "render4_fwd_kernel<FAST=false"),
    "fast_pack1": (3, dict(exact=False, small_path=False), {"render_lowocc": 0, "render_pack": 1}, False, "render4_fwd_kernel<FAST=true"),
    "exact_pack0": (3, dict(exact=True, small_path=False), {"render_lowocc": 0, "render_pack": 0}, False, "render3s_fwd_kernel<SAVE_AUX=false, FAST=false"),
    "scan_th12": (3, dict(exact=False, small_path=False, scan=True), {"render_lowocc": 0, "render_scan_th": 12}, False, "render5_fwd_kernel"),
    "scan_th64": (3, dict(exact=False, small_path=False, scan=True), {"render_lowocc": 0, "render_scan_th": 64}, False, "render5_fwd_kernel"),
    "one_view_fast": (1, dict(exact=False), {}, False, "render3p_fwd_kernel"),
    "one_view_exact": (1, dict(exact=True), {}, False, "render3q_fwd_kernel"),
    "two_views": (2, dict(exact=False), {}, False, "render3p_fwd_kernel"),
    "scan_small": (1, dict(exact=False), {"render_scan": 1}, False, "render5p_fwd_kernel"),
    "lean_channels": (3, dict(exact=False, small_path=False, channels="rgb_depth_alpha"), {"render_lowocc": 0}, False, "NORMAL=false, DIST=false"),
    "fast_save_aux": (3, dict(exact=False, small_path=False), {"render_lowocc": 0}, True, "render3s_fwd_kernel<SAVE_AUX=true, FAST=true"),
}

_ORACLE_REACH = {}


def _oracle_reached(scene, V, g):
    """The oracle's reached set of Gaussian g per view: pixels whose RGB moves when g's colour goes from 0 to 1000."""
    key = (V, g)
    if key not in _ORACLE_REACH:
        reach = []
        for v in range(V):
            outs = []
            for val in (0.0, 1000.0):
                sc = dict(scene)
                sc["colors_precomp"] = scene["colors_precomp"].clone()
                sc["colors_precomp"][g] = val
                outs.append(run_oracle(sc, view=v)["out_color"])
            reach.append((outs[0][:3] != outs[1][:3]).any(0))
        _ORACLE_REACH[key] = np.stack(reach)
    return _ORACLE_REACH[key]


@pytest.mark.parametrize("cell", list(FWD_CELLS))
def test_nonfinite_colour_stays_in_its_pixels(cell, gpu_device):
    V, kw, opts, save_aux, kernel = FWD_CELLS[cell]
    scene = _scene(V)
    L = _lib.lib()
    written = [0, 1, 2, 6, 7] if kw.get("channels") == "rgb_depth_alpha" else list(range(9))
    bits = lambda a: a.view(np.uint32)
    _set(opts)
    try:
        for g in _pick_gaussians(scene):
            def render(col):
                c = scene["colors_precomp"].clone()
                c[g] = torch.tensor(col, dtype=torch.float32)
                out, _, _ = _forward(scene, gpu_device, c, kw, save_aux)
                name = L.f3dg_debug_last_render_kernel().decode()
                assert kernel in name, (cell, name)
                return out.cpu().numpy()
            base = render([0.0, 0.0, 0.0])
            reach = (base[:, :3] != render([1000.0, 1000.0, 1000.0])[:, :3]).any(1)           # [V, H, W]
            assert reach.any(), (cell, g)
            ora = _oracle_reached(scene, V, g)
            flips = int((reach != ora).sum())
            assert flips <= 1e-3 * reach.size, (cell, g, flips)
            for ch in range(3):
                for val in (float("inf"), float("nan")):
                    col = [0.0, 0.0, 0.0]
                    col[ch] = val
                    out = render(col)
                    bad = ~np.isfinite(out[:, ch])
                    assert np.array_equal(bad, reach), (cell, g, ch, val, int((bad & ~reach).sum()), int((reach & ~bad).sum()))
                    for c in written:
                        if c == ch:
                            assert np.array_equal(bits(out[:, c][~reach]), bits(base[:, c][~reach])), (cell, g, ch, val)
                        else:
                            assert np.array_equal(bits(out[:, c]), bits(base[:, c])), (cell, g, ch, val, c)
    finally:
        _reset(opts)


# ---- backward --------------------------------------------------------------------------------------------------------------------------

BWD_CELLS = {
    "dense_exact_3v": (3, dict(exact=True, small_path=False), {"bwd_dense": 1}),
    "walk_exact_3v": (3, dict(exact=True, small_path=False), {"bwd_dense": 0}),
    "dense_fast_aux_3v": (3, dict(exact=False, small_path=False), {"bwd_dense": 1}),
    "walk_fast_aux_3v": (3, dict(exact=False, small_path=False), {"bwd_dense": 0}),
    "dense_small_path_1v": (1, dict(exact=True), {"bwd_dense": 1, "small_path_aux": 1}),
    "walk_small_path_1v": (1, dict(exact=True), {"bwd_dense": 0, "small_path_aux": 1}),
}
PER_VIEW = ("dL_dview2gaussian", "dL_dcolors", "dL_dmeans2D")
SUMMED = ("dL_dopacity", "dL_dmeans3D", "dL_dscales", "dL_drotations")
ORACLE_NAME = {"dL_dview2gaussian": "dL_dview2gaussian", "dL_dcolors": "dL_dcolor", "dL_dmeans2D": "dL_dmean2D", "dL_dopacity": "dL_dopacity",
               "dL_dmeans3D": "dL_dmean3D", "dL_dscales": "dL_dscale", "dL_drotations": "dL_drot"}


def _pick_pixels(o, W, H):
    """The pixel with the most blended entries, the deepest quadrant corner (x % 8 = 7, y % 8 = 7), and a tile corner."""
    nc = o["n_contrib"][0].astype(np.int64)
    deep = np.unravel_index(np.argmax(nc), nc.shape)
    qc = nc.copy()
    mask = np.zeros_like(qc, bool)
    mask[7::8, 7::8] = True
    qc[~mask] = -1
    quad = np.unravel_index(np.argmax(qc), nc.shape)
    return [(int(deep[0]), int(deep[1])), (int(quad[0]), int(quad[1])), (15, 16)]


@pytest.mark.parametrize("cell", list(BWD_CELLS))
def test_nonfinite_pixel_gradient_stays_in_its_gaussians(cell, gpu_device):
    V, kw, opts = BWD_CELLS[cell]
    scene = _scene(V, seed=23)
    H, W, P = scene["H"], scene["W"], scene["P"]
    v = V - 1                                  # the view that gets the NaN
    dev = lambda t: None if t is None else t.to(gpu_device)
    _set(opts)
    try:
        _, radii, ws = _forward(scene, gpu_device, scene["colors_precomp"], kw, save_aux=True)

        def backward(dpix):
            g = rasterize_backward_raw(ws, dev(scene["means3D"]), None, dev(scene["colors_precomp"]), dev(scene["scales"]), dev(scene["rotations"]),
                                       radii, torch.from_numpy(dpix).to(gpu_device), scene["sh_degree"], dev(scene["viewmatrix"]),
                                       dev(scene["projmatrix"]), dev(scene["campos"]), dev(scene["bg"]), scene["tanfovx"], scene["tanfovy"],
                                       scene["kernel_size"], scene["scale_modifier"])
            torch.cuda.synchronize()
            return {k: g[k].cpu().numpy() for k in PER_VIEW + SUMMED}

        o = run_oracle(scene, view=v)
        rng = np.random.default_rng(31)
        dpix = rng.standard_normal((V, 9, H, W)).astype(np.float32)

        # the alpha plane is never read (backward.cu): NaN there gives the gradients of a zero plane
        z, n = dpix.copy(), dpix.copy()
        z[:, 7] = 0.0
        n[:, 7] = np.nan
        gz, gn = backward(z), backward(n)
        for k in gz:
            assert np.isfinite(gn[k]).all(), (cell, "alpha plane", k)
            m = np.abs(gz[k]).max()
            assert np.abs(gn[k] - gz[k]).max() <= 1e-5 * m, (cell, "alpha plane", k)

        for (py, px) in _pick_pixels(o, W, H):
            # S(p): the Gaussians with a nonzero colour gradient under a one-hot dL_dpixels at p (nonzero for every blended pair)
            one = np.zeros_like(dpix)
            one[v, 0, py, px] = 1.0
            gk = backward(one)["dL_dcolors"][v, :, 0]
            go = o["oracle"].backward(one[v])["dL_dcolor"][:, 0]
            S = gk != 0
            assert S.any(), (cell, py, px)
            diff = S != (go != 0)
            thr = 1e-6 * max(np.abs(go).max(), np.abs(gk).max())
            assert (np.maximum(np.abs(gk), np.abs(go))[diff] < thr).all(), (cell, py, px, np.nonzero(diff)[0])
            S = S | (go != 0)

            zero = dpix.copy()
            zero[v, :, py, px] = 0.0
            gz = backward(zero)
            for c in (0, 3, 6, 8):
                bad = dpix.copy()
                bad[v, c, py, px] = np.nan
                gb = backward(bad)
                ob = o["oracle"].backward(bad[v])
                for k in PER_VIEW + SUMMED:
                    got, ref = gb[k], gz[k]
                    m = np.abs(ref).max()
                    if k in PER_VIEW:
                        # other views: untouched everywhere; view v: untouched outside S(p)
                        others = [u for u in range(V) if u != v]
                        assert np.isfinite(got[others]).all(), (cell, c, k, "other views")
                        assert np.abs(got[others] - ref[others]).max(initial=0.0) <= 1e-5 * m, (cell, c, k, "other views")
                        got_v, ref_v = got[v], ref[v]
                    else:
                        got_v, ref_v = got, ref
                    assert np.isfinite(got_v[~S]).all(), (cell, (py, px), c, k, np.nonzero(~np.isfinite(got_v).all(-1) & ~S)[0][:8])
                    if k in ("dL_dview2gaussian", "dL_dopacity", "dL_dcolors", "dL_dmeans2D"):
                        assert np.abs(got_v[~S] - ref_v[~S]).max() <= 1e-5 * m, (cell, (py, px), c, k)
                    # inside S(p): non-finite exactly where the reference is
                    fin_o = np.isfinite(ob[ORACLE_NAME[k]].reshape(P, -1)[S])
                    fin_k = np.isfinite(got_v.reshape(P, -1)[S][:, :fin_o.shape[1]])
                    assert np.array_equal(fin_k, fin_o), (cell, (py, px), c, k, int((fin_k != fin_o).sum()))
    finally:
        _reset(opts)
