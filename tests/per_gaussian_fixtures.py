"""Well-conditioned scenes for the per-Gaussian stage of the backward (preprocess_bwd_kernel), shared by
tests/test_per_gaussian_backward.py (CPU: the oracle and the conditions) and tests/test_per_gaussian_backward_gpu.py.

Large splats (sigma0 0.12 .. 0.2): the float32 error of the chain rule against its float64 statement stays at 1e-5 .. 1e-3 of the
gradient's maximum, where the sigma0 = 0.02 .. 0.05 scenes of tests/test_raster_backward_gpu.py sit at 1e-2 .. 0.4. The oracle's side
(its backward per view summed in float32 in view order, the float64 truth from its own per-view dL_dview2gaussian / dL_dcolor, the
term magnitude A and the error figures) is computed once per scene and shared; nothing here is modified by a test."""
import numpy as np

from grad_truth import per_gaussian_term_magnitude, per_gaussian_truth_views
from helpers import make_scene, run_oracle

GROUPS = ("dL_dmean3D", "dL_drot", "dL_dscale")
HIP_KEY = dict(dL_dmean3D="dL_dmeans3D", dL_drot="dL_drotations", dL_dscale="dL_dscales", dL_dsh="dL_dsh")
EPS = 2.0 ** -24
_CACHE = {}


def _stretched(scene):
    """means3D x2 about their mean in x and y: part of the cloud leaves the image, in some views or in all of them."""
    m = scene["means3D"]
    c = m.mean(0)
    m2 = m.clone()
    m2[:, :2] = c[:2] + 2.0 * (m[:, :2] - c[:2])
    scene["means3D"] = m2.contiguous()
    return scene


def _degree_below_storage(scene):
    scene["sh_degree"] = 1          # D = 1 active of M = 16 stored
    return scene


_BUILD = {
    "oblique_deg1": lambda: make_scene(P=600, res=(64, 64), s0=0.2, view="oblique", sh_degree=1),
    "odd_deg3": lambda: make_scene(P=700, res=(49, 37), s0=0.15, view="oblique", sh_degree=3),
    "odd_deg1_of_16": lambda: _degree_below_storage(make_scene(P=700, res=(49, 37), s0=0.15, view="oblique", sh_degree=3)),
    "precomp": lambda: make_scene(P=600, res=(64, 64), s0=0.2, view="oblique", colors_precomp=True),
    "three_views": lambda: _stretched(make_scene(P=900, res=(64, 64), s0=0.12, view=[1, 4, 7], sh_degree=2)),
    # not among the five of the table: the second set of the two-set run, and the scene of the add-into test
    "three_views_seed1": lambda: _stretched(make_scene(P=900, res=(64, 64), s0=0.12, seed=1, view=[1, 4, 7], sh_degree=2)),
    "odd_deg1_of_16_stretched": lambda: _stretched(_degree_below_storage(make_scene(P=700, res=(49, 37), s0=0.15, view="oblique", sh_degree=3))),
}
FIXTURES = ("oblique_deg1", "odd_deg3", "odd_deg1_of_16", "precomp", "three_views")
EXTRA = ("three_views_seed1", "odd_deg1_of_16_stretched")


def scene(name):
    if ("scene", name) not in _CACHE:
        _CACHE["scene", name] = _BUILD[name]()
    return _CACHE["scene", name]


def dpix(name):
    """default_rng(5).standard_normal over all nine channels; the second set of the two-set run takes the second half of the six views'."""
    sc = scene(name)
    V = sc["viewmatrix"].shape[0]
    if name == "three_views_seed1":
        return np.random.default_rng(5).standard_normal((2 * V, 9, sc["H"], sc["W"])).astype(np.float32)[V:]
    return np.random.default_rng(5).standard_normal((V, 9, sc["H"], sc["W"])).astype(np.float32)


def rel(a, b):
    """max|a - b| / max|b|."""
    m = np.abs(b).max()
    return 0.0 if m == 0 else float(np.abs(np.asarray(a, np.float64) - b).max() / m)


def k_stats(g, truth, A, seen):
    """K = |g - truth| / (2^-24 * A) over the elements of the Gaussians some view sees: (median, 99th percentile, maximum).
    An element without any term (A = 0) has to be exact."""
    err = np.abs(np.asarray(g, np.float64) - truth)[seen].ravel()
    a = A[seen].ravel() * EPS
    k = np.where(err == 0, 0.0, err / np.where(a > 0, a, 1.0))
    k[(a == 0) & (err > 0)] = np.inf
    return float(np.median(k)), float(np.percentile(k, 99)), float(k.max())


def oracle_reference(name):
    """The oracle on one scene: per-view radii / clamped / dL_dview2gaussian / dL_dcolor, the per-Gaussian gradients summed over the
    views in float32 in view order, the truth from those per-view arrays, A, e_o = rel(oracle, truth) and the oracle's K statistics."""
    if ("ref", name) in _CACHE:
        return _CACHE["ref", name]
    sc, d = scene(name), dpix(name)
    V = sc["viewmatrix"].shape[0]
    radii, clamped, dv2g, dcol, g = [], [], [], [], None
    for v in range(V):
        o = run_oracle(sc, view=v)
        go = o["oracle"].backward(d[v])
        radii.append(o["radii"]); clamped.append(o["clamped"]); dv2g.append(go["dL_dview2gaussian"]); dcol.append(go["dL_dcolor"])
        part = {k: go[k] for k in GROUPS + ("dL_dsh",)}
        g = part if g is None else {k: g[k] + part[k] for k in g}           # float32 + float32
    assert all(a.dtype == np.float32 for a in g.values())
    if sc["shs"] is None:
        g["dL_dsh"] = None
    radii, clamped, dv2g, dcol = np.stack(radii), np.stack(clamped), np.stack(dv2g), np.stack(dcol)
    truth = per_gaussian_truth_views(sc, range(V), radii, dv2g, dcol)
    A = per_gaussian_term_magnitude(sc, range(V), radii, dv2g, dcol)
    seen = (radii > 0).any(0)
    keys = GROUPS + (("dL_dsh",) if sc["shs"] is not None else ())
    ref = dict(radii=radii, clamped=clamped, dL_dview2gaussian=dv2g, dL_dcolor=dcol, g=g, truth=truth, A=A, seen=seen,
               e_o={k: rel(g[k], truth[k]) for k in keys}, K={k: k_stats(g[k], truth[k], A[k], seen) for k in GROUPS})
    _CACHE["ref", name] = ref
    return ref
