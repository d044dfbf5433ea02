"""Fixtures, cotangent groups, output groups and the shared CPU references of the per-channel checks of the compositing backward
(tests/test_oracle_backward_channels.py, tests/test_raster_backward_channels_gpu.py; notes/compositing_backward_channels.md).

Every fixture has depth_range (1, 30): without a depth spread the distortion gradient is roundoff. A cotangent group is fed alone, the
other planes exactly 0; every output group is judged against its own maximum. Everything computed here is cached per process and never
modified by its users."""
import numpy as np

from grad_truth import compositing_truth
from helpers import make_scene, run_oracle

FIXTURES = {
    "A": dict(P=800, res=(64, 64), s0=0.3, view="canonical"),
    "B": dict(P=800, res=(48, 40), s0=0.3, view="oblique", bg=(0.3, 0.1, 0.6)),
    "C": dict(P=600, res=(40, 36), s0=0.3, view=[0, 3], bg=(0.3, 0.1, 0.6)),        # two views, partial tiles and quadrants
    "D": dict(P=1200, res=(33, 47), s0=0.15, view=[3, 5]),
}
GROUPS = {"rgb": (0, 1, 2), "normal": (3, 4, 5), "depth": (6,), "alpha": (7,), "distortion": (8,)}
GROUP_NAMES = list(GROUPS)
TRUTH_OUT = ("opacity", "colour", "v2g_Sigma", "v2g_B", "v2g_C")          # the output groups the float64 truth gives
MEAN2D_OUT = ("mean2D_xy", "mean2D_2")                                     # ... and those compared with the oracle
# under a depth or distortion cotangent these are identically zero; under the alpha cotangent, everything is
ZERO_OUT = {"depth": ("opacity", "colour", "mean2D_xy", "mean2D_2", "v2g_C"), "distortion": ("opacity", "colour", "mean2D_xy", "mean2D_2", "v2g_C"),
            "alpha": TRUTH_OUT + MEAN2D_OUT, "rgb": (), "normal": ()}
MARGIN, FLOOR, CONDITION = 4.0, 1e-5, 1e-3      # DESIGN.md section 4's margin, SURVEY 8c's compositing bar, the conditioning asked of a fixture

_CACHE = {}


def scene_of(name, seed=0):
    key = ("scene", name, seed)
    if key not in _CACHE:
        _CACHE[key] = make_scene(depth_range=(1.0, 30.0), seed=seed, **FIXTURES[name])
    return _CACHE[key]


def n_views(name):
    return scene_of(name)["viewmatrix"].shape[0]


def cotangent(scene, view, group):
    """[9,H,W] float32: default_rng(7 + view).standard_normal on the planes of `group`, exactly 0 elsewhere."""
    full = np.random.default_rng(7 + view).standard_normal((9, scene["H"], scene["W"])).astype(np.float32)
    w = np.zeros_like(full)
    w[list(GROUPS[group])] = full[list(GROUPS[group])]
    return w


def split(opacity, colour, v2g, mean2D=None):
    """The output groups of one view's compositing-stage gradients."""
    out = {"opacity": np.asarray(opacity, np.float64).reshape(-1), "colour": np.asarray(colour, np.float64),
           "v2g_Sigma": np.asarray(v2g, np.float64)[:, 0:6], "v2g_B": np.asarray(v2g, np.float64)[:, 6:9],
           "v2g_C": np.asarray(v2g, np.float64)[:, 9]}
    if mean2D is not None:
        out["mean2D_xy"], out["mean2D_2"] = np.asarray(mean2D, np.float64)[:, 0:2], np.asarray(mean2D, np.float64)[:, 2]
    return out


def split_truth(t):
    return split(t["dL_dopacity"], t["dL_dcolor"], t["dL_dview2gaussian"])


def err(a, b):
    """max|a - b| / max|b|; 0 for two all-zero arrays, inf for a non-zero `a` against an all-zero `b`."""
    m = np.abs(b).max() if b.size else 0.0
    d = np.abs(np.asarray(a, np.float64) - b).max() if b.size else 0.0
    return 0.0 if d == 0 else (float("inf") if m == 0 else float(d / m))


def is_zero(a):
    return not np.asarray(a).any()          # (-0.0 counts as zero)


def median_rows(truth, weight):
    """The Gaussians that are the blended median contributor of a pixel with a non-zero depth cotangent."""
    ids = truth["median_id"][(weight[6] != 0) & (truth["median_id"] >= 0)]
    return np.unique(ids)


def nonzero_rows(v2g):
    return np.flatnonzero(np.asarray(v2g).reshape(len(v2g), -1).any(1))


def oracle_case(name, view, seed=0):
    """One view of a fixture through the oracle, once: its state `o`, its backward per cotangent group, the float64 and float32
    truth on ITS state, and per group and output group the errors  e_oracle = |oracle - t64|,  e32 = |t32 - t64|  over max|t64|."""
    key = ("oracle", name, view, seed)
    if key not in _CACHE:
        scene = scene_of(name, seed)
        o = run_oracle(scene, view=view)
        ws = [cotangent(scene, view, g) for g in GROUP_NAMES]
        sv = dict(scene, bg=scene["bg"])
        t64 = compositing_truth(sv, o, ws)
        t32 = compositing_truth(sv, o, ws, dtype=np.float32)
        case = dict(scene=scene, o=o, weights=dict(zip(GROUP_NAMES, ws)), grads={}, t64={}, t32={}, e_oracle={}, e32={})
        for g, w, a, b in zip(GROUP_NAMES, ws, t64, t32):
            go = o["oracle"].backward(w)
            case["grads"][g] = go
            case["t64"][g], case["t32"][g] = a, b
            so, s64, s32 = split(go["dL_dopacity"], go["dL_dcolor"], go["dL_dview2gaussian"]), split_truth(a), split_truth(b)
            case["e_oracle"][g] = {k: err(so[k], s64[k]) for k in TRUTH_OUT}
            case["e32"][g] = {k: err(s32[k], s64[k]) for k in TRUTH_OUT}
        _CACHE[key] = case
    return _CACHE[key]
