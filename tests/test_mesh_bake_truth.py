"""The numpy restatement of the vertex colour baking (tests/mesh_bake_truth.py) pinned by routes that do not share its code -- all on the
CPU: scenes whose vertices land exactly on the pixel lattice of an identity camera, with image values that are multiples of 1/256, so
that every expected colour, weight and count can be written down by hand or with fractions.Fraction."""
from fractions import Fraction

import numpy as np

import mesh_bake_truth as B
import mesh_raster_truth as R

FX = B.FX


def _plane(shift, H=7, W=9, C=3, seed=1):
    P, faces, inner, (iu, iv) = B.pixel_plane(H, W, shift)
    img = B.dyadic_image(1, C, H, W, seed)
    b, r = B.bake_mesh(P, faces, None, R.identity_view(), FX, FX, img, depth_tol=0.01)
    assert inner.sum() == (H - 2) * (W - 2) and (b["cls"][0][inner] == B.USED).all()
    assert (b["n_used"][inner] == 1).all() and (b["best_view"][inner] == 0).all() and (b["weight"][inner] == 1.0).all()
    return b, img[0], inner, iu, iv


def test_vertices_on_pixel_centres_take_the_pixels_exactly():
    b, img, inner, iu, iv = _plane(0)
    assert np.array_equal(b["colors"][inner], img[:, iv[inner], iu[inner]].T)


def test_vertices_in_the_middle_of_four_pixels_take_their_exact_mean():
    b, img, inner, iu, iv = _plane(128)
    i, j = iu[inner], iv[inner]
    mean = (img[:, j, i].astype(np.float64) + img[:, j, i + 1] + img[:, j + 1, i] + img[:, j + 1, i + 1]) / 4.0     # exact: multiples of 1/1024
    assert np.array_equal(b["colors"][inner].astype(np.float64), mean.T)
    assert len(np.unique(mean)) > 10


def test_class_counts_of_the_two_plane_scene_equal_the_hand_written_numbers():
    P, faces, expected = B.two_planes_scene()
    img = B.dyadic_image(1, 2, 8, 8, 3)
    b, r = B.bake_mesh(P, faces, None, R.identity_view(), FX, FX, img, depth_tol=0.5)
    assert b["counts"] == expected and sum(b["counts"][:7]) == len(P)
    cls = b["cls"][0]
    assert (cls[:4] == B.USED).all()                                        # the front quad's own corners
    back = cls[4:53].reshape(7, 7)
    want = np.full((7, 7), B.UNCOVERED)
    want[1:6, 1:6] = B.USED
    want[2:5, 2:5] = B.OCCLUDED
    assert np.array_equal(back, want)
    assert cls[53:].tolist() == [B.UNCOVERED] * 3 + [B.OUTSIDE] * 2 + [B.NEAR] * 2
    # a vertex without a used sample: the four outputs are 0, 0, 0, -1
    dead = cls != B.USED
    assert not b["colors"][dead].any() and not b["weight"][dead].any() and not b["n_used"][dead].any() and (b["best_view"][dead] == -1).all()
    assert (b["n_used"][~dead] == 1).all() and (b["best_view"][~dead] == 0).all()
    # a wider tolerance than the gap between the planes makes the occluded vertices used; nothing else moves
    b2, _ = B.bake_mesh(P, faces, None, R.identity_view(), FX, FX, img, depth_tol=4.5)
    assert b2["counts"] == [2, 2, 27, 0, 0, 0, 29, 29]


def _probe(tx, images, **kw):
    P, faces, normals, wv, fx, H, W = B.probe_scene(tx)
    b, _ = B.bake_mesh(P, faces, normals, wv, fx, fx, images, depth_tol=0.01, **kw)
    return b


def _four_tap_mean(img, i, j):
    """Exact: the mean of the four taps around (i + 0.5, j + 0.5) of every channel, as Fractions."""
    return [(Fraction(float(ch[j, i])) + Fraction(float(ch[j, i + 1])) + Fraction(float(ch[j + 1, i])) + Fraction(float(ch[j + 1, i + 1]))) / 4 for ch in img]


def test_blend_is_the_exact_weighted_mean_and_best_takes_the_larger_weight():
    img = B.dyadic_image(2, 3, 8, 16, 7)
    s0, s1 = _four_tap_mean(img[0], 7, 3), _four_tap_mean(img[1], 11, 3)       # u = 7.5 and 11.5, v = 3.5
    for tx, w, best in (((0.0, 4.0), (Fraction(1), Fraction(1, 2)), 0), ((4.0, 0.0), (Fraction(1, 2), Fraction(1)), 1)):
        sa, sb = (s0, s1) if tx[0] == 0.0 else (_four_tap_mean(img[0], 11, 3), _four_tap_mean(img[1], 7, 3))
        blend = _probe(tx, img, cos_min=0.5, mode="blend")
        assert blend["cls"][:, 4].tolist() == [B.USED, B.USED] and blend["w"][:, 4].tolist() == [float(w[0]), float(w[1])]
        want = [np.float32(float((w[0] * a + w[1] * c) / (w[0] + w[1]))) for a, c in zip(sa, sb)]
        assert blend["colors"][4].tolist() == want and blend["weight"][4] == np.float32(1.5)
        assert blend["n_used"][4] == 2 and blend["best_view"][4] == best
        pick = _probe(tx, img, cos_min=0.5, mode="best")
        assert pick["colors"][4].tolist() == [np.float32(float(c)) for c in (sa, sb)[best]]
        assert pick["weight"][4] == 1.0 and pick["n_used"][4] == 2 and pick["best_view"][4] == best
    # equal weights: the earlier view
    pick = _probe((0.0, 0.0), img, mode="best")
    assert pick["best_view"][4] == 0 and pick["colors"][4].tolist() == [np.float32(float(c)) for c in s0]
    assert pick["colors"][4].tolist() != [np.float32(float(c)) for c in _four_tap_mean(img[1], 7, 3)]
    assert _probe((0.0, 0.0), img, mode="blend")["best_view"][4] == 0


def test_an_alpha_tap_below_the_threshold_and_a_nan_colour_tap_each_mask_the_sample():
    img = B.dyadic_image(1, 3, 8, 16, 8)
    alpha = np.ones((1, 8, 16), np.float32)
    assert _probe((0.0,), img, alpha=alpha)["cls"][0, 4] == B.USED
    for j, i in ((3, 7), (3, 8), (4, 7), (4, 8)):                              # each of the four taps on its own
        a = alpha.copy()
        a[0, j, i] = 0.4375
        assert _probe((0.0,), img, alpha=a, alpha_min=0.5)["cls"][0, 4] == B.MASKED
        assert _probe((0.0,), img, alpha=a, alpha_min=0.4375)["cls"][0, 4] == B.USED   # alpha >= alpha_min is used
        a[0, j, i] = np.nan
        assert _probe((0.0,), img, alpha=a)["cls"][0, 4] == B.MASKED
        for bad in (np.nan, np.inf):
            im = img.copy()
            im[0, 2, j, i] = bad
            b = _probe((0.0,), im)
            assert b["cls"][0, 4] == B.MASKED and b["n_used"][4] == 0 and b["best_view"][4] == -1 and not b["colors"][4].any()
    a = alpha.copy()
    a[0, 3, 6] = a[0, 5, 8] = 0.0                                              # not a tap
    assert _probe((0.0,), img, alpha=a)["cls"][0, 4] == B.USED


def test_cos_min_on_either_side_of_the_cosine_and_a_zero_normal():
    img = B.dyadic_image(1, 1, 8, 16, 9)
    root = float(np.sqrt(0.5))                                                 # the sample under tx = 4 has cos^2 = 1/2 exactly
    below, above = float(np.nextafter(root, 0.0)), float(np.nextafter(root, 1.0))
    assert below * below < 0.5 < above * above                                 # cm2 = cos_min cos_min, as the host forms it
    assert _probe((4.0,), img, cos_min=below)["cls"][0, 4] == B.USED
    assert _probe((4.0,), img, cos_min=above)["cls"][0, 4] == B.GRAZING
    assert _probe((4.0,), img, cos_min=0.0)["w"][0, 4] == 0.5
    P, faces, normals, wv, fx, H, W = B.probe_scene((0.0,))
    for n in ((0, 0, 0), (0, 0, 1), (1, 0, 0), (np.nan, 0, -1), (np.inf, 0, -1)):  # zero, facing away, edge-on, not finite
        nm = normals.copy()
        nm[4] = n
        b, _ = B.bake_mesh(P, faces, nm, wv, fx, fx, img, depth_tol=0.01, cos_min=0.0)
        assert b["cls"][0, 4] == B.GRAZING, n
    b, _ = B.bake_mesh(P, faces, None, wv, fx, fx, img, depth_tol=0.01, cos_min=1.0)     # without normals nothing is grazing, w = 1
    assert b["cls"][0, 4] == B.USED and b["weight"][4] == 1.0 and b["counts"][B.GRAZING] == 0
