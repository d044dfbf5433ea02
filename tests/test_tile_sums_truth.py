"""CPU checks of tests/tile_sums_truth.py, the numpy restatement of the loss sums' order (csrc/f3dg_tile_sums.h): it adds every
element exactly once, it is a float32 sum like any other, and on the inputs the GPU test uses it is NOT the bits of a plain sequential
sum -- so tests/test_tile_sums_gpu.py, which asks the kernels for the restatement's bits, tells a faithful kernel from a reordered one.
Every figure is printed before it is asserted (``pytest -s``)."""
import numpy as np
import pytest

import tile_sums_truth as T


@pytest.mark.parametrize("C", [None, 3])
@pytest.mark.parametrize("shape", T.SHAPES + ((3, 17, 33), (1, 16, 32)))
def test_integer_terms_sum_exactly(shape, C):
    """Integer-valued terms whose total stays below 2^24: every float32 addition is exact, so any dropped, doubled or misplaced element
    shows, whatever the order."""
    F, H, W = shape
    full = shape if C is None else (F, C, H, W)
    t = np.random.default_rng(5).integers(0, 16, full).astype(np.float32)
    want = t.astype(np.int64).reshape(F, -1).sum(1)
    assert int(want.max()) < 2 ** 24
    got = T.tile_sums(t)
    assert got.dtype == np.float32 and got.shape == (F,) and np.array_equal(got.astype(np.int64), want)
    parts = T.tile_partials(t)
    assert parts.shape == (F, ((H + 15) // 16) * ((W + 31) // 32)) and np.array_equal(parts.astype(np.int64).sum(1), want)


def test_the_big_shape_reaches_every_path():
    F, H, W = T.BIG
    ny, nx = (H + T.TH - 1) // T.TH, (W + T.TW - 1) // T.TW
    assert (ny, nx) == (8, 9) and ny * nx > T.LANES             # a second round of the second stage's lane loop
    assert W - (nx - 1) * T.TW == 4                             # the right column of tiles is 4 pixels wide
    assert H - (ny - 1) * T.TH == T.ROWS                        # the bottom tiles are 8 high: no thread there has a second row


@pytest.mark.parametrize("shape", T.SHAPES)
@pytest.mark.parametrize("family", sorted(T.FAMILIES))
def test_seeded_inputs_pin_the_order(family, shape):
    """Within N 2^-24 sum |t| of float64, the worst case of any float32 summation order over N elements; and at the big shape not the
    bits of the row-major sequential sum in at least one (frame, column)."""
    _, terms, sums = T.case(family, shape)
    differs = 0
    for col, t in sorted(terms.items()):
        assert t.dtype == np.float32 and sums[col].dtype == np.float32
        F, N = t.shape[0], t[0].size
        t64 = t.astype(np.float64).reshape(F, -1)
        s64, bound = t64.sum(1), N * 2.0 ** -24 * np.abs(t64).sum(1)
        seq = T.sequential_sums(t)
        for f in range(F):
            err = abs(float(sums[col][f]) - float(s64[f]))
            print(f"{family} {shape} frame {f} col {col}: s64 {s64[f]:.9e}  restated {float(sums[col][f]):.9e}  err {err:.3e}  bound {bound[f]:.3e}  "
                  f"sequential {float(seq[f]):.9e}")
            assert err <= bound[f]
        differs += int((seq != sums[col]).sum())
    if shape == T.BIG:
        assert differs >= 1, "the restatement equals the sequential sum everywhere: the pin would be vacuous"
