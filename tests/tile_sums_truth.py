"""The order of the per-frame loss sums (csrc/f3dg_tile_sums.h), restated in numpy float32, and the seeded inputs the order-pin tests
share (tests/test_tile_sums_truth.py on the CPU, tests/test_tile_sums_gpu.py on the device).

The kernels promise bit-reproducible sums, so the ORDER of the float32 additions is part of their contract. For per-pixel terms
t[F, H, W] (or [F, C, H, W] for the masked L1) of F frames (SSIM: planes):

  thread   a frame is cut into tiles 32 wide and 16 high; thread tid = 32 ty + tx (ty < 8) of a tile starts at 0.0f and adds the pixel
           of row ty, then that of row ty + 8, both in column tx; a pixel outside the image is skipped. With channels, the C values of a
           pixel go into the same running sum in ascending order.
  tile     the 256 thread sums through the tree s[i] += s[i + half] (i < half), half = 128, 64, ... 1; s[0] is the tile's slot.
  frame    lane l of 64 starts at 0.0f and adds the slots of tiles l, l + 64, ... (row-major tile index) in ascending order; the 64
           lane sums through the same tree with half = 32 ... 1.

Every operation is one float32 addition. Only terms that numpy forms to the same bits as the kernels are pinned with this: differences,
absolute values and single products of float32 inputs -- no divide, no square root."""
import numpy as np

TW, TH, THREADS, ROWS, LANES = 32, 16, 256, 8, 64
BIG = (2, 120, 260)         # 9 x 8 = 72 tiles per frame: lanes 0..7 take a second slot, the right tiles are 4 wide, the bottom tiles 8 high
TINY = (1, 3, 5)            # one tile with 15 pixels
SHAPES = (BIG, TINY)


def _tree(s, half):
    """s [..., 2 * half] float32 -> [...] by the pairwise tree (a copy: the input stays)."""
    s = s.copy()
    while half >= 1:
        s[..., :half] = s[..., :half] + s[..., half:2 * half]
        half >>= 1
    return s[..., 0]


def tile_partials(t):
    """First stage: t [F, H, W] or [F, C, H, W] float32 -> the tile slots [F, tiles_y * tiles_x] float32."""
    t = np.asarray(t)
    assert t.dtype == np.float32
    if t.ndim == 3:
        t = t[:, None]
    F, C, H, W = t.shape
    ny, nx = (H + TH - 1) // TH, (W + TW - 1) // TW
    pad = np.zeros((F, C, ny * TH, nx * TW), np.float32)
    pad[:, :, :H, :W] = t
    inside = np.zeros((ny * TH, nx * TW), bool)
    inside[:H, :W] = True
    # [F, C, tile row, j, ty, tile column, tx]: the pixel of thread (ty, tx) in its round j is row 8 j + ty of the tile
    pad = pad.reshape(F, C, ny, TH // ROWS, ROWS, nx, TW)
    inside = inside.reshape(ny, TH // ROWS, ROWS, nx, TW)
    acc = np.zeros((F, ny, ROWS, nx, TW), np.float32)
    for j in range(TH // ROWS):
        for c in range(C):
            acc = np.where(inside[:, j], acc + pad[:, c, :, j], acc)
    s = acc.transpose(0, 1, 3, 2, 4).reshape(F, ny * nx, THREADS)           # thread index 32 ty + tx
    return _tree(s, THREADS // 2)


def frame_sums(partials):
    """Second stage: the tile slots [F, T] float32 -> the frame sums [F] float32."""
    partials = np.asarray(partials)
    assert partials.dtype == np.float32
    F, T = partials.shape
    rounds = (T + LANES - 1) // LANES
    pad = np.zeros((F, rounds * LANES), np.float32)
    pad[:, :T] = partials
    have = (np.arange(rounds * LANES) < T).reshape(rounds, LANES)
    pad = pad.reshape(F, rounds, LANES)
    acc = np.zeros((F, LANES), np.float32)
    for r in range(rounds):
        acc = np.where(have[r], acc + pad[:, r], acc)
    return _tree(acc, LANES // 2)


def tile_sums(t):
    """Both stages: the sums [F] float32 of t [F, H, W] or [F, C, H, W], in the kernels' order."""
    return frame_sums(tile_partials(t))


def sequential_sums(t):
    """What the pin is told apart from: one float32 accumulator per frame over the elements in storage order."""
    t = np.asarray(t)
    return np.add.accumulate(t.reshape(t.shape[0], -1), axis=1, dtype=np.float32)[:, -1]


# ------------------------------------------------------------------------------------------------ seeded inputs
def _spread(rng, shape):
    """Positive float32 values over three decades, 1e-3 .. 1: large and small terms meet in every tile, so the order shows."""
    return (rng.random(shape) * 10.0 ** rng.uniform(-3.0, 0.0, shape)).astype(np.float32)


def ssim_inputs(shape):
    """(img1, img2) [n_planes, H, W] and the pinned columns {1: |a - b|, 2: (a - b)^2} of the plane sums."""
    rng = np.random.default_rng(1000 + shape[1])
    a, b = _spread(rng, shape), _spread(rng, shape)
    d = a - b
    return (a, b), {1: np.abs(d), 2: d * d}


def masked_l1_inputs(shape, C=3):
    """(a, b [F, C, H, W], m [F, 1, H, W]) and both columns {0: m |a - b| (per channel), 1: m}. The mask is soft -- about 70 % of the
    pixels, magnitudes spread like the images -- so the sum of the mask depends on the order too."""
    F, H, W = shape
    rng = np.random.default_rng(2000 + H)
    a, b = _spread(rng, (F, C, H, W)), _spread(rng, (F, C, H, W))
    m = np.where(rng.random((F, 1, H, W)) < 0.7, _spread(rng, (F, 1, H, W)), np.float32(0.0)).astype(np.float32)
    return (a, b, m), {0: m * np.abs(a - b), 1: m[:, 0]}


def geometry_inputs(shape):
    """A fixture of tests/geometry_loss_truth.py whose distortion plane, alpha plane, depth target and mask are spread over decades,
    and the pinned columns {1: raster[8], 2: m |raster[6] - depth_target|, 4: |raster[7] - alpha_target|}."""
    import torch
    import geometry_loss_truth as G
    F, H, W = shape
    f = G.make_fixture(F, H, W, seed=3)
    rng = np.random.default_rng(3000 + H)
    f["raster"][:, 8] = torch.from_numpy(_spread(rng, shape))
    f["raster"][:, 7] = torch.from_numpy(_spread(rng, shape))
    sign = np.where(rng.random(shape) < 0.5, np.float32(-1.0), np.float32(1.0))
    f["depth_target"] = f["raster"][:, 6] + torch.from_numpy(sign * _spread(rng, shape))
    f["mask"] = torch.from_numpy(np.where(rng.random(shape) < 0.7, _spread(rng, shape), np.float32(0.0)).astype(np.float32))
    r = f["raster"].numpy()
    return f, {1: r[:, 8].copy(), 2: f["mask"].numpy() * np.abs(r[:, 6] - f["depth_target"].numpy()),
               4: np.abs(r[:, 7] - f["alpha_target"].numpy())}


FAMILIES = {"ssim": ssim_inputs, "masked_l1": masked_l1_inputs, "geometry": geometry_inputs}
_CACHE = {}


def case(family, shape):
    """(inputs, {column: per-pixel terms}, {column: restated sums [F] float32}) of a family at a shape: computed once, shared, never
    modified."""
    key = (family, tuple(shape))
    if key not in _CACHE:
        inputs, terms = FAMILIES[family](tuple(shape))
        _CACHE[key] = (inputs, terms, {k: tile_sums(t) for k, t in terms.items()})
    return _CACHE[key]
