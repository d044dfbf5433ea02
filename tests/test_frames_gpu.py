"""Frame composer on the device: f3dg_compose_frames against frames_truth, byte for byte. The truth is integer arithmetic on float32
values that both sides compute with IEEE operations, so the only tolerance is equality. Shapes are the smallest that still break a
wrong kernel: 5 x 7 pixels (a row byte count and a total that are no multiples of 16: chunks cross panel, cell, row and frame
boundaries), B from 1 (the bare strip) over 5 (an empty cell) to 8, several workgroups, and one workgroup for the grid-stride loop.
The multi-GB 64-bit offset path (B = 64 at 256^2 x 128 views is 8.1 GB) is not run at size; tests/test_frames_truth.py checks its
size arithmetic."""
import os

import numpy as np
import pytest
import torch

import frames_truth as T
from frames_cases import hand_grid_cases

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "frames")
H, W, V = 5, 7, 3


@pytest.fixture(scope="module")
def lut():
    return np.load(os.path.join(GOLDEN, "magma_r_lut.npy"))


def _compose(dev, panels, nrow=None, ranges=None, max_workgroups=0, host=False, lut=None, padding=2):
    """frames.compose_frames on numpy (or device) panels, into an `out` carved from a buffer pre-filled with 0xAA and 64 bytes longer
    than the frames: returns the frames as numpy after checking that the guard is intact."""
    from f3dgaus_amd import frames
    dp = [(torch.from_numpy(np.ascontiguousarray(p[0])).to(dev) if isinstance(p[0], np.ndarray) else p[0], p[1], p[2]) for p in panels]
    B, PW = dp[0][0].shape[0], len(dp) * dp[0][0].shape[-1]
    Vn = max([p[0].shape[1] for p in dp if p[0].dim() == 5] + [1])
    Hg, Wg, _, _ = T.grid_shape(B, dp[0][0].shape[-2], PW, int(np.sqrt(B)) if nrow is None else nrow, padding)
    nb = Vn * Hg * Wg * 3
    buf = torch.full((nb + 64,), 0xAA, dtype=torch.uint8, device="cpu" if host else dev)
    if host:
        buf = buf.pin_memory()
    r = None if ranges is None else torch.from_numpy(np.asarray(ranges, dtype=np.float32).reshape(-1, 2)).to(dev)
    got = frames.compose_frames(dp, nrow=nrow, padding=padding, ranges=r, out=buf[:nb], max_workgroups=max_workgroups,
                                lut=None if lut is None else torch.from_numpy(lut).to(dev))
    torch.cuda.synchronize()
    assert tuple(got.shape) == (Vn, Hg, Wg, 3) and got.data_ptr() == buf.data_ptr()
    assert (buf[nb:] == 0xAA).all(), "bytes behind the frames were written"
    return got.cpu().numpy().copy()


def _reference_panels(B, seed):
    """The five panels of visualize.py:414 with out-of-range colours and special depths sprinkled in."""
    rng = np.random.default_rng(seed)
    u = lambda *s: rng.random(s, dtype=np.float32)
    images = u(B, 3, H, W) * np.float32(1.2) - np.float32(0.1)
    depth_in = u(B, 1, H, W) * np.float32(2.5) + np.float32(6.5)
    depth_in.reshape(-1)[rng.choice(depth_in.size, 2, replace=False)] = -99
    render = u(B, V, 3, H, W) * np.float32(1.2) - np.float32(0.1)
    depth = u(B, V, 1, H, W) * np.float32(4) + np.float32(5.5)
    depth.reshape(-1)[rng.choice(depth.size, 5, replace=False)] = np.array([-99, np.nan, np.inf, -np.inf, 0], dtype=np.float32)
    normal = u(B, V, 3, H, W) * np.float32(2.2) - np.float32(1.1)
    normal.reshape(-1)[rng.choice(normal.size, 2, replace=False)] = np.array([np.nan, -1.0], dtype=np.float32)
    valid = depth_in[depth_in != -99]
    ranges = np.array([[np.percentile(valid, 2), np.percentile(valid, 85)]], dtype=np.float32)
    return [(images, "rgb", None), (depth_in, "colormap", 0), (render, "rgb", None), (depth, "colormap", 0), (normal, "signed", None)], ranges


@pytest.mark.parametrize("B", [1, 2, 3, 4, 5, 8])
def test_five_panels_and_one_panel_equal_the_truth(gpu_device, lut, B):
    panels, ranges = _reference_panels(B, seed=B)
    want = T.compose(panels, ranges=ranges, lut=lut)
    assert want.shape[1:] == ((H, 5 * W, 3) if B == 1 else T.grid_shape(B, H, 5 * W, int(np.sqrt(B)), 2)[:2] + (3,))
    if B in (1, 3, 5):
        assert want.size % 16 != 0 and (want.shape[2] * 3) % 16 != 0       # the stream ends inside a chunk, and so does every row
    for wg in (0, 1):                                                   # 1: one workgroup walks every chunk
        got = _compose(gpu_device, panels, ranges=ranges, max_workgroups=wg)
        assert np.array_equal(got, want), (B, wg, int((got != want).sum()))
        assert (got == 0xAA).sum() == (want == 0xAA).sum()             # nothing of the pre-fill is left inside
    one = [panels[2]]
    want1 = T.compose(one)
    for wg in (0, 1):
        assert np.array_equal(_compose(gpu_device, one, max_workgroups=wg), want1), (B, wg)
    if B == 3:                                                          # other paddings: none, and one wider than a panel of the strip
        for pad, nrow in ((0, 2), (9, 2), (1, 3)):
            got = _compose(gpu_device, panels, nrow=nrow, ranges=ranges, padding=pad, max_workgroups=1)
            assert np.array_equal(got, T.compose(panels, nrow=nrow, padding=pad, ranges=ranges, lut=lut)), pad
    if B == 5:                                                          # another nrow: three columns, one empty cell
        assert np.array_equal(_compose(gpu_device, panels, nrow=3, ranges=ranges), T.compose(panels, nrow=3, ranges=ranges, lut=lut))


def test_hand_written_grids_hold_for_the_kernel(gpu_device):
    for name, panels, nrow, want in hand_grid_cases():
        got = _compose(gpu_device, panels, nrow=nrow)
        assert got.shape == want.shape and np.array_equal(got, want), name


def test_edge_values_placed_by_hand(gpu_device, lut):
    f = np.float32
    h, w = 8, 100
    ninf, pinf = f(-np.inf), f(np.inf)

    def plane(values, fill):
        a = np.full(h * w, fill, dtype=f)
        v = np.asarray(values, dtype=f)
        assert v.size <= a.size
        a[:v.size] = v
        return a.reshape(1, 1, 1, h, w)

    special = [np.nan, np.inf, -np.inf, -99, -0.0, 0.0, 1.0, 2.0, -1.0, 1e-30, -1e-30, 3e38]
    k = np.arange(257, dtype=f) / f(256)                               # the bin edges of the range [0, 1] are exact
    d01 = plane(np.concatenate([k, np.nextafter(k, ninf), np.nextafter(k, pinf), np.array(special, dtype=f)]), 0.5)
    vmin, vmax = f(6.5427785), f(8.611702)
    step = (vmax - vmin) / f(256)
    edges = [vmin, vmax, np.nextafter(vmin, ninf), np.nextafter(vmin, pinf), np.nextafter(vmax, ninf), np.nextafter(vmax, pinf)]
    dr = plane(np.concatenate([np.array(edges + special, dtype=f), vmin + np.arange(257, dtype=f) * step]), 7.0)
    dflat = plane([3.0, 2.0, 4.0, np.nextafter(f(3), pinf)] + special, 3.0)          # vmin == vmax: t = d * 0
    ranges = np.array([[0, 1], [vmin, vmax], [3, 3]], dtype=f)
    kb = np.arange(256, dtype=f) / f(255)
    colour = np.concatenate([kb, np.nextafter(kb, ninf), np.nextafter(kb, pinf), np.array(special + [1.5, -0.5], dtype=f)])
    rgb = np.concatenate([plane(colour, 0.25), plane(colour[::-1], 0.5), plane(np.roll(colour, 7), 0.75)], axis=2)
    with np.errstate(over="ignore"):
        sgn = f(2) * colour - f(1)                                          # (v + 1) / 2 lands on and around k / 255
    signed3 = np.concatenate([plane(sgn, 0.0), plane(np.roll(sgn, 3), -1.0), plane(sgn[::-1], 1.0)], axis=2)
    signed1 = plane(np.concatenate([sgn, np.array([-1.1, 1.1, -1.0, 1.0], dtype=f)]), 0.5)
    panels = [(d01, "colormap", 0), (dr, "colormap", 1), (dflat, "colormap", 2), (rgb, "rgb", None), (signed3, "signed", None),
              (signed1, "signed", None)]
    want = T.compose(panels, ranges=ranges, lut=lut)
    got = _compose(gpu_device, panels, ranges=ranges)
    assert np.array_equal(got, want), np.argwhere(got != want)[:8]
    # the truth itself says what the contract says at these places
    strip = want[0]
    at = lambda panel, i: strip[i // w, panel * w + i % w]
    assert (at(0, 0) == lut[0]).all() and (at(0, 256) == lut[255]).all() and (at(0, 128) == lut[128]).all()     # d = 0, 1, 0.5
    assert (at(0, 257 + 5) == lut[4]).all() and (at(0, 514 + 5) == lut[5]).all()                                 # just below / above 5 / 256
    assert (at(1, 0) == lut[0]).all() and (at(1, 1) == lut[255]).all() and (at(1, 2) == lut[0]).all()           # vmin, vmax, below vmin
    assert (at(2, 0) == lut[0]).all() and (at(2, 1) == lut[0]).all() and (at(2, 4) == 0).all() and (at(2, 7) == 128).all()   # vmin == vmax
    # another colour table through the same path
    other = np.ascontiguousarray(lut[::-1])
    assert np.array_equal(_compose(gpu_device, panels[:2], ranges=ranges, lut=other), T.compose(panels[:2], ranges=ranges, lut=other))


def test_strided_sources_are_read_in_place(gpu_device, lut):
    from f3dgaus_amd import frames
    B = 3
    rng = np.random.default_rng(11)
    raster = (rng.random((B * V, 9, H, W), dtype=np.float32) * np.float32(1.4) - np.float32(0.2)).astype(np.float32)
    raster[:, 6] = raster[:, 6] * np.float32(3) + np.float32(6)
    ranges = np.array([[6.5, 9.0]], dtype=np.float32)
    r5 = raster.reshape(B, V, 9, H, W)
    kinds = ((slice(0, 3), "rgb", None), (slice(6, 7), "colormap", 0), (slice(3, 6), "signed", None), (slice(7, 8), "signed", None))
    want = T.compose([(r5[:, :, s], k, i) for s, k, i in kinds], ranges=ranges, lut=lut)
    d = torch.from_numpy(raster).to(gpu_device)
    views = [(d.view(B, V, 9, H, W)[:, :, s], k, i) for s, k, i in kinds]
    for t, k, _ in views:                                               # no gather copy: the descriptor points into the raster
        keep = []
        p = frames._describe(t, k, 0, 1, keep)[0]
        assert keep[0].data_ptr() == t.data_ptr() and p.src == t.data_ptr() and p.frame_stride == 9 * H * W and p.image_stride == V * 9 * H * W
    assert np.array_equal(_compose(gpu_device, views, ranges=ranges), want)
    assert np.array_equal(_compose(gpu_device, [(t.contiguous(), k, i) for t, k, i in views], ranges=ranges), want)
    # the [B, V, C, H, W] tensors of render_orbit, one of them transposed in memory ([V, B, ...] storage)
    tv = d.view(B, V, 9, H, W)[:, :, 0:3].transpose(0, 1).contiguous().transpose(0, 1)
    assert not tv.is_contiguous()
    assert np.array_equal(_compose(gpu_device, [(tv, "rgb", None)] + views[1:], ranges=ranges), want)


def test_static_panel_equals_the_same_data_on_every_frame(gpu_device, lut):
    panels, ranges = _reference_panels(4, seed=21)
    rep = [(np.repeat(p[0][:, None], V, axis=1) if p[0].ndim == 4 else p[0], p[1], p[2]) for p in panels]
    a = _compose(gpu_device, panels, ranges=ranges)
    b = _compose(gpu_device, rep, ranges=ranges)
    assert np.array_equal(a, b) and np.array_equal(a, T.compose(panels, ranges=ranges, lut=lut))
    # an expanded view (stride 0 along the frame axis) is a static panel too
    dev_rep = [(torch.from_numpy(p[0]).to(gpu_device)[:, None].expand(-1, V, -1, -1, -1) if p[0].ndim == 4 else p[0], p[1], p[2]) for p in panels]
    assert np.array_equal(_compose(gpu_device, dev_rep, ranges=ranges), a)


def test_pinned_host_out_and_repeat_runs_are_byte_identical(gpu_device, lut):
    from f3dgaus_amd import frames
    panels, ranges = _reference_panels(5, seed=31)
    a = _compose(gpu_device, panels, ranges=ranges)
    assert np.array_equal(a, _compose(gpu_device, panels, ranges=ranges))                    # two runs
    for wg in (0, 2):
        assert np.array_equal(_compose(gpu_device, panels, ranges=ranges, host=True, max_workgroups=wg), a), wg
    x = torch.from_numpy(panels[0][0]).to(gpu_device)
    with pytest.raises(RuntimeError, match="must be pinned"):
        frames.compose_frames([(x, "rgb", None)], out=torch.empty(23 * 20 * 3, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="out must be a contiguous uint8 tensor"):
        frames.compose_frames([(x, "rgb", None)], out=torch.empty(5, dtype=torch.uint8, device=gpu_device))
    with pytest.raises(RuntimeError, match="float32"):
        frames.compose_frames([(x.half(), "rgb", None)])
    with pytest.raises(RuntimeError, match="needs `ranges`"):
        frames.compose_frames([(x[:, :1], "colormap", 0)])
    with pytest.raises(RuntimeError, match="range_index 1 outside"):
        frames.compose_frames([(x[:, :1], "colormap", 1)], ranges=torch.zeros(1, 2, device=gpu_device))


def test_depth_range_on_the_device_is_the_host_result(gpu_device):
    from f3dgaus_amd import frames
    z = np.load(os.path.join(GOLDEN, "colorize.npz"))
    d = torch.from_numpy(z["depth_in"])
    host = frames.depth_range(d)
    dev = frames.depth_range(d.to(gpu_device))
    assert dev.device.type == "cuda" and dev.cpu().numpy().view(np.uint32).tolist() == host.numpy().view(np.uint32).tolist()
    assert [float(v) for v in dev.cpu()] == [float(z["vmin"]), float(z["vmax"])]
    rng = np.random.default_rng(5)
    big = torch.from_numpy((rng.random(70001, dtype=np.float32) * np.float32(3) + np.float32(5)).astype(np.float32))
    big[::13] = -99
    assert frames.depth_range(big.to(gpu_device)).cpu().numpy().view(np.uint32).tolist() == frames.depth_range(big).numpy().view(np.uint32).tolist()


def test_no_host_read_in_depth_range_and_orbit_frames(gpu_device, lut):
    """depth_range and compose_orbit_frames under torch's sync debug mode "error": any synchronising read of the device by the host
    (an .item(), a 0-d tensor used as an index, a blocking copy) raises. One call before it, so that the one-time upload of the colour
    table is not what is judged; values as before."""
    from f3dgaus_amd import frames
    panels, ranges = _reference_panels(3, seed=41)
    dev = [torch.from_numpy(p[0]).to(gpu_device) for p in panels]
    orbit = {"render": dev[2], "rendered_depth": dev[3], "depth_normal": dev[4]}
    out = torch.empty_like(frames.compose_orbit_frames(dev[0], dev[1], orbit))
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        r = frames.depth_range(dev[1])
        got = frames.compose_orbit_frames(dev[0], dev[1], orbit, out=out)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert r.cpu().numpy().view(np.uint32).tolist() == ranges.reshape(-1).view(np.uint32).tolist()
    assert np.array_equal(got.cpu().numpy(), T.compose(panels, ranges=ranges, lut=lut))


def test_orbit_frames_end_to_end(f3d, gpu_device, lut):
    """make_gaussians -> render_orbit -> compose_orbit_frames against the truth on the same tensors copied to the host."""
    from f3dgaus_amd import cameras, frames, synthetic
    B, res, views = 3, 32, 4
    cfg = cameras.default_cfg(res)
    gs = [synthetic.make_gaussians(3000, s0=0.05, seed=60 + b, device=gpu_device) for b in range(B)]
    pc = {k: torch.stack([g[k] for g in gs]) for k in gs[0]}
    orbit = f3d.cycle.render_orbit(pc, cfg, num_views=views, views_per_call=4)
    g = torch.Generator().manual_seed(8)
    images = torch.rand(B, 3, res, res, generator=g).to(gpu_device)
    depth_in = (torch.rand(B, 1, res, res, generator=g) * 2 + 6.667).to(gpu_device)
    got = frames.compose_orbit_frames(images, depth_in, orbit)
    torch.cuda.synchronize()
    ranges = frames.depth_range(depth_in.cpu()).numpy().reshape(1, 2)
    n = lambda t: t.cpu().numpy()
    want = T.compose([(n(images), "rgb", None), (n(depth_in), "colormap", 0), (n(orbit["render"]), "rgb", None),
                      (n(orbit["rendered_depth"]), "colormap", 0), (n(orbit["depth_normal"]), "signed", None)], ranges=ranges, lut=lut)
    assert got.dtype == torch.uint8 and tuple(got.shape) == want.shape == (views, 3 * (res + 2) + 2, 5 * res + 4, 3)
    assert np.array_equal(n(got), want), int((n(got) != want).sum())
    assert len(np.unique(want[:, 2:2 + res, 2 + 2 * res:2 + 5 * res])) > 50          # the rendered panels are not blank
