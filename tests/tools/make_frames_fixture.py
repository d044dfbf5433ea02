"""Generates tests/golden/frames/colorize.npz and magma_r_lut.npy (and the package's own text table, f3d-gaus_amd/magma_r_lut.txt) -- build container only.

The reference's OWN ``colorize_first`` and ``colorize`` (src/utils.py, imported from where the reference lies through the stand-in
modules of ref_import.py; nothing of it is copied) run on two seeded [4, 1, 6, 7] depth batches:
  * ``depth_in`` -> colorize_first(cmap='magma_r'): the percentile range (vmin, vmax) and the bytes, as at visualize.py:408. It holds
    -99 entries and +-inf, no NaN: numpy's percentile of data with a NaN is NaN, which would grey nothing and blacken everything;
  * ``depth_render`` -> colorize(vmin=vmin, vmax=vmax, cmap='magma_r'), as at :410: -99, NaN, +-inf and entries exactly at, just
    below and just above vmin and vmax.
The colour table is matplotlib's ``magma_r`` as 256 RGB byte triples. matplotlib >= 3.9 has dropped ``matplotlib.cm.get_cmap``, which
the reference calls; the generator points that name at ``matplotlib.colormaps.__getitem__`` for the run."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ref_import  # noqa: E402


def main():
    import matplotlib
    import matplotlib.cm
    if not hasattr(matplotlib.cm, "get_cmap"):
        matplotlib.cm.get_cmap = lambda name: matplotlib.colormaps[name]
    ref_import.install()
    import src.utils as U

    rng = np.random.default_rng(20)
    f32 = np.float32
    depth_in = (rng.random((4, 1, 6, 7), dtype=f32) * f32(2.5) + f32(6.5)).astype(f32)
    flat = depth_in.reshape(-1)
    flat[rng.choice(flat.size, 9, replace=False)] = -99
    flat[3], flat[100] = np.inf, -np.inf
    img_in, vmin, vmax = U.colorize_first(torch.from_numpy(depth_in.copy()), cmap='magma_r')
    assert isinstance(vmin, np.float32) and isinstance(vmax, np.float32) and vmin < vmax, (type(vmin), vmin, vmax)

    depth_render = (rng.random((4, 1, 6, 7), dtype=f32) * f32(4) + f32(5.5)).astype(f32)      # spills over both ends of the range
    flat = depth_render.reshape(-1)
    special = [-99, np.nan, np.inf, -np.inf, vmin, np.nextafter(vmin, f32(-np.inf)), np.nextafter(vmin, f32(np.inf)),
               vmax, np.nextafter(vmax, f32(-np.inf)), np.nextafter(vmax, f32(np.inf)), -99, np.nan, 0.0, -0.0]
    flat[rng.choice(flat.size, len(special), replace=False)] = np.array(special, dtype=f32)
    img_render = U.colorize(torch.from_numpy(depth_render.copy()), cmap='magma_r', vmin=vmin, vmax=vmax)
    assert img_in.shape == img_render.shape == (4, 6, 7, 4) and img_in.dtype == img_render.dtype == np.uint8

    lut = np.ascontiguousarray(matplotlib.colormaps['magma_r'](np.arange(256), bytes=True)[:, :3])
    assert lut.shape == (256, 3) and lut.dtype == np.uint8
    out = os.path.join(ROOT, "tests", "golden", "frames")
    os.makedirs(out, exist_ok=True)
    np.savez_compressed(os.path.join(out, "colorize.npz"), depth_in=depth_in, vmin=vmin, vmax=vmax, bytes_in=img_in,
                        depth_render=depth_render, bytes_render=img_render)
    np.save(os.path.join(out, "magma_r_lut.npy"), lut)
    np.savetxt(os.path.join(ROOT, "f3d-gaus_amd", "magma_r_lut.txt"), lut, fmt="%d",
               header="matplotlib's magma_r as 256 lines of R G B bytes: entry i = cmap(i, bytes=True)[:3]")
    print("vmin", vmin, "vmax", vmax, "sizes", [os.path.getsize(os.path.join(out, f)) for f in sorted(os.listdir(out))])


if __name__ == "__main__":
    main()
