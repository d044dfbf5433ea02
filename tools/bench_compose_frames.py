"""Times the frame composer (f3dg_compose_frames through frames.compose_frames) against the same frames built from torch operations
on the device -- colour-table indexing, cat, a padded grid copy, then pack_frames: the only route the package offered before -- at
B = 8 images of 256 x 256 and 32 and 128 orbit views. Prints ONE JSON line. Device events around runs that end in a synchronise;
both routes alternate in one process; the median of the rounds is reported. The kernel's rate is its compulsory byte count (every
dynamic plane once, every static plane once, every frame byte once) over its time.

    python tools/bench_compose_frames.py [--rounds 7] [--views 32 128]
"""
import argparse
import json
import math
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import f3dgaus_amd as f3d  # noqa: E402
from f3dgaus_amd import frames  # noqa: E402
from f3dgaus_amd.gaussian_renderer import pack_frames  # noqa: E402


def torch_route(images, depth_in, render, depth, normal, ranges, lut, padding=2, invalid_val=-99.0):
    """The composer's contract in torch operations: float strips and a zero grid filled cell by cell; float32 [V, 3, Hg, Wg] for
    pack_frames."""
    B, V = render.shape[:2]
    H, W = render.shape[-2:]
    table = lut.float() / 255                                         # pack_frames returns the table's bytes from these
    vmin, vmax = ranges[0, 0], ranges[0, 1]

    def colour(d):                                                    # [..., 1, H, W] -> [..., 3, H, W]
        t = (d - vmin) / (vmax - vmin)
        idx = torch.where(t < 0, 0, torch.where(t >= 1, 255, (torch.nan_to_num(t, nan=0.0, posinf=0.0, neginf=0.0) * 256).long())).clamp_(0, 255)
        c = table[idx.squeeze(-3)]
        c = torch.where(torch.isnan(t).squeeze(-3).unsqueeze(-1), torch.zeros_like(c), c)
        c = torch.where((d == invalid_val).squeeze(-3).unsqueeze(-1), torch.full_like(c, 128 / 255), c)
        return c.movedim(-1, -3)

    strip = torch.cat([images[:, None].expand(-1, V, -1, -1, -1), colour(depth_in)[:, None].expand(-1, V, -1, -1, -1), render, colour(depth),
                       (normal + 1) / 2], dim=4)                      # [B, V, 3, H, 5 W]
    PW = strip.shape[-1]
    xmaps = min(int(math.sqrt(B)), B)
    ymaps = -(-B // xmaps)
    grid = torch.zeros((V, 3, ymaps * (H + padding) + padding, xmaps * (PW + padding) + padding), dtype=torch.float32, device=strip.device)
    for k in range(B):
        y0, x0 = (k // xmaps) * (H + padding) + padding, (k % xmaps) * (PW + padding) + padding
        grid[:, :, y0:y0 + H, x0:x0 + PW] = strip[k]
    return grid


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--views", type=int, nargs="+", default=[32, 128])
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--res", type=int, default=256)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_compose_frames needs a HIP device: a time measured anywhere else says nothing")
    dev = torch.device("cuda:0")
    B, R = args.batch, args.res
    g = torch.Generator(device=dev).manual_seed(0)
    u = lambda *s: torch.rand(s, generator=g, device=dev)
    images, depth_in = u(B, 3, R, R), u(B, 1, R, R) * 2 + 6.667
    lut = frames.colormap_lut().to(dev)
    results = []
    for V in args.views:
        orbit = {"render": u(B, V, 3, R, R) * 1.2 - 0.1, "rendered_depth": u(B, V, 1, R, R) * 4 + 5.5, "depth_normal": u(B, V, 3, R, R) * 2 - 1}
        ranges = frames.depth_range(depth_in).reshape(1, 2)
        out = torch.empty(frames.compose_orbit_frames(images, depth_in, orbit).shape, dtype=torch.uint8, device=dev)
        panels = [(images, "rgb", None), (depth_in, "colormap", 0), (orbit["render"], "rgb", None), (orbit["rendered_depth"], "colormap", 0),
                  (orbit["depth_normal"], "signed", None)]
        kernel = lambda: frames.compose_frames(panels, ranges=ranges, out=out)                 # the range is given to both routes
        whole = lambda: frames.compose_orbit_frames(images, depth_in, orbit, out=out)           # ... and here computed per call
        eager = lambda: pack_frames(torch_route(images, depth_in, orbit["render"], orbit["rendered_depth"], orbit["depth_normal"], ranges, lut))
        same = bool(torch.equal(kernel(), eager()))
        tk, tt, tw = [], [], []
        for _ in range(2):                                            # warm-up of every route
            timed(kernel), timed(eager), timed(whole)
        for _ in range(args.rounds):
            tk.append(timed(kernel)[0])
            tt.append(timed(eager)[0])
            tw.append(timed(whole)[0])
        read = 4 * R * R * B * (7 * V + 4)
        written = out.numel()
        k_ms, t_ms = statistics.median(tk), statistics.median(tt)
        results.append({"views": V, "kernel_ms": round(k_ms, 4), "kernel_min_ms": round(min(tk), 4), "torch_ms": round(t_ms, 4),
                        "torch_min_ms": round(min(tt), 4), "with_depth_range_ms": round(statistics.median(tw), 4), "speedup": round(t_ms / k_ms, 2), "bytes_read": read, "bytes_written": written,
                        "kernel_GBps": round((read + written) / k_ms / 1e6, 1), "frame_shape": list(out.shape), "routes_byte_equal": same})
        del orbit, out, panels, kernel, whole, eager
        torch.cuda.empty_cache()
    print(json.dumps({"tool": "bench_compose_frames", "device": torch.cuda.get_device_name(0), "batch": B, "res": R, "rounds": args.rounds,
                      "note": "kernel_ms / torch_ms: both routes are handed the colour range; with_depth_range_ms: compose_orbit_frames, which sorts the input depths per call",
                      "results": results, "kernel_faster_at_every_size": all(r["kernel_ms"] < r["torch_ms"] for r in results)}))


if __name__ == "__main__":
    main()
