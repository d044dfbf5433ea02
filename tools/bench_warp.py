"""Times the forward warp (warp.forward_warp: f3dg_forward_warp's launch sequence -- fill, z-buffer, accumulate, resolve, erode) at the
training shape of DESIGN.md section 5 -- 8 source frames x 4 target cameras at 256 x 256, C = 3, erode 5 -- against a plain torch composite
of the same definition on the same device: ``scatter_reduce_(amin)`` for the z-buffer, ``index_add_`` for the sums, a division and
``max_pool2d`` for the erosion, batched over all pairs, float32. The parent of this feature could not warp at all, so the composite is the
baseline. Prints ONE JSON line. Device events around runs that end in a synchronise; both routes alternate in one process; the median of
the rounds is reported, with the bytes each call has to move (inputs read once, outputs written once) and the workspace it also touches.
``--loss`` adds forward + backward of losses.warping_loss of a random render against the warp's output (src x views frames), the same way.

    python tools/bench_warp.py [--rounds 15] [--src 8] [--views 4] [--res 256] [--erode 5] [--loss]
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
import f3dgaus_amd  # noqa: E402,F401
from f3dgaus_amd import _lib, losses, synthetic, warp  # noqa: E402


def torch_composite(image, depth, rel, fx, fy, z_near=0.01, tol=0.05, floor=1 / 16, threshold=0.9, erode=5):
    """The definition of include/f3dg.h in float32 torch operations, all B x V pairs at once (every source pixel is live here)."""
    B, C, H, W = image.shape
    V = rel.shape[1]
    HW = H * W
    ii = torch.arange(W, device=image.device, dtype=torch.float32).reshape(1, 1, 1, W)
    jj = torch.arange(H, device=image.device, dtype=torch.float32).reshape(1, 1, H, 1)
    d = depth.reshape(B, 1, H, W)
    X, Y = (ii + 0.5 - W / 2) / fx * d, (jj + 0.5 - H / 2) / fy * d
    R = rel.reshape(B, V, 4, 4, 1, 1)
    x = X * R[:, :, 0, 0] + Y * R[:, :, 1, 0] + d * R[:, :, 2, 0] + R[:, :, 3, 0]
    y = X * R[:, :, 0, 1] + Y * R[:, :, 1, 1] + d * R[:, :, 2, 1] + R[:, :, 3, 1]
    z = X * R[:, :, 0, 2] + Y * R[:, :, 1, 2] + d * R[:, :, 2, 2] + R[:, :, 3, 2]
    u, v = fx * x / z + W / 2 - 0.5, fy * y / z + H / 2 - 0.5
    ok = (z > z_near) & (u > -1) & (u < W) & (v > -1) & (v < H)
    u, v = torch.where(ok, u, 0.0), torch.where(ok, v, 0.0)
    x0, y0 = torch.floor(u), torch.floor(v)
    a, b = u - x0, v - y0
    pair = torch.arange(B * V, device=image.device).reshape(B, V, 1, 1) * HW
    zmin = torch.full((B * V * HW,), float("inf"), device=image.device)
    taps = []
    for dy in (0, 1):
        for dx in (0, 1):
            tx, ty = x0.long() + dx, y0.long() + dy
            w = (a if dx else 1 - a) * (b if dy else 1 - b)
            cand = ok & (tx >= 0) & (tx < W) & (ty >= 0) & (ty < H) & (w > 0)
            idx = pair + ty.clamp(0, H - 1) * W + tx.clamp(0, W - 1)
            taps.append((cand, idx, w))
            sel = cand & (w >= floor)
            zmin.scatter_reduce_(0, idx[sel], z[sel], "amin", include_self=True)
    acc = torch.zeros(B * V * HW, C + 2, device=image.device)
    img = image.reshape(B, 1, C, H, W).expand(B, V, C, H, W).permute(0, 1, 3, 4, 2)          # [B,V,H,W,C]
    for cand, idx, w in taps:
        sel = cand & (z <= zmin[idx] + tol)
        ws = w[sel].unsqueeze(1)
        acc.index_add_(0, idx[sel], torch.cat([ws, ws * img[sel], ws * z[sel].unsqueeze(1)], 1))
    acc = acc.reshape(B, V, H, W, C + 2)
    Ws = acc[..., 0]
    safe = torch.where(Ws > 0, Ws, 1.0)
    warped = torch.where((Ws > 0).unsqueeze(2), acc[..., 1:1 + C].permute(0, 1, 4, 2, 3) / safe.unsqueeze(2), 0.0)
    wdepth = torch.where(Ws > 0, acc[..., 1 + C] / safe, 0.0).unsqueeze(2)
    mask = (Ws >= threshold).float().reshape(B * V, 1, H, W)
    if erode > 1:
        mask = -torch.nn.functional.max_pool2d(-mask, erode, 1, erode // 2)
    return {"warped": warped, "mask": mask.reshape(B, V, 1, H, W), "warped_depth": wdepth, "weight": Ws.unsqueeze(2)}


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--src", type=int, default=8)
    ap.add_argument("--views", type=int, default=4)
    ap.add_argument("--res", type=int, default=256)
    ap.add_argument("--erode", type=int, default=5)
    ap.add_argument("--loss", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_warp needs a HIP device: a time measured anywhere else says nothing")
    dev = torch.device("cuda:0")
    B, V, R, C = args.src, args.views, args.res, 3
    g = torch.Generator(device=dev).manual_seed(0)
    image = torch.rand(B, C, R, R, generator=g, device=dev)
    t = (torch.arange(R, device=dev).float() + 0.5) / R * 2 - 1
    depth = 7.667 + 0.6 * torch.sin(2.5 * t).reshape(1, 1, R) * torch.cos(2.0 * t).reshape(1, R, 1) + 0.002 * torch.randn(B, R, R, generator=g, device=dev)
    step = V + 4
    cam = synthetic.orbit_cameras(B * step, R, device=dev)          # source b is orbit view b * step, its targets the next V views
    cfg = cam["cfg"]
    src = cam["viewmatrix"][::step].contiguous()
    dst = torch.stack([cam["viewmatrix"][b * step + 1:b * step + 1 + V] for b in range(B)]).contiguous()
    FoV = cfg["model"]["fov"] * math.pi / 180
    fx = fy = R / (2 * math.tan(FoV / 2.))
    threshold = cfg["model"].get("threshold", 0.9)
    state = {"ws": None}

    def fused():
        out = warp.forward_warp(image, depth, src, dst, cfg, erode=args.erode, want_weight=True, workspace=state["ws"])
        state["ws"] = out["workspace"]
        return out

    def composite():
        return torch_composite(image, depth, warp.relative_transforms(src, dst), fx, fy, threshold=threshold, erode=args.erode)

    of, oc = fused(), composite()
    torch.cuda.synchronize()
    # the composite is float32: a pixel on a depth test may take another side there (the fragile pixels of tests/warp_truth.py), so the
    # agreement is a share of pixels and a median, not a maximum
    dw = (of["weight"] - oc["weight"]).abs()
    agree = {"weight_median_abs_diff": float(dw.median()), "weight_share_differing_by_1e-3": float((dw > 1e-3).float().mean()),
             "mask_share_differing": float((of["mask"] != oc["mask"]).float().mean())}
    agree["mask_share"] = float(of["mask"].mean())
    again = fused()
    agree["fused_bitwise_repeatable"] = all(torch.equal(of[k], again[k]) for k in ("warped", "mask", "warped_depth", "weight"))
    tf, tc = [], []
    for _ in range(2):
        timed(fused), timed(composite)
    for _ in range(args.rounds):
        tf.append(timed(fused)[0])
        tc.append(timed(composite)[0])
    f_ms, c_ms = statistics.median(tf), statistics.median(tc)
    px = B * V * R * R
    io_bytes = 4 * (B * (C + 1) * R * R + B * V * 16 + px * (C + 3))          # image, depth, rel read; warped, mask, depth, weight written
    ws_bytes = int(_lib.lib().f3dg_forward_warp_workspace_bytes(B, V, C, R, R))
    out = {"tool": "bench_warp", "device": torch.cuda.get_device_name(0), "src": B, "views": V, "res": R, "C": C, "erode": args.erode,
           "rounds": args.rounds, "fused_ms": round(f_ms, 4), "fused_min_ms": round(min(tf), 4), "torch_ms": round(c_ms, 4),
           "torch_min_ms": round(min(tc), 4), "torch_over_fused": round(c_ms / f_ms, 2), "fused_faster": f_ms < c_ms,
           "io_bytes": io_bytes, "workspace_bytes": ws_bytes, "io_GBps_fused": round(io_bytes / (f_ms * 1e-3) / 1e9, 1), "agreement": agree,
           "note": "per call of all src x views pairs, rel included in both routes; io_bytes = inputs read once + outputs written once, "
                   "workspace_bytes = accumulators + z-buffer + pre-erosion mask that the fused route also fills, updates and reads"}
    if args.loss:
        render = torch.rand(B * V, C, R, R, generator=g, device=dev).requires_grad_()

        def loss():
            render.grad = None
            losses.warping_loss(render, of["warped"], of["mask"]).backward()

        for _ in range(2):
            timed(loss)
        tl = [timed(loss)[0] for _ in range(args.rounds)]
        out["loss_fwd_bwd_ms"], out["loss_fwd_bwd_min_ms"] = round(statistics.median(tl), 4), round(min(tl), 4)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
