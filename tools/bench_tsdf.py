"""Times the TSDF mesh route at the shape a user of the demo would run: the real image's merged Gaussians (tests/real_data.py), its 128-view
orbit rendered at 256 x 256 (``render_views(..., channels="rgb_depth_alpha", epilogue=False)``) and a 256^3 volume around the central
98 % of the Gaussians. ``TSDFVolume.integrate`` (f3dg_tsdf_integrate: one launch for the 128 views) against a float32 torch composite of
the same definition on the same device -- index arithmetic plus gathers, ``--chunk`` views batched per step -- both from an empty volume;
then the cell entries, marching tetrahedra and the vertex kernel of ``extract``. The parent of this feature had no TSDF route, so the
composite is the baseline. Prints ONE JSON line. Device events around runs that end in a synchronise; both routes alternate in one
process; the median of the rounds is reported, with the volume's own traffic (one read plus one write of its 24 B per voxel).

    python tools/bench_tsdf.py [--rounds 7] [--res 256] [--views 128] [--image 256] [--chunk 8]
"""
import argparse
import json
import math
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import f3dgaus_amd  # noqa: E402,F401
from f3dgaus_amd import mesh, synthetic, tsdf  # noqa: E402


def torch_integrate(vol, depth, color, alpha, wv, fx, fy, z_near, alpha_min, chunk):
    """The definition of include/f3dg.h in float32 torch operations on an EMPTY volume: returns (tsdf, weight, color, color_weight)."""
    nx, ny, nz = vol.dims
    dev = depth.device
    V, H, W = depth.shape
    HW = H * W
    ax = lambda n, o: o + vol.voxel_size * torch.arange(n, device=dev, dtype=torch.float32)
    z, y, x = torch.meshgrid(ax(nz, vol.origin[2]), ax(ny, vol.origin[1]), ax(nx, vol.origin[0]), indexing="ij")
    p = torch.stack([x.reshape(-1), y.reshape(-1), z.reshape(-1)], 1)                    # [N,3]
    N = p.shape[0]
    S, n = torch.zeros(N, device=dev), torch.zeros(N, device=dev)
    Cs, nc = torch.zeros(3, N, device=dev), torch.zeros(N, device=dev)
    dflat, aflat, cflat = depth.reshape(-1), alpha.reshape(-1), color.reshape(V, 3, HW)
    for v0 in range(0, V, chunk):
        M = wv[v0:v0 + chunk]
        c = M.shape[0]
        cam = p.unsqueeze(0) @ M[:, :3, :3] + M[:, 3:4, :3]                             # [c,N,3]
        X, Y, Z = cam[..., 0], cam[..., 1], cam[..., 2]
        front = Z > z_near
        Zs = torch.where(front, Z, 1.0)
        u, w = fx * X / Zs + W / 2, fy * Y / Zs + H / 2
        inside = front & (u >= 0) & (u < W) & (w >= 0) & (w < H)
        i, j = torch.where(inside, u, 0.0).floor().long(), torch.where(inside, w, 0.0).floor().long()
        pix = j * W + i
        gpix = pix + (torch.arange(v0, v0 + c, device=dev) * HW).reshape(c, 1)
        d = dflat[gpix]
        live = inside & torch.isfinite(d) & (d > 0) & (aflat[gpix] >= alpha_min)
        sdf = torch.where(live, d, 1.0) - Z
        live = live & ~(sdf < -vol.trunc)
        S += torch.where(live, (sdf / vol.trunc).clamp(max=1.0), 0.0).sum(0)
        n += live.sum(0)
        col = live & (sdf.abs() <= vol.trunc)
        for ch in range(3):
            Cs[ch] += torch.where(col, torch.gather(cflat[v0:v0 + c, ch], 1, pix), 0.0).sum(0)
        nc += col.sum(0)
    seen, cseen = n > 0, nc > 0
    shape = (nz, ny, nx)
    return (torch.where(seen, S / n.clamp(min=1), 0.0).reshape(shape), n.reshape(shape),
            torch.where(cseen, Cs / nc.clamp(min=1), 0.0).reshape((3,) + shape), nc.reshape(shape))


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), out


def host_timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--res", type=int, default=256)
    ap.add_argument("--views", type=int, default=128)
    ap.add_argument("--image", type=int, default=256)
    ap.add_argument("--chunk", type=int, default=8)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_tsdf needs a HIP device: a time measured anywhere else says nothing")
    dev = torch.device("cuda:0")
    R, V, n = args.image, args.views, args.res
    from real_data import real_merged_set
    g = real_merged_set(dev)
    pc = {k: t[None].contiguous() for k, t in g.items()}
    cams = synthetic.orbit_cameras(V, resolution=R, device=dev)
    cfg = cams["cfg"]
    bg = torch.zeros(3, device=dev)
    with torch.no_grad():
        out = f3dgaus_amd.render_views(pc, 0, cams["viewmatrix"], cams["projmatrix"], cams["campos"], bg, cfg, channels="rgb_depth_alpha", epilogue=False)
    depth, alpha, color = out["rendered_depth"][:, 0].contiguous(), out["rendered_alpha"][:, 0].contiguous(), out["render"].contiguous()
    wv = cams["viewmatrix"].reshape(V, 4, 4).contiguous()
    q = torch.quantile(g["xyz"][torch.randperm(g["xyz"].shape[0], device=dev)[:100000]].double(), torch.tensor([0.01, 0.99], dtype=torch.float64, device=dev), dim=0).cpu()
    lo, hi = q[0].tolist(), q[1].tolist()
    voxel = max(b - a for a, b in zip(lo, hi)) / (n - 9)
    lo = [a - 4 * voxel for a in lo]
    vol = tsdf.TSDFVolume(lo, voxel, (n, n, n), device=dev)
    FoV = cfg["model"]["fov"] * math.pi / 180
    fx = fy = R / (2 * math.tan(FoV / 2.))
    z_near, alpha_min = 0.01, 0.5

    def fused():
        vol.reset()
        return timed(lambda: vol.integrate(depth, wv, (fx, fy), color=color, alpha=alpha, alpha_min=alpha_min, z_near=z_near))[0]

    def composite():
        return timed(lambda: torch_integrate(vol, depth, color, alpha, wv, fx, fy, z_near, alpha_min, args.chunk))

    fused()
    first = {k: getattr(vol, k).clone() for k in ("tsdf", "weight", "color", "color_weight")}
    _, ref = composite()
    # the composite is float32: a voxel on a floor or a band test may take another side there (the fragile voxels of tests/tsdf_truth.py),
    # so the agreement is a share of voxels and a median, not a maximum
    both = (first["weight"] > 0) & (ref[1] > 0)
    agree = {"observed_share": float((first["weight"] > 0).float().mean()),
             "weight_share_differing": float((first["weight"] != ref[1]).float().mean()),
             "tsdf_median_abs_diff_where_weights_agree": float((first["tsdf"] - ref[0]).abs()[both & (first["weight"] == ref[1])].median()),
             "color_weight_share_differing": float((first["color_weight"] != ref[3]).float().mean())}
    fused()
    agree["fused_bitwise_repeatable"] = all(torch.equal(first[k], getattr(vol, k)) for k in first)
    del ref
    tf, tc = [], []
    for _ in range(args.rounds):
        tf.append(fused())
        tc.append(composite()[0])
    f_ms, c_ms = statistics.median(tf), statistics.median(tc)
    # the rest of the route on the fused volume: cells, marching tetrahedra, vertices (host clock: the entries hold blocking reads)
    parts = {"cells_ms": [], "marching_tets_ms": [], "vertices_ms": []}
    sizes = {}
    for _ in range(max(3, args.rounds // 2)):
        t_cells, tets = host_timed(lambda: vol.surface_tets())
        sdf = -vol.tsdf.reshape(-1)
        t_mt, (iv, faces) = host_timed(lambda: mesh.marching_tets_topology(sdf, tets))
        t_all, m = host_timed(lambda: vol.extract())
        parts["cells_ms"].append(t_cells)
        parts["marching_tets_ms"].append(t_mt)
        parts["vertices_ms"].append(max(0.0, t_all - t_cells - t_mt))
        sizes = {"active_cells": int(tets.shape[0] // 6), "edges": int(iv.shape[0]), "faces": int(faces.shape[0])}
    N = n ** 3
    vol_bytes = 2 * 24 * N
    out = {"tool": "bench_tsdf", "device": torch.cuda.get_device_name(0), "data": "real", "volume": [n, n, n], "views": V, "image": R,
           "chunk": args.chunk, "rounds": args.rounds, "fused_ms": round(f_ms, 4), "fused_min_ms": round(min(tf), 4), "fused_max_ms": round(max(tf), 4),
           "torch_ms": round(c_ms, 3), "torch_min_ms": round(min(tc), 3), "torch_over_fused": round(c_ms / f_ms, 2), "fused_faster": f_ms < c_ms,
           "volume_bytes": vol_bytes, "volume_GBps_fused": round(vol_bytes / (f_ms * 1e-3) / 1e9, 1),
           "voxel_view_samples_per_s_fused": round(N * V / (f_ms * 1e-3) / 1e9, 2),
           **{k: round(statistics.median(v), 3) for k, v in parts.items()}, **sizes, "agreement": agree,
           "note": "integrate: per call of all views into an empty volume (the reset is outside the timed window); volume_bytes = one read plus one "
                   "write of 24 B per voxel; voxel_view_samples_per_s in 1e9/s; vertices_ms = extract minus its cells and marching-tets parts"}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
