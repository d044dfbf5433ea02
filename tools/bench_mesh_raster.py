"""Times mesh.render_mesh with colours and normals (C = 6) on the two meshes a user of the TSDF route would draw: the 256^3 TSDF mesh of the
real image over its own orbit at 256^2 and the synthetic two-sphere mesh at 256^3 (the meshes of tools/bench_mesh_smooth.py, built the
same way; the two spheres are moved in front of the orbit's cameras) at 512^2. The comparator is a torch route of the same definition in
the same process, since the parent of this feature drew no mesh: per view, the dense int64 edge functions of faces x pixels in chunks,
depth and key on the covered pairs in float64, visibility by scatter_reduce_('amin') on the packed key. It is timed on ONE view per round
(a view of the two spheres takes seconds), and only where a warm-up view fits ``--torch-seconds``. Both routes alternate in one process after a warm-up each; device events around whole
calls; the median of the rounds; the alternation runs twice. Also reported: the share of (view, face) pairs whose box holds no pixel
centre, and the depth agreement of the real mesh against the Gaussian render with and without ten Taubin iterations. Prints ONE JSON
line.

    python tools/bench_mesh_raster.py [--rounds 7] [--res 256] [--views 128] [--image 256] [--sphere-views 8] [--sphere-image 512]
                                      [--torch-seconds 20] [--skip-real] [--skip-torch]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import f3dgaus_amd  # noqa: E402,F401
from f3dgaus_amd import mesh, synthetic  # noqa: E402
from bench_mesh_clean import timed, two_spheres  # noqa: E402

I64_MAX = (1 << 63) - 1
CHUNK_PAIRS = 1 << 26               # (face, pixel) pairs of one dense chunk


def torch_view(vertices, faces, m, fx, fy, H, W, z_near, keys, budget_s=None):
    """One view of the definition in torch: ``keys`` [H W] int64 (I64_MAX: empty) receives the packed winners. Returns the number of
    faces processed (all of them unless ``budget_s`` ran out first)."""
    p, m = vertices.double(), m.double()
    X, Y, Z = p[:, 0], p[:, 1], p[:, 2]
    x = ((X * m[0, 0] + Y * m[1, 0]) + Z * m[2, 0]) + m[3, 0]
    y = ((X * m[0, 1] + Y * m[1, 1]) + Z * m[2, 1]) + m[3, 1]
    z = ((X * m[0, 2] + Y * m[1, 2]) + Z * m[2, 2]) + m[3, 2]
    u = ((fx * x) / z + W / 2.0) - 0.5
    v = ((fy * y) / z + H / 2.0) - 0.5
    ok = torch.isfinite(x) & torch.isfinite(y) & torch.isfinite(z) & (z > z_near) & torch.isfinite(u) & torch.isfinite(v) & (u.abs() <= 16384) & (v.abs() <= 16384)
    U = torch.where(ok, torch.round(256.0 * u), torch.zeros_like(u)).long()
    Vs = torch.where(ok, torch.round(256.0 * v), torch.zeros_like(v)).long()
    q = 1.0 / z
    pix = torch.arange(H * W, device=vertices.device)
    Px, Py = (256 * (pix % W))[None], (256 * (pix // W))[None]
    step = max(1, CHUNK_PAIRS // (H * W))
    t0, done = time.perf_counter(), 0
    for f0 in range(0, faces.shape[0], step):
        f = faces[f0:f0 + step]
        i0, i1, i2 = f[:, 0], f[:, 1], f[:, 2]
        area = (U[i1] - U[i0]) * (Vs[i2] - Vs[i0]) - (Vs[i1] - Vs[i0]) * (U[i2] - U[i0])
        live = ok[i0] & ok[i1] & ok[i2] & (area != 0) & (i0 != i1) & (i1 != i2) & (i0 != i2)
        s = torch.sign(area)
        inside = live[:, None].expand(-1, H * W)
        E = []
        for a, b in ((i0, i1), (i1, i2), (i2, i0)):             # the face's own edges, the orientation as a sign
            du, dv = (s * (U[b] - U[a]))[:, None], (s * (Vs[b] - Vs[a]))[:, None]
            e = du * (Py - Vs[a][:, None]) - dv * (Px - U[a][:, None])
            inside = inside & ((e > 0) | ((e == 0) & ((dv > 0) | ((dv == 0) & (du < 0)))))
            E.append(e)
        fi, pi = torch.nonzero(inside, as_tuple=True)           # the covered pairs: depth and key on them only
        if fi.numel():
            absA = area.abs().double()[fi]
            w = [E[1][fi, pi].double() / absA, E[2][fi, pi].double() / absA, E[0][fi, pi].double() / absA]     # opposite corners 0, 1, 2
            D = (w[0] * q[i0[fi]] + w[1] * q[i1[fi]]) + w[2] * q[i2[fi]]
            bits = (1.0 / D).float().view(torch.int32).long()
            keys.scatter_reduce_(0, pi, (bits << 32) | (fi + f0), "amin")
        done = min(f0 + step, faces.shape[0])
        if budget_s is not None:
            torch.cuda.synchronize()
            if time.perf_counter() - t0 > budget_s:
                break
    return done


def alternate(hip, ref, rounds):
    runs = []
    for _ in range(2):                                          # the whole alternation twice: run-to-run spread
        th, tt = [], []
        for _ in range(rounds):
            th.append(timed(hip)[0])
            if ref is not None:
                tt.append(timed(ref)[0])
        r = {"hip_ms": round(statistics.median(th), 4), "hip_min_ms": round(min(th), 4), "hip_max_ms": round(max(th), 4)}
        if tt:
            r.update(torch_ms_per_view=round(statistics.median(tt), 3), torch_min_ms_per_view=round(min(tt), 3))
        runs.append(r)
    return runs


def measure(name, vertices, faces, colors, normals, wv, fov, image, rounds, torch_seconds):
    V, F = wv.shape[0], faces.shape[0]
    vertices, colors, normals = vertices.detach().contiguous(), colors.detach().contiguous(), normals.detach().contiguous()
    draw = lambda: mesh.render_mesh(vertices, faces, wv, fov, image, vertex_colors=colors, vertex_normals=normals)
    r = draw()
    again = draw()
    c = r["counts"]
    out = {"mesh": name, "vertices": vertices.shape[0], "faces": F, "views": V, "image": image, "counts": c,
           "covered_fraction": round(c["covered"] / (V * image * image), 4),
           "hip_bitwise_repeatable": all(torch.equal(r[k], again[k]) for k in ("face_id", "depth", "bary", "color", "normal")),
           "workspace_MB": round(f3dgaus_amd._lib.lib().f3dg_mesh_raster_workspace_bytes(V, F, image, image) / 2 ** 20, 1)}
    ref = None
    if torch_seconds > 0:
        fx, fy = mesh._focal_pair(fov, image, image)
        keys = torch.full((image * image,), I64_MAX, dtype=torch.int64, device=vertices.device)
        done = torch_view(vertices, faces, wv[0], fx, fy, image, image, 0.01, keys, budget_s=torch_seconds)      # warm-up, and does a view fit?
        out["torch_faces_done_in_budget"] = done
        if done == F:
            fid = torch.where(keys != I64_MAX, keys & 0xFFFFFFFF, torch.full_like(keys, -1)).reshape(image, image)
            dep = torch.where(keys != I64_MAX, keys >> 32, torch.zeros_like(keys)).int().view(torch.float32).reshape(image, image)
            out["torch_view0_face_id_equal"] = bool(torch.equal(fid, r["face_id"][0].long()))
            out["torch_view0_depth_bits_equal"] = bool(torch.equal(dep.view(torch.int32), r["depth"][0].view(torch.int32)))

            def ref():
                keys.fill_(I64_MAX)
                torch_view(vertices, faces, wv[0], fx, fy, image, image, 0.01, keys)
        else:
            out["torch_route"] = "not timed: one view does not fit --torch-seconds"
    out["timing"] = alternate(draw, ref, rounds)
    if ref is not None:
        hip = statistics.median(x["hip_ms"] for x in out["timing"])
        out["torch_all_views_over_hip"] = round(statistics.median(x["torch_ms_per_view"] for x in out["timing"]) * V / hip, 1)
    return out


def empty_box_share(vertices, faces, wv, fov, image):
    """The share of rasterised (view, face) pairs whose box of pixel centres is empty, from the snapped corners (torch, float64)."""
    fx, fy = mesh._focal_pair(fov, image, image)
    p = vertices.double()
    empty = total = 0
    for m in wv.double():
        x = ((p[:, 0] * m[0, 0] + p[:, 1] * m[1, 0]) + p[:, 2] * m[2, 0]) + m[3, 0]
        y = ((p[:, 0] * m[0, 1] + p[:, 1] * m[1, 1]) + p[:, 2] * m[2, 1]) + m[3, 1]
        z = ((p[:, 0] * m[0, 2] + p[:, 1] * m[1, 2]) + p[:, 2] * m[2, 2]) + m[3, 2]
        U = torch.round(256.0 * (((fx * x) / z + image / 2.0) - 0.5)).long()[faces]
        Vs = torch.round(256.0 * (((fy * y) / z + image / 2.0) - 0.5)).long()[faces]
        area = (U[:, 1] - U[:, 0]) * (Vs[:, 2] - Vs[:, 0]) - (Vs[:, 1] - Vs[:, 0]) * (U[:, 2] - U[:, 0])
        live = (z[faces] > 0.01).all(dim=1) & (area != 0)
        lo = lambda a: torch.clamp(-((-a.min(dim=1)[0]) // 256), min=0)
        hi = lambda a: torch.clamp(a.max(dim=1)[0] // 256, max=image - 1)
        none = (hi(U) < lo(U)) | (hi(Vs) < lo(Vs))
        empty += int((none & live).sum())
        total += int(live.sum())
    return round(empty / max(total, 1), 4), total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--res", type=int, default=256)
    ap.add_argument("--views", type=int, default=128)
    ap.add_argument("--image", type=int, default=256)
    ap.add_argument("--sphere-views", type=int, default=8)
    ap.add_argument("--sphere-image", type=int, default=512)
    ap.add_argument("--torch-seconds", type=float, default=20.0)
    ap.add_argument("--skip-real", action="store_true")
    ap.add_argument("--skip-torch", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_mesh_raster needs a HIP device: a time measured anywhere else says nothing")
    dev = torch.device("cuda:0")
    budget = 0.0 if args.skip_torch else args.torch_seconds
    results = []
    if not args.skip_real:
        from f3dgaus_amd.gaussian_renderer import render_views
        from real_data import real_merged_set
        g = real_merged_set(dev)
        torch.manual_seed(0)                                                        # the sample the volume's box is taken from
        pc = {k: t[None].contiguous() for k, t in g.items()}
        cams = synthetic.orbit_cameras(args.views, resolution=args.image, device=dev)
        q = torch.quantile(g["xyz"][torch.randperm(g["xyz"].shape[0], device=dev)[:100000]].double(),
                           torch.tensor([0.01, 0.99], dtype=torch.float64, device=dev), dim=0).cpu()
        lo, hi = q[0].tolist(), q[1].tolist()
        voxel = max(b - a for a, b in zip(lo, hi)) / (args.res - 9)                # the volume of tools/bench_tsdf.py: the central 98 %, padded
        lo = [a - 4 * voxel for a in lo]
        hi = [a + voxel * (args.res - 1) for a in lo]
        cam_args = (pc, 0, cams["viewmatrix"], cams["projmatrix"], cams["campos"], torch.zeros(3, device=dev), cams["cfg"])
        fov = cams["cfg"]["model"]["fov"]
        rendered = render_views(*cam_args, channels="rgb_depth_alpha", epilogue=False)
        agreement = {}
        for label, it in (("raw", None), ("smooth_iterations=10", 10)):
            m = mesh.extract_mesh_tsdf(*cam_args, resolution=args.res, bounds=(lo, hi), trunc=4 * voxel, smooth_iterations=it, vertex_normals=True)
            d = mesh.render_mesh(m["vertices"], m["faces"], cams["viewmatrix"], fov, args.image)
            agreement[label] = mesh.mesh_depth_agreement(d["depth"], d["alpha"], rendered["rendered_depth"], rendered["rendered_alpha"])
            if it is None:
                raw = m
        res = measure("real image orbit, TSDF %d^3" % args.res, raw["vertices"], raw["faces"], raw["vertex_colors"], raw["vertex_normals"],
                         cams["viewmatrix"].reshape(-1, 4, 4).contiguous(), fov, args.image, args.rounds, budget)
        res["depth_agreement_vs_gaussian_render"] = agreement
        res["empty_box_share"], res["pairs_in_front"] = empty_box_share(raw["vertices"], raw["faces"], cams["viewmatrix"].reshape(-1, 4, 4), fov, args.image)
        results.append(res)
        del m, raw, pc, g, rendered
    m = two_spheres(args.res, dev)
    cams = synthetic.orbit_cameras(args.sphere_views, resolution=args.sphere_image, device=dev)
    fov = cams["cfg"]["model"]["fov"]
    # the body of radius 14 / 48 res voxels becomes 0.35 world units, in front of the orbit's cameras
    vertices = (m["vertices"] * (0.35 / (14.0 / 48.0 * args.res)) + torch.tensor([0.0, 0.0, 7.667], device=dev)).float().contiguous()
    normals = mesh.vertex_normals(vertices, m["faces"])
    colors = torch.rand(vertices.shape, device=dev, generator=torch.Generator(device=dev).manual_seed(1))
    wv = cams["viewmatrix"].reshape(-1, 4, 4).contiguous()
    res = measure("two analytic spheres, TSDF %d^3" % args.res, vertices, m["faces"], colors, normals, wv, fov, args.sphere_image, args.rounds, budget)
    res["empty_box_share"], res["pairs_in_front"] = empty_box_share(vertices, m["faces"], wv, fov, args.sphere_image)
    results.append(res)
    print(json.dumps({"tool": "bench_mesh_raster", "device": torch.cuda.get_device_name(0), "rounds": args.rounds, "results": results,
                      "note": "hip = mesh.render_mesh with colours and normals (C = 6), ALL views in one call; torch = the dense edge functions of ONE "
                              "view in chunks + scatter_reduce_('amin'); device events around whole calls; medians; two runs of the alternation"}))


if __name__ == "__main__":
    main()
