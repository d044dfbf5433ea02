"""Times the vertex colour baking (f3dg_mesh_bake_colors, mesh.bake_vertex_colors) on the mesh a user of the TSDF route would colour: the
256^3 TSDF mesh of the real image over its own 128-view orbit at 256^2, C = 3, with the mesh's normals and the rendered alpha. Four
routes alternate in one process after a warm-up each, device events around whole calls, the median of the rounds, the alternation twice:
    c_call     f3dg_mesh_bake_colors alone on preallocated outputs (memset, one launch, the host read of the counts)
    reused     mesh.bake_vertex_colors(..., visibility=r) with a render_mesh result handed in
    drawn      mesh.bake_vertex_colors(...) that draws its own visibility
    torch      a torch route of the same definition in float64: [V,N] intermediates, advanced-index gathers, sums over the view axis
               (no fixed order); its n_used and best_view are compared exactly, its colours by their largest difference
Also reported: the PSNR of render_mesh(..., vertex_colors=...) against the Gaussian render over the pixels both cover, once with the
volume's colours and once with the baked ones. ``--lib``: time another build of the library instead (for instance one compiled with
-DBAKE_VS=1, the plain loop of one lane per vertex over the views). Prints ONE JSON line.

    python tools/bench_mesh_color.py [--rounds 7] [--res 256] [--views 128] [--image 256] [--skip-torch] [--lib PATH]
"""
import argparse
import ctypes as C
import json
import math
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import f3dgaus_amd  # noqa: E402,F401
from f3dgaus_amd import _lib, mesh, synthetic  # noqa: E402
from f3dgaus_amd.diff_gof_rasterization import _stream  # noqa: E402
from bench_mesh_clean import timed  # noqa: E402


def torch_bake(vertices, normals, wv, fx, fy, images, face_id, depth, alpha, alpha_min, depth_tol, cos_min, z_near=0.01):
    """The definition of include/f3dg.h in torch, float64, BLEND: (colors [N,C] float32, weight, n_used, best_view). The sums over the
    views are torch.sum's: their order is not the definition's."""
    V, Cn, H, W = images.shape
    p, n, m = vertices.double(), normals.double(), wv.double()
    X, Y, Z = p[None, :, 0], p[None, :, 1], p[None, :, 2]
    row = lambda r, c: m[:, r, c][:, None]
    x = ((X * row(0, 0) + Y * row(1, 0)) + Z * row(2, 0)) + row(3, 0)
    y = ((X * row(0, 1) + Y * row(1, 1)) + Z * row(2, 1)) + row(3, 1)
    z = ((X * row(0, 2) + Y * row(1, 2)) + Z * row(2, 2)) + row(3, 2)
    u = ((fx * x) / z + W / 2.0) - 0.5
    v = ((fy * y) / z + H / 2.0) - 0.5
    fin = torch.isfinite
    ok = fin(x) & fin(y) & fin(z) & fin(u) & fin(v) & (z > z_near) & (u >= 0) & (u <= W - 1) & (v >= 0) & (v <= H - 1)
    us, vs = torch.where(ok, u, torch.zeros_like(u)), torch.where(ok, v, torch.zeros_like(v))
    view = torch.arange(V, device=p.device)[:, None].expand(V, p.shape[0])
    i, j = torch.round(us).long(), torch.round(vs).long()
    ok &= face_id[view, j, i] >= 0
    ok &= (z - depth[view, j, i].double()) <= depth_tol
    nc = [(n[None, :, 0] * row(0, c) + n[None, :, 1] * row(1, c)) + n[None, :, 2] * row(2, c) for c in range(3)]
    g = -((nc[0] * x + nc[1] * y) + nc[2] * z)
    nn = (nc[0] * nc[0] + nc[1] * nc[1]) + nc[2] * nc[2]
    pp = (x * x + y * y) + z * z
    ok &= fin(nn) & (nn > 0) & (g > 0) & (g * g >= (cos_min * cos_min) * (nn * pp))
    w = (g * g) / (nn * pp)
    i0, j0 = torch.floor(us).long(), torch.floor(vs).long()
    i1, j1 = (i0 + 1).clamp(max=W - 1), (j0 + 1).clamp(max=H - 1)
    for jj, ii in ((j0, i0), (j0, i1), (j1, i0), (j1, i1)):
        ok &= alpha[view, jj, ii].double() >= alpha_min
    a, b = (us - i0)[..., None], (vs - j0)[..., None]
    img = images.permute(0, 2, 3, 1)                                            # [V,H,W,C]
    c00, c10, c01, c11 = (img[view, jj, ii].double() for jj, ii in ((j0, i0), (j0, i1), (j1, i0), (j1, i1)))
    ok &= (fin(c00) & fin(c10) & fin(c01) & fin(c11)).all(dim=-1)
    top = c00 + a * (c10 - c00)
    bot = c01 + a * (c11 - c01)
    s = top + b * (bot - top)
    wz = torch.where(ok, w, torch.zeros_like(w))
    Sw = wz.sum(dim=0)
    S = (wz[..., None] * torch.where(ok[..., None], s, torch.zeros_like(s))).sum(dim=0)
    n_used = ok.sum(dim=0).int()
    seen = n_used > 0
    colors = torch.where(seen[:, None], S / Sw[:, None], torch.zeros_like(S)).float()
    best = torch.where(ok, w, torch.full_like(w, -1.0)).argmax(dim=0)           # the first of equal maxima is not promised by torch
    return colors, torch.where(seen, Sw, torch.zeros_like(Sw)).float(), n_used, torch.where(seen, best, torch.full_like(best, -1)).int()


def psnr(a, b, mask):
    d = (a.double() - b.double())[mask.expand_as(a)]
    return round(-10.0 * math.log10(float((d * d).mean())), 3), int(mask.sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--res", type=int, default=256)
    ap.add_argument("--views", type=int, default=128)
    ap.add_argument("--image", type=int, default=256)
    ap.add_argument("--skip-torch", action="store_true")
    ap.add_argument("--lib", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_mesh_color needs a HIP device: a time measured anywhere else says nothing")
    if args.lib:
        _lib.LIB_PATH = os.path.abspath(args.lib)
    dev = torch.device("cuda:0")
    from f3dgaus_amd.gaussian_renderer import render_views
    from real_data import real_merged_set
    g = real_merged_set(dev)
    torch.manual_seed(0)                                                        # the sample the volume's box is taken from
    pc = {k: t[None].contiguous() for k, t in g.items()}
    cams = synthetic.orbit_cameras(args.views, resolution=args.image, device=dev)
    q = torch.quantile(g["xyz"][torch.randperm(g["xyz"].shape[0], device=dev)[:100000]].double(),
                       torch.tensor([0.01, 0.99], dtype=torch.float64, device=dev), dim=0).cpu()
    lo, hi = q[0].tolist(), q[1].tolist()
    voxel = max(b - a for a, b in zip(lo, hi)) / (args.res - 9)                # the volume of tools/bench_mesh_raster.py: the central 98 %, padded
    lo = [a - 4 * voxel for a in lo]
    hi = [a + voxel * (args.res - 1) for a in lo]
    cam_args = (pc, 0, cams["viewmatrix"], cams["projmatrix"], cams["campos"], torch.zeros(3, device=dev), cams["cfg"])
    fov = cams["cfg"]["model"]["fov"]
    H = W = args.image
    m = mesh.extract_mesh_tsdf(*cam_args, resolution=args.res, bounds=(lo, hi), trunc=4 * voxel, vertex_normals=True, color_from_views=True)
    rendered = render_views(*cam_args, channels="rgb_depth_alpha", epilogue=False)
    vertices, faces, normals = m["vertices"].contiguous(), m["faces"], m["vertex_normals"]
    images, alpha = rendered["render"].contiguous(), rendered["rendered_alpha"].reshape(-1, H, W).contiguous()
    wv = cams["viewmatrix"].reshape(-1, 4, 4).contiguous()
    V, N = wv.shape[0], vertices.shape[0]
    tol = 2 * (max(b - a for a, b in zip(lo, hi)) / (args.res - 1))             # extract_mesh_tsdf's two voxels, as it forms them from the bounds
    kw = dict(vertex_normals=normals, alpha=alpha, depth_tol=tol)
    vis = mesh.render_mesh(vertices, faces, wv, fov, (H, W))
    b = mesh.bake_vertex_colors(vertices, faces, images, wv, fov, visibility=vis, **kw)
    again = mesh.bake_vertex_colors(vertices, faces, images, wv, fov, **kw)
    keys = ("vertex_colors", "weight", "n_used", "best_view")
    out = {"mesh": "real image orbit, TSDF %d^3" % args.res, "vertices": N, "faces": int(faces.shape[0]), "views": V, "image": args.image, "C": 3,
           "depth_tol": tol, "counts": b["counts"], "pairs": V * N, "hip_bitwise_repeatable": all(torch.equal(b[k], again[k]) for k in keys),
           "route_equals_direct_call": bool(torch.equal(m["color_views"], b["n_used"]) and
                                            torch.equal(m["vertex_colors"][b["n_used"] > 0], b["vertex_colors"][b["n_used"] > 0])),
           "library": _lib.LIB_PATH if args.lib else "the tree's"}

    L = _lib.lib()
    fx, fy = mesh._focal_pair(fov, H, W)
    ws = torch.empty((L.f3dg_mesh_bake_workspace_bytes(V, N, H, W),), dtype=torch.uint8, device=dev)
    o = [torch.empty((N, 3), device=dev), torch.empty((N,), device=dev), torch.empty((N,), dtype=torch.int32, device=dev),
         torch.empty((N,), dtype=torch.int32, device=dev)]
    counts = (C.c_longlong * 8)()

    def c_call():
        _lib.check(L.f3dg_mesh_bake_colors(_stream(), _lib.ptr(ws), ws.numel(), N, _lib.ptr(vertices), _lib.ptr(normals), V, _lib.ptr(wv), fx, fy, H, W,
                                           0.01, 3, _lib.ptr(images), _lib.ptr(vis["face_id"]), _lib.ptr(vis["depth"]), _lib.ptr(alpha), 0.5, tol, 0.1,
                                           0, _lib.ptr(o[0]), _lib.ptr(o[1]), _lib.ptr(o[2]), _lib.ptr(o[3]), counts), "f3dg_mesh_bake_colors")
    routes = {"c_call": c_call,
              "reused": lambda: mesh.bake_vertex_colors(vertices, faces, images, wv, fov, visibility=vis, **kw),
              "drawn": lambda: mesh.bake_vertex_colors(vertices, faces, images, wv, fov, **kw)}
    if not args.skip_torch:
        routes["torch"] = lambda: torch_bake(vertices, normals, wv, fx, fy, images, vis["face_id"], vis["depth"], alpha, 0.5, tol, 0.1)
        tc, tw, tn, tb = routes["torch"]()
        seen = b["n_used"] > 0
        out["torch_n_used_equal"] = bool(torch.equal(tn, b["n_used"]))
        out["torch_best_view_differs_at"] = int((tb != b["best_view"]).sum())
        out["torch_max_abs_color_difference"] = float((tc - b["vertex_colors"]).abs().max())
        out["torch_colors_bits_differ_at"] = int((tc.view(torch.int32) != b["vertex_colors"].view(torch.int32)).sum())
        del tc, tw, tn, tb, seen
    for fn in routes.values():
        fn()
    c_call()
    out["c_call_equals_python"] = all(torch.equal(a, b[k]) for a, k in zip(o, keys))
    runs = []
    for _ in range(2):                                                          # the whole alternation twice: run-to-run spread
        t = {k: [] for k in routes}
        for _ in range(args.rounds):
            for k, fn in routes.items():
                t[k].append(timed(fn)[0])
        runs.append({k: {"median_ms": round(statistics.median(x), 4), "min_ms": round(min(x), 4), "max_ms": round(max(x), 4)} for k, x in t.items()})
    out["timing"] = runs

    both = (vis["face_id"] >= 0)[:, None] & (rendered["rendered_alpha"].reshape(-1, 1, H, W) >= 0.5)
    quality = {}
    for label, colors in (("volume", m["vertex_colors_tsdf"]), ("baked", m["vertex_colors"])):
        drawn = mesh.render_mesh(vertices, faces, wv, fov, (H, W), vertex_colors=colors.contiguous())["color"]
        quality[label] = dict(zip(("psnr_db", "pixels"), psnr(drawn, rendered["render"], both)))
    out["psnr_vs_gaussian_render"] = quality
    print(json.dumps({"tool": "bench_mesh_color", "device": torch.cuda.get_device_name(0), "rounds": args.rounds, "result": out,
                      "note": "device events around whole calls; medians; two runs of the alternation; PSNR with peak 1 over the pixels the "
                              "mesh and the Gaussian render (alpha >= 0.5) both cover, all views"}))


if __name__ == "__main__":
    main()
