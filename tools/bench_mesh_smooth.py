"""Times mesh smoothing and vertex normals on the two meshes a user of the TSDF route would smooth: the 256^3 TSDF mesh of the real image's
orbit and the synthetic two-sphere mesh at 256^3 (the meshes of tools/bench_mesh_clean.py, built the same way). Three parts, each against a
torch route of the same definition in the same process:
    adjacency   mesh.mesh_adjacency                          vs  torch.unique over the packed directed edges + bincount
    smoothing   mesh.smooth_mesh, 10 Taubin iterations       vs  20 steps of index_add_ over the unique directed edges, in float64
    normals     mesh.vertex_normals                          vs  float64 face cross products, index_add_ to the corners, normalise
The torch sums add with float atomics in no fixed order, so they agree with the HIP route to float64 rounding, not to the bit; the largest
difference is reported. Both routes alternate in one process after a warm-up call each; device events around whole calls and the host clock
around the same calls (the adjacency build and torch.unique hold host reads); the median of the rounds; the alternation runs twice. Prints
ONE JSON line.

    python tools/bench_mesh_smooth.py [--rounds 7] [--res 256] [--views 128] [--image 256] [--skip-real]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import f3dgaus_amd  # noqa: E402,F401
from f3dgaus_amd import mesh, synthetic  # noqa: E402
from bench_mesh_clean import timed, two_spheres  # noqa: E402


def torch_adjacency(faces, N):
    """(src, dst) of the unique directed edges, deg [N], boundary [N] bool."""
    live = ~((faces[:, 0] == faces[:, 1]) | (faces[:, 1] == faces[:, 2]) | (faces[:, 0] == faces[:, 2]))
    f = faces[live]
    a = torch.cat([f[:, 0], f[:, 1], f[:, 2], f[:, 1], f[:, 2], f[:, 0]])
    b = torch.cat([f[:, 1], f[:, 2], f[:, 0], f[:, 0], f[:, 1], f[:, 2]])
    pairs, count = torch.unique(a * N + b, return_counts=True)
    src, dst = pairs // N, pairs % N
    deg = torch.bincount(src, minlength=N)
    boundary = torch.zeros(N, dtype=torch.bool, device=faces.device)
    boundary[src[count == 1]] = True
    return src, dst, deg, boundary


def torch_smooth(vertices, src, dst, deg, pinned, iterations, lam, mu):
    move = ((deg > 0) & ~pinned)[:, None]
    d = deg.clamp(min=1).to(torch.float64)[:, None]
    P = vertices
    for _ in range(iterations):
        for s in (lam, mu):
            s64 = float(torch.tensor(s, dtype=torch.float32))
            p64 = P.to(torch.float64)
            S = torch.zeros_like(p64).index_add_(0, src, p64[dst])
            P = torch.where(move, p64 + s64 * (S / d - p64), p64).to(torch.float32)
    return P


def torch_normals(vertices, faces):
    p = vertices.to(torch.float64)
    live = ~((faces[:, 0] == faces[:, 1]) | (faces[:, 1] == faces[:, 2]) | (faces[:, 0] == faces[:, 2]))
    f = faces[live]
    c = torch.cross(p[f[:, 1]] - p[f[:, 0]], p[f[:, 2]] - p[f[:, 0]], dim=1)
    S = torch.zeros_like(p)
    for k in range(3):
        S.index_add_(0, f[:, k], c)
    n = S.norm(dim=1, keepdim=True)
    return torch.where((n > 0) & torch.isfinite(n), S / n, torch.zeros_like(S)).to(torch.float32)


def alternate(hip, ref, rounds):
    runs = []
    for _ in range(2):                                          # the whole alternation twice: run-to-run spread
        th, tt, hh, ht = [], [], [], []
        for _ in range(rounds):
            d, h, _ = timed(hip)
            th.append(d)
            hh.append(h)
            d, h, _ = timed(ref)
            tt.append(d)
            ht.append(h)
        runs.append({"hip_ms": round(statistics.median(th), 4), "hip_min_ms": round(min(th), 4), "hip_max_ms": round(max(th), 4),
                     "hip_host_ms": round(statistics.median(hh), 4), "torch_ms": round(statistics.median(tt), 4), "torch_min_ms": round(min(tt), 4),
                     "torch_host_ms": round(statistics.median(ht), 4), "torch_over_hip": round(statistics.median(tt) / statistics.median(th), 2)})
    return runs


def measure(name, vertices, faces, rounds, iterations=10, lam=0.5, mu=-0.53):
    N, F = vertices.shape[0], faces.shape[0]
    vertices = vertices.detach().contiguous()
    a = mesh.mesh_adjacency(faces, N)                           # warm-up of both routes, and the two give one mesh
    src, dst, deg, bnd = torch_adjacency(faces, N)
    start = a["nbr_start"].to(torch.int64)
    same_adj = torch.equal(a["nbr"].to(torch.int64), dst) and torch.equal(start[1:] - start[:-1], deg) and torch.equal(a["boundary"], bnd)
    hs = mesh.smooth_mesh(vertices, faces, iterations=iterations, lam=lam, mu=mu, adjacency=a)["vertices"]
    ts = torch_smooth(vertices, src, dst, deg, bnd, iterations, lam, mu)
    hn, tn = mesh.vertex_normals(hs, faces, adjacency=a), torch_normals(hs, faces)
    again = mesh.smooth_mesh(vertices, faces, iterations=iterations, lam=lam, mu=mu)["vertices"]
    moved = (hs - vertices).double().norm(dim=1)
    deg_f = deg.double()
    out = {"mesh": name, "vertices": N, "faces": F, "edges": a["n_edges"], "boundary_vertices": a["n_boundary_vertices"],
           "degenerate_faces": a["n_degenerate"], "longest_row_entries": a["max_row"], "mean_degree": round(float(deg_f.mean()), 3),
           "max_degree": int(deg.max()), "adjacency_routes_agree": same_adj, "smooth_max_abs_diff_vs_torch": float((hs - ts).abs().max()),
           "normals_max_abs_diff_vs_torch": float((hn - tn).abs().max()), "hip_bitwise_repeatable": torch.equal(hs, again),
           "mean_displacement": float(moved.mean()), "max_displacement": float(moved.max()),
           "bytes_per_step_model": int(N * (12 + 12 + 8) + 2 * a["n_edges"] * (4 + 12)),
           "adjacency": alternate(lambda: mesh.mesh_adjacency(faces, N), lambda: torch_adjacency(faces, N), rounds),
           "smooth": alternate(lambda: mesh.smooth_mesh(vertices, faces, iterations=iterations, lam=lam, mu=mu, adjacency=a),
                               lambda: torch_smooth(vertices, src, dst, deg, bnd, iterations, lam, mu), rounds),
           "normals": alternate(lambda: mesh.vertex_normals(hs, faces, adjacency=a), lambda: torch_normals(hs, faces), rounds)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--res", type=int, default=256)
    ap.add_argument("--views", type=int, default=128)
    ap.add_argument("--image", type=int, default=256)
    ap.add_argument("--skip-real", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_mesh_smooth needs a HIP device: a time measured anywhere else says nothing")
    dev = torch.device("cuda:0")
    results = []
    if not args.skip_real:
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
        m = mesh.extract_mesh_tsdf(pc, 0, cams["viewmatrix"], cams["projmatrix"], cams["campos"], torch.zeros(3, device=dev), cams["cfg"],
                                   resolution=args.res, bounds=(lo, hi), trunc=4 * voxel)
        results.append(measure("real image orbit, TSDF %d^3" % args.res, m["vertices"], m["faces"], args.rounds))
        del m, pc, g
    m = two_spheres(args.res, dev)
    results.append(measure("two analytic spheres, TSDF %d^3" % args.res, m["vertices"], m["faces"], args.rounds))
    print(json.dumps({"tool": "bench_mesh_smooth", "device": torch.cuda.get_device_name(0), "rounds": args.rounds, "results": results,
                      "note": "hip = mesh.mesh_adjacency / smooth_mesh (10 Taubin iterations, boundary pinned) / vertex_normals, torch = unique directed "
                              "edges + index_add_ in float64; *_ms: device events around whole calls, *_host_ms: host clock around the same calls; "
                              "medians; two runs of the alternation"}))


if __name__ == "__main__":
    main()
