"""Times the mesh simplification, ``mesh.simplify_mesh``, on the two meshes of tools/bench_mesh_clean.py -- the 256^3 TSDF mesh of the real
image's orbit and the synthetic two-sphere mesh at 256^3 -- at cells of 2, 4 and 8 voxels, for the three placements (`quadric` with the
adjacency built inside the call and with one handed in). The comparator is a torch route of the same definition with the `mean` placement
in the same process: ``unique`` over the cell keys, ``scatter_reduce_('amin')`` for the roots, ``index_add_`` in float64 for the means,
``unique`` over the sorted cluster triples for the duplicates, mask / cumsum renumbering. Its integer outputs must equal the library's; its
means differ in the last bits (``index_add_`` adds in arrival order), the largest difference is reported. Both routes alternate in one
process after a warm-up call each; device events around whole calls (both hold host reads, so the host clock is reported as well); the
median of the rounds. Prints ONE JSON line.

    python tools/bench_mesh_simplify.py [--rounds 7] [--res 256] [--views 128] [--image 256] [--cells 2,4,8] [--skip-real]
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


def torch_simplify_mean(vertices, faces, origin, cell, colors):
    """The definition in torch with the `mean` placement: (vertices, faces, colours, vertex_map, cluster_root, counts)."""
    N, F, dev = vertices.shape[0], faces.shape[0], vertices.device
    p64 = vertices.double()
    c = torch.floor((p64 - origin) / cell).long()
    key = c[:, 0] | (c[:, 1] << 21) | (c[:, 2] << 42)
    _, inv = torch.unique(key, return_inverse=True)
    K = int(inv.max()) + 1
    ids = torch.arange(N, device=dev)
    root = torch.full((K,), N, dtype=torch.int64, device=dev).scatter_reduce_(0, inv, ids, "amin")
    size = torch.bincount(inv, minlength=K)
    mean = torch.zeros((K, 3), dtype=torch.float64, device=dev).index_add_(0, inv, p64) / size[:, None]
    col = torch.zeros((K, colors.shape[1]), dtype=torch.float64, device=dev).index_add_(0, inv, colors.double()) / size[:, None]
    dead = (faces[:, 0] == faces[:, 1]) | (faces[:, 1] == faces[:, 2]) | (faces[:, 0] == faces[:, 2])
    g = inv[faces]
    collapsed = ~dead & ((g[:, 0] == g[:, 1]) | (g[:, 1] == g[:, 2]) | (g[:, 0] == g[:, 2]))
    live = torch.nonzero(~dead & ~collapsed).reshape(-1)
    _, tinv = torch.unique(torch.sort(g[live], dim=1)[0], dim=0, return_inverse=True)
    first = torch.full((int(tinv.max()) + 1 if live.numel() else 0,), F, dtype=torch.int64, device=dev).scatter_reduce_(0, tinv, live, "amin")
    kept = torch.sort(first)[0]
    used = torch.zeros(K, dtype=torch.bool, device=dev)
    used[g[kept].reshape(-1)] = True
    # the output vertices are numbered by ascending root, the clusters of `unique` by ascending key
    order = torch.argsort(torch.where(used, root, torch.full_like(root, N)))
    n = int(used.sum())
    order = order[:n]
    new_id = torch.full((K,), -1, dtype=torch.int64, device=dev)
    new_id[order] = torch.arange(n, device=dev)
    counts = {"clusters": K, "used_clusters": n, "degenerate": int(dead.sum()), "collapsed": int(collapsed.sum()),
              "duplicate": int(live.numel() - kept.numel()), "kept": int(kept.numel()), "max_cluster": int(size.max())}
    return mean[order].float(), new_id[g[kept]], col[order].float(), new_id[inv], root[order], counts


def measure(name, vertices, faces, colors, voxel, cells, rounds):
    N, F = vertices.shape[0], faces.shape[0]
    origin = vertices.amin(dim=0).double()
    adjacency = mesh.mesh_adjacency(faces, N)
    rows = []
    for k in cells:
        cell = k * voxel
        call = lambda placement, adj=None: mesh.simplify_mesh(vertices, faces, cell, placement=placement, vertex_colors=colors, adjacency=adj)
        ref = lambda: torch_simplify_mean(vertices, faces, origin, cell, colors)
        a, b = call("mean"), ref()                              # warm-up, and the two routes give one mesh
        same = (torch.equal(a["faces"], b[1]) and torch.equal(a["vertex_map"], b[3]) and torch.equal(a["cluster_root"], b[4])
                and a["counts"] == b[5])
        diff = float((a["vertices"].double() - b[0].double()).abs().max()) if a["vertices"].numel() else 0.0
        again = call("mean")
        repeatable = all(torch.equal(a[x], again[x]) for x in ("vertices", "faces", "vertex_colors", "vertex_map"))
        q = call("quadric")
        moved = float((q["vertices"].double() - a["vertices"].double()).norm(dim=1).max()) if q["vertices"].numel() else 0.0
        routes = {"root": lambda: call("root"), "mean": lambda: call("mean"), "quadric": lambda: call("quadric"),
                  "quadric_adjacency_given": lambda: call("quadric", adjacency), "torch_mean": ref}
        for fn in routes.values():
            fn()
        t = {r: ([], []) for r in routes}
        for _ in range(rounds):
            for r, fn in routes.items():
                d, h, _ = timed(fn)
                t[r][0].append(d)
                t[r][1].append(h)
        row = {"cell_voxels": k, "cell": cell, "counts": a["counts"], "integer_outputs_agree": same, "largest_mean_difference": diff,
               "hip_bitwise_repeatable": repeatable, "largest_quadric_step": moved}
        for r in routes:
            row[r + "_ms"] = round(statistics.median(t[r][0]), 4)
            row[r + "_min_ms"] = round(min(t[r][0]), 4)
            row[r + "_host_ms"] = round(statistics.median(t[r][1]), 4)
        row["torch_over_hip_mean"] = round(row["torch_mean_ms"] / row["mean_ms"], 2)
        rows.append(row)
    return {"mesh": name, "vertices": N, "faces": F, "voxel": voxel, "cells": rows}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--res", type=int, default=256)
    ap.add_argument("--views", type=int, default=128)
    ap.add_argument("--image", type=int, default=256)
    ap.add_argument("--cells", default="2,4,8")
    ap.add_argument("--skip-real", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_mesh_simplify needs a HIP device: a time measured anywhere else says nothing")
    dev = torch.device("cuda:0")
    cells = [float(x) for x in args.cells.split(",")]
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
        results.append(measure("real image orbit, TSDF %d^3" % args.res, m["vertices"], m["faces"], m["vertex_colors"], voxel, cells, args.rounds))
        del m, pc, g
    m = two_spheres(args.res, dev)
    colors = m["vertex_colors"] if m["vertex_colors"] is not None else torch.rand((m["vertices"].shape[0], 3), device=dev)
    results.append(measure("two analytic spheres, TSDF %d^3" % args.res, m["vertices"], m["faces"], colors, 1.0, cells, args.rounds))
    print(json.dumps({"tool": "bench_mesh_simplify", "device": torch.cuda.get_device_name(0), "rounds": args.rounds, "results": results,
                      "note": "hip = mesh.simplify_mesh (root / mean / quadric; quadric builds the adjacency inside the call unless it is given), "
                              "torch_mean = unique + scatter_reduce + index_add_ + unique(dim=0); *_ms: device events around whole calls, "
                              "*_host_ms: host clock around the same calls (both routes hold host reads); medians"}))


if __name__ == "__main__":
    main()
