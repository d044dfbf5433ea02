"""Marching tetrahedra at the mesh path's own size: the library call (f3dgaus_amd.mesh.marching_tets_topology, its two host reads
included) against the only alternative a user has without it -- the reference's algorithm as plain torch on the same device
(torch.unique(dim=0) over the six edges of every surface tetrahedron, boolean-mask indexing; src/utils_tetmesh.py:97-136).

Workload: an n^3 Kuhn-split grid (default n = 176: 5.45 M points, 32.2 M tetrahedra, just under the reference's chunk limit of 32 Mi)
with a noisy-sphere sdf. Both routes must give the same interp_v and faces (checked once). Prints one JSON line:
    {"n": ..., "points": ..., "tets": ..., "torch_ms": ..., "library_ms": ..., "ratio": torch_ms / library_ms, "E": ..., "faces": ...}

    python tools/bench_marching_tets.py [--n 176] [--repeat 5] [--int32]"""
import argparse
import itertools
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import f3dgaus_amd as f3d  # noqa: E402

TRIANGLES = [[-1, -1, -1, -1, -1, -1], [1, 0, 2, -1, -1, -1], [4, 0, 3, -1, -1, -1], [1, 4, 2, 1, 3, 4], [3, 1, 5, -1, -1, -1],
             [2, 3, 0, 2, 5, 3], [1, 4, 0, 1, 5, 4], [4, 2, 5, -1, -1, -1], [4, 5, 2, -1, -1, -1], [4, 1, 0, 4, 5, 1],
             [3, 2, 0, 3, 5, 2], [1, 3, 5, -1, -1, -1], [4, 1, 2, 4, 3, 1], [3, 0, 4, -1, -1, -1], [2, 0, 1, -1, -1, -1],
             [-1, -1, -1, -1, -1, -1]]
NUM_TRIANGLES = [0, 1, 1, 2, 1, 2, 2, 1, 1, 2, 2, 1, 2, 1, 1, 0]


def kuhn_grid(n, dev, seed=0):
    """Points, sdf and the 6 (n-1)^3 tetrahedra (rows shuffled) on the device."""
    ax = torch.linspace(0, 1, n, device=dev)
    pts = torch.stack(torch.meshgrid(ax, ax, ax, indexing="ij"), -1).reshape(-1, 3)
    c = torch.stack(torch.meshgrid(*([torch.arange(n - 1, device=dev)] * 3), indexing="ij"), -1).reshape(-1, 3)
    idx = lambda p: (p[:, 0] * n + p[:, 1]) * n + p[:, 2]
    tets = []
    for perm in itertools.permutations(range(3)):
        corner = c.clone()
        path = [idx(corner)]
        for axis in perm:
            corner = corner.clone()
            corner[:, axis] += 1
            path.append(idx(corner))
        tets.append(torch.stack(path, 1))
    tets = torch.stack(tets, 1).reshape(-1, 4)
    g = torch.Generator(device=dev).manual_seed(seed)
    tets = tets[torch.randperm(len(tets), device=dev, generator=g)].contiguous()
    sdf = 0.37 - (pts - 0.5).norm(dim=1) + 0.03 * torch.randn(len(pts), device=dev, generator=g)
    return pts, sdf.float().contiguous(), tets


def torch_route(sdf, tets):
    """The reference's steps in torch: gather the occupancy, keep the surface tetrahedra, sort and unique ALL their edges, mask the
    crossing ones, map, gather the triangle table."""
    dev = sdf.device
    tets = tets.long()
    occ = sdf > 0
    occ4 = occ[tets.reshape(-1)].reshape(-1, 4)
    s = occ4.sum(-1)
    valid = (s > 0) & (s < 4)
    base = torch.tensor([0, 1, 0, 2, 0, 3, 1, 2, 1, 3, 2, 3], device=dev)
    edges = tets[valid][:, base].reshape(-1, 2)
    edges = torch.sort(edges, dim=1)[0]
    uniq, inverse = torch.unique(edges, dim=0, return_inverse=True)
    crossing = occ[uniq.reshape(-1)].reshape(-1, 2).sum(-1) == 1
    mapping = torch.full((len(uniq),), -1, dtype=torch.long, device=dev)
    mapping[crossing] = torch.arange(int(crossing.sum()), device=dev)
    rows = mapping[inverse].reshape(-1, 6)
    interp_v = uniq[crossing]
    case = (occ4[valid] * torch.tensor([1, 2, 4, 8], device=dev)).sum(-1)
    nt = torch.tensor(NUM_TRIANGLES, device=dev)[case]
    table = torch.tensor(TRIANGLES, device=dev)
    faces = torch.cat((torch.gather(rows[nt == 1], 1, table[case[nt == 1]][:, :3]).reshape(-1, 3),
                       torch.gather(rows[nt == 2], 1, table[case[nt == 2]][:, :6]).reshape(-1, 3)), 0)
    return interp_v, faces


def timed(fn, repeat):
    fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(repeat):
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    return sorted(times)[len(times) // 2], out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=176)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--int32", action="store_true", help="hand the library int32 tetrahedra (the torch route always indexes with int64)")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    pts, sdf, tets = kuhn_grid(a.n, dev)
    lib_tets = tets.int() if a.int32 else tets
    lib_ms, (iv, fc) = timed(lambda: f3d.mesh.marching_tets_topology(sdf, lib_tets), a.repeat)
    torch_ms, (iv_t, fc_t) = timed(lambda: torch_route(sdf, tets), a.repeat)
    assert torch.equal(iv, iv_t) and torch.equal(fc, fc_t), "the two routes disagree"
    assert len(iv) > 0 and len(fc) > 0
    print(json.dumps({"n": a.n, "points": len(pts), "tets": len(tets), "tets_dtype": str(lib_tets.dtype), "torch_ms": round(torch_ms, 3),
                      "library_ms": round(lib_ms, 3), "ratio": round(torch_ms / lib_ms, 2), "E": len(iv), "faces": len(fc)}))


if __name__ == "__main__":
    main()
