"""Times the mesh clean-up, ``mesh.clean_mesh(keep_largest=1)``, on the two meshes a user of the TSDF route would clean: the 256^3 TSDF mesh of
the real image's orbit (tests/real_data.py through ``mesh.extract_mesh_tsdf``, the volume of tools/bench_tsdf.py) and a synthetic two-sphere
mesh at 256^3 (a body and a floater, tests/test_mesh_clean_gpu.py's case scaled up). The comparator is a torch route of the same definition
in the same process: min-label propagation with ``scatter_reduce_('amin')`` over the face-vertex pairs until nothing changes, then the
mask / cumsum compaction ``mesh.extract_mesh`` uses. Both routes alternate in one process after a warm-up call each; device events around
whole calls (both hold host reads, so the host clock is reported as well); the median of the rounds. Also reports the stages of the HIP
route through the C ABI, the rounds the library needed, and the components the meshes actually have. Prints ONE JSON line.

    python tools/bench_mesh_clean.py [--rounds 7] [--res 256] [--views 128] [--image 256] [--skip-real]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import f3dgaus_amd  # noqa: E402,F401
from f3dgaus_amd import _lib, mesh, synthetic, tsdf  # noqa: E402


def torch_clean_largest(vertices, faces):
    """The definition in torch: (vertices, faces, vertex_ids, sweeps) of the largest component (the least root among equals)."""
    N = vertices.shape[0]
    deg = (faces[:, 0] == faces[:, 1]) | (faces[:, 1] == faces[:, 2]) | (faces[:, 0] == faces[:, 2])
    f = faces[~deg]
    flat = f.reshape(-1)
    label = torch.arange(N, device=faces.device)
    sweeps = 0
    while True:
        m = label[f].amin(dim=1)
        new = label.clone()
        new.scatter_reduce_(0, flat, m[:, None].expand(-1, 3).reshape(-1), "amin")
        sweeps += 1
        if torch.equal(new, label):
            break
        label = new
    face_label = label[f[:, 0]]
    sizes = torch.bincount(face_label, minlength=N)
    kept = f[face_label == torch.argmax(sizes)]
    used = torch.zeros(N, dtype=torch.bool, device=faces.device)
    used[kept.reshape(-1)] = True
    new_index = torch.cumsum(used.to(torch.int64), 0) - 1
    return vertices[used], new_index[kept], torch.nonzero(used).reshape(-1), sweeps


def timed(fn):
    """(device ms between two events, host ms) around a call that ends in a synchronise."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), (time.perf_counter() - t0) * 1e3, out


def stages(vertices, faces, rounds):
    """Host-clock medians of the HIP route's parts (each ends in its own host read or a synchronise)."""
    L = _lib.lib()
    N, F, dev = vertices.shape[0], faces.shape[0], faces.device
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    nb_c, nb_m = L.f3dg_mesh_components_workspace_bytes(N, F), L.f3dg_mesh_compact_workspace_bytes(N, F)
    ws_c, ws_m = torch.empty(nb_c, dtype=torch.uint8, device=dev), torch.empty(nb_m, dtype=torch.uint8, device=dev)
    fc, cf = torch.empty(F, dtype=torch.int32, device=dev), torch.empty(N, dtype=torch.int32, device=dev)
    h4, h2 = (C.c_longlong * 4)(), (C.c_longlong * 2)()
    t = {"components_ms": [], "ranking_glue_ms": [], "compact_count_ms": [], "compact_emit_ms": [], "gather_ms": []}

    def clock(key, fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        t[key].append((time.perf_counter() - t0) * 1e3)
        return out
    for _ in range(rounds):
        _lib.check(clock("components_ms", lambda: L.f3dg_mesh_components(stream, _lib.ptr(ws_c), nb_c, N, F, _lib.ptr(faces), 0, _lib.ptr(fc), _lib.ptr(cf), h4)), "components")
        roots, sizes, _, _ = clock("ranking_glue_ms", lambda: mesh._rank_components(fc, cf))
        keep = torch.zeros(N, dtype=torch.uint8, device=dev)
        keep[roots[:1]] = 1
        _lib.check(clock("compact_count_ms", lambda: L.f3dg_mesh_compact_count(stream, _lib.ptr(ws_m), nb_m, N, F, _lib.ptr(faces), 0, _lib.ptr(fc), _lib.ptr(keep), h2)), "count")
        out, ids = torch.empty((h2[0], 3), dtype=torch.int64, device=dev), torch.empty(h2[1], dtype=torch.int64, device=dev)
        _lib.check(clock("compact_emit_ms", lambda: L.f3dg_mesh_compact_emit(stream, _lib.ptr(ws_m), nb_m, N, F, _lib.ptr(faces), 0, _lib.ptr(fc), _lib.ptr(keep),
                                                                             h2[0], h2[1], _lib.ptr(out), _lib.ptr(ids))), "emit")
        clock("gather_ms", lambda: vertices[ids])
    return {k: round(statistics.median(v), 4) for k, v in t.items()}


def measure(name, vertices, faces, rounds):
    N, F = vertices.shape[0], faces.shape[0]
    mc = mesh.mesh_components(faces, N)
    sizes = mc["component_sizes"].tolist()
    hip = lambda: mesh.clean_mesh(vertices, faces, keep_largest=1)
    ref = lambda: torch_clean_largest(vertices, faces)
    a, (bv, bf, bids, sweeps) = hip(), ref()                    # warm-up, and the two routes give one mesh
    same = torch.equal(a["faces"], bf) and torch.equal(a["vertex_ids"], bids) and torch.equal(a["vertices"], bv)
    again = hip()
    repeatable = all(torch.equal(a[k], again[k]) for k in ("vertices", "faces", "vertex_ids"))
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
                     "hip_host_ms": round(statistics.median(hh), 4), "torch_ms": round(statistics.median(tt), 3), "torch_min_ms": round(min(tt), 3),
                     "torch_host_ms": round(statistics.median(ht), 3), "torch_over_hip": round(statistics.median(tt) / statistics.median(th), 2)})
    return {"mesh": name, "vertices": N, "faces": F, "components": len(sizes), "largest_sizes": sizes[:8], "faces_outside_largest": F - (sizes[0] if sizes else 0),
            "components_under_100_faces": sum(1 for s in sizes if s < 100), "degenerate_faces": mc["n_degenerate"], "rounds_used": mc["rounds"],
            "torch_sweeps": sweeps, "kept_faces": int(a["faces"].shape[0]), "kept_vertices": int(a["vertex_ids"].shape[0]), "routes_agree": same,
            "hip_bitwise_repeatable": repeatable, "runs": runs, "hip_faster": all(r["hip_ms"] < r["torch_ms"] for r in runs),
            "stages_host_ms": stages(vertices, faces, max(3, rounds))}


def two_spheres(n, dev):
    """The test's two-sphere volume at n^3: a body of radius 14/48 n voxels and a floater of radius 3/48 n voxels, 7/48 n voxels apart."""
    s = n / 48.0
    vol = tsdf.TSDFVolume((-0.5 * (n - 1) + 0.137, -0.5 * (n - 1) - 0.071, -0.5 * (n - 1) + 0.043), 1.0, (n, n, n), device=dev)
    ax = lambda k: vol.origin[k] + torch.arange(n, device=dev, dtype=torch.float32)
    z, y, x = torch.meshgrid(ax(2), ax(1), ax(0), indexing="ij")
    dist = lambda c, r: (torch.sqrt((x - c[0] * s) ** 2 + (y - c[1] * s) ** 2 + (z - c[2] * s) ** 2) - r * s) / vol.trunc
    vol.tsdf.copy_(torch.minimum(dist((-6.0, 0.5, -0.25), 14.0), dist((18.0, 1.0, 0.5), 3.0)).clamp(-1, 1))
    vol.weight.fill_(1.0)
    return vol.extract()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--res", type=int, default=256)
    ap.add_argument("--views", type=int, default=128)
    ap.add_argument("--image", type=int, default=256)
    ap.add_argument("--skip-real", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_mesh_clean needs a HIP device: a time measured anywhere else says nothing")
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
    print(json.dumps({"tool": "bench_mesh_clean", "device": torch.cuda.get_device_name(0), "rounds": args.rounds, "results": results,
                      "note": "hip = mesh.clean_mesh(keep_largest=1), torch = min-label propagation + mask / cumsum compaction; *_ms: device events around "
                              "whole calls, *_host_ms: host clock around the same calls (both routes hold host reads); medians; two runs of the alternation"}))


if __name__ == "__main__":
    main()
