"""Generates tests/golden/marching_tets.npz from the reference's OWN marching tetrahedra, in the build container (the reference does
not travel): src/utils_tetmesh.py is imported from where it lies, by path, and ``marching_tetrahedra`` runs as is on CPU torch.
The fixture holds, per case, the four inputs and the four outputs (the pair of gathered endpoint tensors counts as two arrays).

Cases: 1 the docstring's single tetrahedron; 2 one tetrahedron entirely outside (empty outputs); 3 duplicate tetrahedra with a NaN and
zeros in the sdf; 4, 5 the 3^3 and 6^3 Kuhn grids with a noisy-sphere sdf, tetrahedron rows and in-row corners permuted."""
import importlib.util
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
REF = "/root/reference"
sys.path.insert(0, os.path.join(ROOT, "tests"))
import mesh_truth  # noqa: E402


def cases():
    unit = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], dtype=np.float32)
    yield "single", unit, np.array([[0, 1, 2, 3]]), np.array([-1, -1, .5, .5], dtype=np.float32)
    yield "outside", unit, np.array([[0, 1, 2, 3]]), np.array([-1, -2, -.5, -3], dtype=np.float32)
    five = np.concatenate([unit, [[1, 1, 1]]]).astype(np.float32)
    yield "dup_nan_zero", five, np.array([[0, 1, 2, 3], [3, 2, 1, 0], [0, 1, 2, 3]]), np.array([-1, 1, np.nan, 0, 0], dtype=np.float32)
    for name, n, seed in (("kuhn3", 3, 11), ("kuhn6", 6, 12)):
        pts, tets = mesh_truth.kuhn_grid(n)
        yield name, pts, mesh_truth.permuted(tets, seed), mesh_truth.noisy_sphere_sdf(pts, seed + 100)


def main():
    spec = importlib.util.spec_from_file_location("ref_utils_tetmesh", os.path.join(REF, "src", "utils_tetmesh.py"))
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    out = {}
    names = []
    for name, pts, tets, sdf in cases():
        rng = np.random.default_rng(len(pts))
        scales = rng.random((len(pts), 1)).astype(np.float32)
        verts_list, scale_list, faces_list, interp_list = ref.marching_tetrahedra(
            torch.from_numpy(pts)[None], torch.from_numpy(np.asarray(tets, dtype=np.int64)), torch.from_numpy(sdf)[None], torch.from_numpy(scales)[None])
        (end_points, end_sdf), end_scales, faces, interp_v = verts_list[0], scale_list[0], faces_list[0], interp_list[0]
        names.append(name)
        out.update({name + "_vertices": pts, name + "_tets": np.asarray(tets, dtype=np.int64), name + "_sdf": sdf, name + "_scales": scales,
                    name + "_end_points": end_points.numpy().reshape(-1, 2, 3), name + "_end_sdf": end_sdf.numpy().reshape(-1, 2, 1),
                    name + "_end_scales": end_scales.numpy().reshape(-1, 2, 1), name + "_faces": faces.numpy().reshape(-1, 3),
                    name + "_interp_v": interp_v.numpy().reshape(-1, 2)})
        _, _, st = mesh_truth.marching_tets(sdf, tets)
        print(name, "points", len(pts), "tets", len(tets), "surface", st["surface"], "E", len(out[name + "_interp_v"]), "faces", len(out[name + "_faces"]))
    path = os.path.join(ROOT, "tests", "golden", "marching_tets.npz")
    np.savez_compressed(path, names=np.array(names), **out)
    print(path, os.path.getsize(path))


if __name__ == "__main__":
    main()
