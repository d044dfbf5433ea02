"""Marching tetrahedra without a GPU: the numpy restatement (tests/mesh_truth.py) against the reference's own outputs
(tests/golden/marching_tets.npz, written by tests/tools/gen_mesh_golden.py), the host-side argument checks of the C entry points, the
Python operator's refusal of CPU tensors, and the mesh PLY writer."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import mesh_truth
from mesh_truth import CASES, GOLDEN


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def test_golden_holds_the_five_cases(golden):
    assert tuple(golden["names"]) == CASES
    assert golden["single_interp_v"].shape == (4, 2) and golden["single_faces"].shape == (2, 3)
    assert golden["outside_interp_v"].shape == (0, 2) and golden["outside_faces"].shape == (0, 3)
    assert np.isnan(golden["dup_nan_zero_sdf"]).sum() == 1 and (golden["dup_nan_zero_sdf"] == 0).sum() == 2
    assert golden["kuhn3_tets"].shape == (48, 4) and golden["kuhn6_tets"].shape == (750, 4)
    assert len(golden["kuhn3_interp_v"]) > 0 and len(golden["kuhn6_faces"]) > 0
    assert os.path.getsize(GOLDEN) < 200 * 1024


@pytest.mark.parametrize("name", CASES)
def test_restatement_equals_the_reference(golden, name):
    sdf, tets, verts, scales = (golden[name + k] for k in ("_sdf", "_tets", "_vertices", "_scales"))
    interp_v, faces, stats = mesh_truth.marching_tets(sdf, tets)
    assert interp_v.dtype == np.int64 and faces.dtype == np.int64
    assert np.array_equal(interp_v, golden[name + "_interp_v"])
    assert np.array_equal(faces, golden[name + "_faces"])
    assert len(faces) == stats["n_one"] + 2 * stats["n_two"]
    # the gathers are plain indexing with interp_v (NaN compares by bits)
    assert np.array_equal(verts[interp_v], golden[name + "_end_points"])
    assert golden[name + "_end_sdf"].shape == (len(interp_v), 2, 1) and golden[name + "_end_scales"].shape == (len(interp_v), 2, 1)
    assert np.array_equal(sdf[interp_v][..., None].view(np.uint32), golden[name + "_end_sdf"].view(np.uint32))
    assert np.array_equal(scales[interp_v], golden[name + "_end_scales"])
    if len(interp_v):
        assert (interp_v[:, 0] < interp_v[:, 1]).all()
        key = interp_v[:, 0] * len(sdf) + interp_v[:, 1]
        assert (np.diff(key) > 0).all()                 # ascending lexicographic, unique
        assert ((sdf[interp_v] > 0).sum(1) == 1).all()  # exactly one occupied end


def test_host_side_abi_errors(f3d):
    from f3dgaus_amd import _lib
    L = _lib.lib()
    buf = (C.c_char * 1024)()
    one = C.cast(buf, C.c_void_p)
    counts = (C.c_longlong * 4)()
    # NULL pointers
    assert L.f3dg_marching_tets_count(None, None, 1 << 30, 10, 5, 20, one, one, 0, counts) == _lib.ERR_BAD_ARG
    assert L.f3dg_marching_tets_count(None, one, 1 << 30, 10, 5, 20, None, one, 0, counts) == _lib.ERR_BAD_ARG
    assert L.f3dg_marching_tets_count(None, one, 1 << 30, 10, 5, 20, one, None, 0, counts) == _lib.ERR_BAD_ARG
    assert L.f3dg_marching_tets_count(None, one, 1 << 30, 10, 5, 20, one, one, 0, None) == _lib.ERR_BAD_ARG
    assert L.f3dg_marching_tets_emit(None, one, 1 << 30, 10, 5, 20, one, 0, 1, None, one) == _lib.ERR_BAD_ARG
    assert L.f3dg_marching_tets_emit(None, one, 1 << 30, 10, 5, 20, one, 0, 1, one, None) == _lib.ERR_BAD_ARG
    # sizes: N <= 0, F < 0, N or F >= 2^31, more capacity than 4 F
    for N, F, cap in ((0, 5, 20), (-3, 5, 20), (10, -1, 0), (1 << 31, 5, 20), (10, 1 << 31, 20), (10, 5, 21), (10, 5, -1)):
        assert L.f3dg_marching_tets_count(None, one, 1 << 30, N, F, cap, one, one, 0, counts) == _lib.ERR_BAD_ARG, (N, F, cap)
        assert L.f3dg_marching_tets_workspace_bytes(N, F, cap) == 0, (N, F, cap)
    # a workspace smaller than asked for is refused before anything runs
    need = L.f3dg_marching_tets_workspace_bytes(10, 5, 20)
    assert need > 0
    assert L.f3dg_marching_tets_count(None, one, need - 1, 10, 5, 20, one, one, 0, counts) == _lib.ERR_WORKSPACE
    assert L.f3dg_marching_tets_emit(None, one, need - 1, 10, 5, 20, one, 0, 1, one, one) == _lib.ERR_WORKSPACE
    # the workspace grows with every size; the mesh path's own size (5.3 M points, 30 M tetrahedra) stays near 1 GB
    a, b, c, d = (L.f3dg_marching_tets_workspace_bytes(*s) for s in ((1000, 5000, 5000), (2000, 5000, 5000), (2000, 9000, 5000), (2000, 9000, 36000)))
    assert 0 < a < b < c < d
    assert d - c >= (36000 - 5000) * 8
    assert L.f3dg_marching_tets_workspace_bytes(5_300_000, 30_000_000, 120_000_000) < 1100 << 20
    # F = 0 is legal, gives zero counts and touches no device
    counts[0] = counts[1] = counts[2] = counts[3] = 7
    assert L.f3dg_marching_tets_count(None, one, 1 << 30, 10, 0, 0, one, None, 0, counts) == _lib.OK
    assert list(counts) == [0, 0, 0, 0]


def test_marching_tetrahedra_raises_on_cpu_tensors(f3d, golden):
    v = torch.from_numpy(golden["single_vertices"])[None]
    t = torch.from_numpy(golden["single_tets"])
    s = torch.from_numpy(golden["single_sdf"])[None]
    sc = torch.from_numpy(golden["single_scales"])[None]
    assert f3d.mesh.marching_tetrahedra is f3d.marching_tetrahedra
    with pytest.raises(RuntimeError, match="HIP device"):
        f3d.mesh.marching_tetrahedra(v, t, s, sc)
    with pytest.raises(RuntimeError, match="HIP device"):
        f3d.mesh.marching_tets_topology(s[0], t)
    with pytest.raises(RuntimeError, match="HIP device"):
        f3d.mesh.tetra_points(torch.eye(4)[None], 0.1, 10.0, 1.0, torch.ones(2, 4), torch.zeros(2, 3), torch.ones(2, 3))


def test_bisect_level_set_rule_on_a_known_field():
    """The ind_low rule of visualize.py:509 with a stand-in sweep (a plane; no device needed): a midpoint sdf of exactly 0 moves the
    RIGHT end, and the inputs are not modified."""
    from f3dgaus_amd import mesh
    # final_alpha = 0.5 - x: sdf(x) = (1 - final_alpha) - 0.5 = x; the level set is x = 0
    sweep = lambda p: 0.5 - p[:, 0]
    ends = torch.tensor([[[-1.0, 0, 0], [1.0, 0, 0]],        # midpoint sdf exactly 0 at step 1
                         [[-1.0, 0, 0], [3.0, 0, 0]],        # 1, 0 (exact zero at step 2)
                         [[0.75, 1, 2], [-0.25, 1, 2]]])     # left end inside
    sdf = ends[:, :, :1].clone()
    before = ends.clone()
    # one step by hand: edge 0: mid 0 -> right moves: [-1, 0] -> 0.5 * (-1 + 0) = -0.5
    out = mesh.bisect_level_set(sweep, ends, sdf, n_steps=1)
    assert torch.equal(ends, before)
    assert out[:, 0].tolist() == [-0.5, 0.0, 0.0]
    out8 = mesh.bisect_level_set(sweep, ends, sdf, n_steps=8)
    # edge 0 keeps halving towards 0 from the left: the left end follows the negative side, the right end stays at 0
    assert out8[0, 0].item() == -(2.0 ** -8) and torch.equal(out8[:, 1:], ends[:, 0, 1:])
    assert out8[:, 0].abs().max().item() <= 4.0 / 2 ** 8
    assert mesh.bisect_level_set(sweep, ends, sdf, n_steps=0)[:, 0].tolist() == [0.0, 1.0, 0.25]


def test_save_mesh_ply_round_trips(f3d, tmp_path):
    rng = np.random.default_rng(3)
    v = rng.normal(size=(7, 3)).astype(np.float32)
    f = rng.integers(0, 7, (5, 3)).astype(np.int64)
    col = rng.integers(0, 256, (7, 3)).astype(np.uint8)
    p = str(tmp_path / "sub" / "mesh.ply")
    f3d.ply.save_mesh_ply(p, torch.from_numpy(v), torch.from_numpy(f))
    head = open(p, "rb").read().split(b"end_header\n")[0].decode().splitlines()
    assert head[:3] == ["ply", "format binary_little_endian 1.0", "element vertex 7"]
    assert head[3:] == ["property float x", "property float y", "property float z", "element face 5", "property list uchar int vertex_indices"]
    assert os.path.getsize(p) == len("\n".join(head)) + 1 + len("end_header\n") + 7 * 12 + 5 * 13
    v2, f2, c2 = f3d.ply.read_mesh_ply(p)
    assert np.array_equal(v2, v) and np.array_equal(f2, f) and f2.dtype == np.int32 and c2 is None
    f3d.ply.save_mesh_ply(p, v, f, vertex_colors=col)
    v3, f3, c3 = f3d.ply.read_mesh_ply(p)
    assert np.array_equal(v3, v) and np.array_equal(f3, f) and np.array_equal(c3, col)
    f3d.ply.save_mesh_ply(p, np.zeros((0, 3)), np.zeros((0, 3), dtype=np.int64))
    v4, f4, _ = f3d.ply.read_mesh_ply(p)
    assert v4.shape == (0, 3) and f4.shape == (0, 3)
    with pytest.raises(AssertionError):
        f3d.ply.save_mesh_ply(p, v, f + 7)
