"""extract_mesh (visualize.py:447-546) against the reference-shaped loop written out here, and tetra_points (:120-144) by properties.

The scene: 300 opaque Gaussians in a ball of radius 0.3 at 64^2 under 3 cameras; the points are a 9^3 Kuhn grid (729 points, 3,072
tetrahedra) of side 1.2 around it with a constant scale. The ball was chosen on the CPU with ``oracle_integrate`` (min over the three
cameras): its alpha-0.5 surface crosses 742 grid edges there; the test asserts at least 100 on the device."""
import numpy as np
import pytest
import torch

import mesh_truth
from helpers import make_scene

pytestmark = pytest.mark.gpu

CENTRE = (0.0, 0.0, 7.667)


def _scene():
    P = 300
    scene = make_scene(P=P, res=(64, 64), s0=0.08, seed=0, view=[0, 1, 3])
    g = torch.Generator().manual_seed(1)
    d = torch.randn(P, 3, generator=g)
    d = d / d.norm(dim=1, keepdim=True) * torch.rand(P, 1, generator=g) ** (1 / 3) * 0.3
    scene["means3D"] = (d + torch.tensor(CENTRE)).float().contiguous()
    scene["opacities"] = torch.full((P, 1), 0.99)
    return scene


@pytest.fixture(scope="module")
def setup(f3d, gpu_device):
    from f3dgaus_amd import cameras
    dev = gpu_device
    scene = _scene()
    d = lambda t: t.to(dev)
    cfg = cameras.default_cfg(resolution=64)
    cfg["model"]["max_sh_degree"] = scene["sh_degree"]
    assert abs(np.tan(cfg["model"]["fov"] * np.pi / 360) - scene["tanfovx"]) < 1e-12
    pc = {"xyz": d(scene["means3D"])[None], "opacity": d(scene["opacities"])[None], "scaling": d(scene["scales"])[None],
          "rotation": d(scene["rotations"])[None], "features_dc": d(scene["shs"])[None, :, :1], "features_rest": d(scene["shs"])[None, :, 1:]}
    pts, tets = mesh_truth.kuhn_grid(9)
    pts = ((pts - 0.5) * 1.2 + np.array(CENTRE, dtype=np.float32)).astype(np.float32)
    cams = (d(scene["viewmatrix"]), d(scene["projmatrix"]), d(scene["campos"]), d(scene["bg"]))
    return dict(scene=scene, cfg=cfg, pc=pc, points=torch.from_numpy(pts).to(dev), cells=torch.from_numpy(tets).to(dev),
                points_scale=torch.full((len(pts), 1), 0.04, device=dev), cams=cams, tets=tets)


def _reference_loop(f3d, s, n_steps):
    """visualize.py:447-546 as written there: one integrate call per camera with torch.min, marching tetrahedra (the restatement, on
    the host), the bisection with boolean-mask assignments, the filter."""
    wv, fp, cc, bg = s["cams"]
    pc, cfg, points = s["pc"], s["cfg"], s["points"]

    def final_alpha_of(p):
        final_alpha = torch.ones((p.shape[0]), dtype=torch.float32, device=p.device)
        for th in range(wv.shape[0]):
            out = f3d.render_predicted_more_v2_gof_in(p, pc, 0, wv[th:th + 1].contiguous(), fp[th:th + 1].contiguous(),
                                                      cc[th:th + 1].contiguous(), bg, cfg)
            final_alpha = torch.min(final_alpha, out["alpha_integrated"])
        return final_alpha

    alpha = 1 - final_alpha_of(points)
    sdf = alpha - 0.5
    interp_v, faces, _ = mesh_truth.marching_tets(sdf.cpu().numpy(), s["tets"])
    iv = torch.from_numpy(interp_v).to(points.device)
    end_points = points[iv.reshape(-1)].reshape(-1, 2, 3)
    end_sdf = sdf[iv.reshape(-1)].reshape(-1, 2, 1)
    end_scales = s["points_scale"][iv.reshape(-1)].reshape(-1, 2, 1)
    pts = (end_points[:, 0, :] + end_points[:, 1, :]) / 2.
    left_points, right_points = end_points[:, 0, :], end_points[:, 1, :]
    left_sdf, right_sdf = end_sdf[:, 0, :], end_sdf[:, 1, :]
    left_scale, right_scale = end_scales[:, 0, 0], end_scales[:, 1, 0]
    distance = torch.norm(left_points - right_points, dim=-1)
    scale = left_scale + right_scale
    for _ in range(n_steps):
        mid_points = (left_points + right_points) / 2
        alpha = 1 - final_alpha_of(pts.contiguous())
        mid_sdf = (alpha - 0.5)[None].squeeze().unsqueeze(-1)
        ind_low = ((mid_sdf < 0) & (left_sdf < 0)) | ((mid_sdf > 0) & (left_sdf > 0))
        left_sdf[ind_low] = mid_sdf[ind_low]
        right_sdf[~ind_low] = mid_sdf[~ind_low]
        left_points[ind_low.flatten()] = mid_points[ind_low.flatten()]
        right_points[~ind_low.flatten()] = mid_points[~ind_low.flatten()]
        pts = (left_points + right_points) / 2
    mask = (distance <= 3 * scale).cpu().numpy()
    face_mask = mask[faces].all(axis=1)
    inverse = np.zeros(len(mask), dtype=np.int64)
    inverse[mask] = np.arange(mask.sum())
    return dict(interp_v=interp_v, vertices=pts, faces=faces, keep=mask, vertices_filtered=pts[torch.from_numpy(mask).to(pts.device)],
                faces_filtered=inverse[faces[face_mask]], sdf=sdf)


@pytest.fixture(scope="module")
def reference(f3d, setup):
    return _reference_loop(f3d, setup, 8)


def _assert_same(mesh, ref):
    assert torch.equal(mesh["faces"].cpu(), torch.from_numpy(ref["faces"]))
    assert torch.equal(mesh["keep"].cpu(), torch.from_numpy(ref["keep"]))
    assert mesh["vertices"].shape == ref["vertices"].shape == (len(ref["interp_v"]), 3)
    assert torch.equal(mesh["vertices"].view(torch.int32), ref["vertices"].contiguous().view(torch.int32))
    assert torch.equal(mesh["faces_filtered"].cpu(), torch.from_numpy(ref["faces_filtered"]))
    assert torch.equal(mesh["vertices_filtered"].contiguous().view(torch.int32), ref["vertices_filtered"].contiguous().view(torch.int32))


def test_extract_mesh_equals_the_reference_loop(f3d, setup, reference):
    s, ref = setup, reference
    E = len(ref["interp_v"])
    assert E >= 100 and len(ref["faces"]) > 0
    # the surface crosses at least 100 grid edges, counted on the device
    sdf = ref["sdf"]
    edges = torch.cat([s["cells"][:, [a, b]] for a, b in ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3))])
    crossing = edges[(sdf[edges[:, 0]] > 0) != (sdf[edges[:, 1]] > 0)]
    assert len(torch.unique(torch.sort(crossing, dim=1)[0], dim=0)) == E
    # the filter keeps some vertices and drops others (0.04 + 0.04 against edges of 0.15 .. 0.26)
    assert 0 < ref["keep"].sum() < E
    wv, fp, cc, bg = s["cams"]
    mesh = f3d.mesh.extract_mesh(s["pc"], 0, s["points"], s["points_scale"], s["cells"], wv, fp, cc, bg, s["cfg"])
    _assert_same(mesh, ref)
    assert mesh["faces_filtered"].numel() == 0 or int(mesh["faces_filtered"].max()) < len(mesh["vertices_filtered"])
    # the same with a sweep that is handed in, and with int32 cells
    sweep = f3d.AlphaSweep(s["pc"], 0, wv, fp, cc, bg, s["cfg"], max_points=max(E, len(s["points"])))
    mesh2 = f3d.mesh.extract_mesh(s["pc"], 0, s["points"], s["points_scale"], s["cells"].int(), wv, fp, cc, bg, s["cfg"], sweep=sweep)
    _assert_same(mesh2, ref)


def test_extract_mesh_fewer_steps_and_ply(f3d, setup, tmp_path):
    s = setup
    wv, fp, cc, bg = s["cams"]
    ref = _reference_loop(f3d, s, 2)
    mesh = f3d.mesh.extract_mesh(s["pc"], 0, s["points"], s["points_scale"], s["cells"], wv, fp, cc, bg, s["cfg"], n_binary_steps=2)
    _assert_same(mesh, ref)
    # every bisected vertex lies on its edge, between the two grid points
    iv = torch.from_numpy(ref["interp_v"]).to(s["points"].device)
    a, b = s["points"][iv[:, 0]], s["points"][iv[:, 1]]
    assert ((mesh["vertices"] >= torch.minimum(a, b)) & (mesh["vertices"] <= torch.maximum(a, b))).all()
    p = str(tmp_path / "mesh_binary_search.ply")
    f3d.ply.save_mesh_ply(p, mesh["vertices_filtered"], mesh["faces_filtered"])
    v, f, _ = f3d.ply.read_mesh_ply(p)
    assert np.array_equal(v, mesh["vertices_filtered"].cpu().numpy()) and np.array_equal(f, mesh["faces_filtered"].cpu().numpy())


def test_tetra_points_properties(f3d, gpu_device):
    """Nine points per Gaussian before masking: the eight corners xyz + R (+-3 s) in binary counting order (x slowest), then the
    centres; the scale column is the largest axis of 3 s; the frustum mask equals a float64 restatement wherever the float64 margin to
    a bound exceeds 1e-3 px (at most 1 % of the points may be that close).

    Corner tolerance: a coordinate is xyz + a sum of three products of rotation entries (each <= 1, built from a normalised
    quaternion by ~8 float32 roundings) with 3 s; 32 units of 2^-24 of the magnitude |xyz| + 3 sqrt(3) max(s) cover those roundings and
    the four of the product sum."""
    dev = gpu_device
    scene = make_scene(P=500, res=(64, 64), s0=0.05, seed=3, view=[0, 2, 5])
    xyz, scale, rot = scene["means3D"].to(dev), scene["scales"].to(dev), (scene["rotations"] * 1.7).to(dev)
    wv = scene["viewmatrix"].to(dev)
    near, far, fov = 7.0, 8.4, 0.1                  # fov as the reference reads it (radians): focal 2,559 px at 256^2
    pts, pts_scale, all_pts, all_scale, mask = f3d.mesh.tetra_points(wv, near, far, fov, rot, xyz, scale, return_unmasked=True)
    P = xyz.shape[0]
    assert all_pts.shape == (9 * P, 3) and all_scale.shape == (9 * P, 1) and mask.shape == (9 * P,) and mask.dtype == torch.bool
    assert torch.equal(pts, all_pts[mask]) and torch.equal(pts_scale, all_scale[mask])
    plain = f3d.mesh.tetra_points(wv, near, far, fov, rot, xyz, scale)
    assert torch.equal(plain[0], pts) and torch.equal(plain[1], pts_scale)
    assert torch.equal(all_pts[8 * P:], xyz)
    # scale column: the largest axis of 3 s (sqrt(s^2) is s in IEEE arithmetic), repeated for the eight corners
    smax = (scale * 3.0).max(dim=-1, keepdim=True)[0]
    assert torch.equal(all_scale[8 * P:], smax) and torch.equal(all_scale[:8 * P].reshape(P, 8), smax.expand(-1, 8))
    # corners, float64
    q = rot.double().cpu().numpy()
    q = q / np.linalg.norm(q, axis=1, keepdims=True)
    w, x, y, z = q.T
    R = np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
                  2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                  2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], 1).reshape(P, 3, 3)
    s3 = 3.0 * scale.double().cpu().numpy()
    signs = np.array([[1.0 if (k >> (2 - a)) & 1 else -1.0 for a in range(3)] for k in range(8)])        # [8,3], x slowest
    assert len({tuple(r) for r in signs}) == 8
    want = xyz.double().cpu().numpy()[:, None, :] + np.einsum("pij,pkj->pki", R, signs[None] * s3[:, None, :])
    got = all_pts[:8 * P].reshape(P, 8, 3).double().cpu().numpy()
    tol = 32 * 2.0 ** -24 * (np.abs(xyz.cpu().numpy()).max() + 3 * np.sqrt(3) * float(scale.max()))
    assert np.abs(got - want).max() <= tol, (np.abs(got - want).max(), tol)
    # frustum mask, float64
    p64 = all_pts.double().cpu().numpy()
    H = W = 256
    focal = 256 / (2 * np.tan(fov / 2))
    inside = np.zeros(len(p64), dtype=bool)
    close = np.zeros(len(p64), dtype=bool)
    for V in wv.double().cpu().numpy():
        cam = np.concatenate([p64, np.ones((len(p64), 1))], 1) @ V          # rows of the transposed view matrix
        depth = cam[:, 2]
        u, v = focal * cam[:, 0] / depth + W / 2, focal * cam[:, 1] / depth + H / 2
        inside |= (depth >= near) & (depth <= far) & (u >= 0) & (u <= W - 1) & (v >= 0) & (v <= H - 1)
        margin_px = np.minimum.reduce([np.abs(u), np.abs(u - (W - 1)), np.abs(v), np.abs(v - (H - 1))])
        # depth bounds: the float32 depth is a four-term dot product of numbers below 16 (2^-20 per rounding at most: < 1e-5 in all);
        # a point nearer than 1e-4 to near / far is skipped like one within 1e-3 px of the image border
        margin_depth = np.minimum(np.abs(depth - near), np.abs(depth - far))
        close |= (margin_px <= 1e-3) | (margin_depth <= 1e-4)
    assert close.mean() <= 0.01
    m = mask.cpu().numpy()
    assert np.array_equal(m[~close], inside[~close])
    assert 0.05 < m.mean() < 0.95               # the bounds cut through the cloud: both outcomes are tested
