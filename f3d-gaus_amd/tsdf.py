"""TSDF fusion on the HIP device: the mesh route that needs no external tetrahedralisation.

    vol = TSDFVolume(origin, voxel_size, (nx, ny, nz), device=dev)
    vol.integrate(depth, world_views, cfg['model']['fov'], color=rgb, alpha=alpha)      # all views in one launch
    m = vol.extract()
    ply.save_mesh_ply(path, m["vertices"], m["faces"], (m["vertex_colors"].clamp(0, 1) * 255).round().to(torch.uint8))

The reference meshes through a Delaunay tetrahedralisation built outside of it and holds no TSDF code: the semantics are THIS project's
(include/f3dg.h has the definition, DESIGN.md section 3g-bis the reasons, tests/tsdf_truth.py a float64 restatement). Rendered z-depth maps
are fused into a truncated signed distance volume -- per voxel and view a projective gather, a running weighted mean of
``min(1, (depth - Z) / trunc)`` and of the colour inside the band -- by ``f3dg_tsdf_integrate``; ``f3dg_tsdf_cells_count`` / ``_emit`` turn the
cells the surface passes through into consistently oriented Kuhn tetrahedra, ``mesh.marching_tets_topology`` triangulates them, and
``f3dg_tsdf_vertices`` places the vertices and their colours on the crossing edges. One writer per voxel, a fixed view order, no atomics:
every output is bit-reproducible.

The volume is data: no gradient flows to the depth, the colour or the cameras, and inputs that require grad are refused. Inputs are
float32 on the volume's HIP device (no CPU fallback); everything is enqueued on the current stream."""
import ctypes as C
import math

import torch

from . import _lib
from .diff_gof_rasterization import _stream

__all__ = ["TSDFVolume"]


def _data(t, name, shapes, dev, who):
    """``t`` as a contiguous float32 tensor of one of ``shapes`` on ``dev``; tensors that require grad and host tensors raise."""
    if not torch.is_tensor(t):
        raise TypeError(f"{who}: `{name}` must be a tensor")
    if torch.is_grad_enabled() and t.requires_grad:
        raise NotImplementedError(f"{who} produces no gradient for `{name}`: detach it (the volume is data)")
    if not t.is_cuda or t.device != dev:
        raise RuntimeError(f"f3dgaus_amd.tsdf.{who} needs `{name}` on the volume's HIP device (no CPU fallback)")
    if t.dtype != torch.float32:
        raise TypeError(f"{who}: `{name}` must be float32 (got {t.dtype})")
    if tuple(t.shape) not in shapes:
        raise ValueError(f"{who}: `{name}` is {tuple(t.shape)}; expected one of {shapes}")
    return t.detach().contiguous()


class TSDFVolume:
    """A truncated signed distance volume of ``dims = (nx, ny, nz)`` voxels of edge ``voxel_size``; ``origin`` (three numbers) is the world
    position of the centre of voxel (0, 0, 0). ``trunc`` defaults to four voxels. State, float32 on ``device``, x fastest:
    ``tsdf`` [nz,ny,nx], ``weight`` [nz,ny,nx], ``color`` [3,nz,ny,nx], ``color_weight`` [nz,ny,nx]; all-zero means empty."""

    def __init__(self, origin, voxel_size, dims, trunc=None, device=None):
        dev = torch.device("cuda" if device is None else device)
        if dev.type != "cuda":
            raise RuntimeError("f3dgaus_amd.tsdf.TSDFVolume lives on a HIP device (no CPU fallback)")
        if dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        origin = [float(v) for v in (origin.detach().cpu().reshape(-1).tolist() if torch.is_tensor(origin) else origin)]
        dims = tuple(int(d) for d in dims)
        voxel_size = float(voxel_size)
        trunc = 4.0 * voxel_size if trunc is None else float(trunc)
        if len(origin) != 3 or len(dims) != 3:
            raise ValueError(f"TSDFVolume: `origin` and `dims` hold three numbers each; got {origin}, {dims}")
        if min(dims) < 1 or dims[0] * dims[1] * dims[2] >= 2 ** 31:
            raise ValueError(f"TSDFVolume: dims {dims} must be positive with fewer than 2^31 voxels")
        if not (math.isfinite(voxel_size) and voxel_size > 0 and math.isfinite(trunc) and trunc > 0 and all(math.isfinite(v) for v in origin)):
            raise ValueError(f"TSDFVolume: origin {origin} must be finite, voxel_size {voxel_size} and trunc {trunc} finite and positive")
        self.device, self.dims, self.voxel_size, self.trunc = dev, dims, voxel_size, trunc
        self.origin = tuple(origin)
        self._origin = (C.c_float * 3)(*origin)
        nx, ny, nz = dims
        self.tsdf = torch.zeros((nz, ny, nx), dtype=torch.float32, device=dev)
        self.weight = torch.zeros((nz, ny, nx), dtype=torch.float32, device=dev)
        self.color = torch.zeros((3, nz, ny, nx), dtype=torch.float32, device=dev)
        self.color_weight = torch.zeros((nz, ny, nx), dtype=torch.float32, device=dev)

    def reset(self):
        """Empty the volume."""
        for t in (self.tsdf, self.weight, self.color, self.color_weight):
            t.zero_()
        return self

    def integrate(self, depth, world_views, fov, color=None, alpha=None, alpha_min=0.5, z_near=0.01):
        """Fuse V views into the volume: ``depth`` [V,H,W] or [V,1,H,W] z-depth (plane 6 of the raster), ``world_views`` [V,4,4] (or
        [V,1,4,4]) in the renderer's row-vector convention, ``fov`` the field of view in degrees as ``cfg['model']['fov']`` (fx and fy
        formed as ``render_views`` forms them) or a pair ``(fx, fy)`` in pixels; ``color`` [V,3,H,W] and ``alpha`` [V,H,W] / [V,1,H,W]
        optional. A pixel is used iff its depth is finite and positive and its alpha, when given, reaches ``alpha_min``; a voxel takes
        a sample iff it lies beyond ``z_near`` in the camera, projects into the image and is not more than ``trunc`` behind the depth.
        One launch for up to 128 views; more are chunked, which equals consecutive calls. Accumulates: call it again for further views."""
        who = "TSDFVolume.integrate"
        if not torch.is_tensor(depth) or depth.dim() not in (3, 4):
            raise ValueError(f"{who}: `depth` is [V,H,W] or [V,1,H,W]")
        V, H, W = int(depth.shape[0]), int(depth.shape[-2]), int(depth.shape[-1])
        if V == 0 or H == 0 or W == 0:
            raise ValueError(f"{who}: empty depth {tuple(depth.shape)}")
        dev = self.device
        depth = _data(depth, "depth", ((V, H, W), (V, 1, H, W)), dev, who)
        wv = _data(world_views, "world_views", ((V, 4, 4), (V, 1, 4, 4)), dev, who)
        if color is not None:
            color = _data(color, "color", ((V, 3, H, W),), dev, who)
        if alpha is not None:
            alpha = _data(alpha, "alpha", ((V, H, W), (V, 1, H, W)), dev, who)
        if isinstance(fov, (tuple, list)):
            fx, fy = float(fov[0]), float(fov[1])
        else:
            FoV = float(fov) * math.pi / 180
            fx, fy = W / (2 * math.tan(FoV / 2.)), H / (2 * math.tan(FoV / 2.))
        nx, ny, nz = self.dims
        with torch.cuda.device(dev):
            rc = _lib.lib().f3dg_tsdf_integrate(_stream(), nx, ny, nz, self._origin, self.voxel_size, self.trunc, float(z_near), V, H, W,
                                                _lib.ptr(depth), _lib.ptr(color), _lib.ptr(alpha), float(alpha_min), _lib.ptr(wv), fx, fy,
                                                _lib.ptr(self.tsdf), _lib.ptr(self.weight), _lib.ptr(self.color), _lib.ptr(self.color_weight))
        _lib.check(rc, "f3dg_tsdf_integrate")
        return self

    def surface_tets(self, min_weight=1.0):
        """tets [6 n_active, 4] int32: the six Kuhn tetrahedra (one orientation) of every cell whose eight corners have
        ``weight >= min_weight`` and a finite tsdf that does not have one sign throughout; cells in ascending id. One host read."""
        nx, ny, nz = self.dims
        dev = self.device
        if min(self.dims) < 2:
            raise ValueError(f"TSDFVolume: cells need at least two voxels along every axis (dims {self.dims})")
        L = _lib.lib()
        nbytes = L.f3dg_tsdf_cells_workspace_bytes(nx, ny, nz)
        if nbytes == 0:
            raise _lib.F3dgError(_lib.ERR_BAD_ARG, "f3dg_tsdf_cells_workspace_bytes")
        n_active = C.c_longlong(0)
        with torch.cuda.device(dev):
            ws = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
            _lib.check(L.f3dg_tsdf_cells_count(_stream(), nx, ny, nz, float(min_weight), _lib.ptr(self.tsdf), _lib.ptr(self.weight),
                                               _lib.ptr(ws), nbytes, C.byref(n_active)), "f3dg_tsdf_cells_count")
            n = int(n_active.value)
            tets = torch.empty((6 * n, 4), dtype=torch.int32, device=dev)
            if n > 0:
                _lib.check(L.f3dg_tsdf_cells_emit(_stream(), nx, ny, nz, _lib.ptr(ws), nbytes, n, _lib.ptr(tets)), "f3dg_tsdf_cells_emit")
        return tets

    def extract(self, min_weight=1.0):
        """The zero level set as a triangle mesh: a dict of ``vertices`` [E,3] float32, ``faces`` [F,3] int64, ``vertex_colors`` [E,3]
        float32 (the volume's colour interpolated along the edge; 0 where neither end holds one), ``interp_v`` [E,2] int64 (the voxel
        ids of the edge each vertex lies on) and ``tets`` [6 n_active, 4] int32. Occupied means behind the surface (tsdf < 0);
        ``tsdf == 0`` is free. An empty or unobserved volume gives an empty mesh."""
        from .mesh import marching_tets_topology
        nx, ny, nz = self.dims
        dev = self.device
        tets = self.surface_tets(min_weight)
        interp_v, faces = marching_tets_topology(-self.tsdf.reshape(-1), tets)
        E = int(interp_v.shape[0])
        vertices = torch.empty((E, 3), dtype=torch.float32, device=dev)
        colors = torch.empty((E, 3), dtype=torch.float32, device=dev)
        if E > 0:
            with torch.cuda.device(dev):
                rc = _lib.lib().f3dg_tsdf_vertices(_stream(), nx, ny, nz, self._origin, self.voxel_size, E, _lib.ptr(interp_v),
                                                   _lib.ptr(self.tsdf), _lib.ptr(self.color), _lib.ptr(self.color_weight),
                                                   _lib.ptr(vertices), _lib.ptr(colors))
            _lib.check(rc, "f3dg_tsdf_vertices")
        return {"vertices": vertices, "faces": faces, "vertex_colors": colors, "interp_v": interp_v, "tets": tets}
