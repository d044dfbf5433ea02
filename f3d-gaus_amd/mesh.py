"""Mesh extraction (the reference's scripts/test_mesh.sh route, visualize.py:440-548): everything between the opacity sweeps.

    points, points_scale = tetra_points(world_views, near, far, fov, rotation, xyz, scale)      # visualize.py:120-144
    cells = ...                                   # any [F,4] tetrahedralisation of `points` (the reference: CGAL, on the host)
    mesh = extract_mesh(pc, bs, points, points_scale, cells, world_views, full_projs, camera_centers, bg, cfg)
    ply.save_mesh_ply(path, mesh["vertices_filtered"], mesh["faces_filtered"])

``marching_tetrahedra`` has the signature and return structure of src/utils_tetmesh.py:141-190. Its integer topology (which edges cross
the level set, their order, the triangles) is the HIP library's (f3dg_marching_tets_count / _emit, csrc/f3dg_mesh.hip); the three
gathers are plain torch indexing, so the result stays differentiable in ``vertices`` and ``sdf`` exactly as in the reference.

``extract_mesh_tsdf`` is the route that needs no ``cells`` from outside: the orbit's rendered depth fused into a TSDF volume
(``f3dgaus_amd.tsdf``) whose surface cells the library itself turns into tetrahedra. Its semantics are this project's, not the reference's.
No CPU fallback: tensors that are not on a HIP device raise."""
import ctypes as C
import math

import torch

from . import _lib
from .diff_gof_rasterization import _stream

# largest workspace that is sized for the worst case (four crossing edges per tetrahedron, 32 B each) without looking at the data
_WORST_CASE_BYTES = 4 << 30


def _require_hip(*tensors):
    for t in tensors:
        if not torch.is_tensor(t) or not t.is_cuda:
            raise RuntimeError("f3dgaus_amd.mesh needs tensors on a HIP device (no CPU fallback)")


def marching_tets_topology(sdf, tets, max_edges=None):
    """sdf [N] float32, tets [F,4] int64 (or int32), both on one HIP device -> (interp_v [E,2] int64, faces [n1 + 2 n2, 3] int64).

    interp_v: the unique edges with exactly one occupied end (sdf > 0; NaN and 0 are outside) as (lo, hi), lo < hi, in ascending
    lexicographic order. faces: rows of interp_v; first the triangles of the one-triangle surface tetrahedra in tetrahedron order, then
    the two triangles of every two-triangle tetrahedron in tetrahedron order. That is _unbatched_marching_tetrahedra's output for up to
    32 Mi tetrahedra; above that the reference recurses over chunks and returns ANOTHER PERMUTATION of the same faces, while this
    function always works in one piece and keeps the unchunked order. Two blocking host reads (the counts, then E). A tetrahedron with
    an id outside [0, N) raises (the kernel checks every id before it indexes anything). ``max_edges``: workspace capacity for the
    crossing edges, duplicates included; default 4 F (always enough) while that workspace stays under 4 GiB, F beyond (the call is
    repeated with the exact count if that is too small)."""
    _require_hip(sdf, tets)
    if sdf.dim() != 1 or sdf.dtype != torch.float32:
        raise ValueError(f"sdf must be [N] float32, got {tuple(sdf.shape)} {sdf.dtype}")
    if tets.dim() != 2 or tets.shape[1] != 4 or tets.dtype not in (torch.int64, torch.int32):
        raise ValueError(f"tets must be [F,4] int64 or int32, got {tuple(tets.shape)} {tets.dtype}")
    if tets.device != sdf.device:
        raise ValueError("sdf and tets must be on the same device")
    N, F = int(sdf.shape[0]), int(tets.shape[0])
    dev = sdf.device
    if F == 0:
        if N <= 0:
            raise ValueError("sdf is empty")
        return torch.empty((0, 2), dtype=torch.int64, device=dev), torch.empty((0, 3), dtype=torch.int64, device=dev)
    sdf, tets = sdf.detach().contiguous(), tets.contiguous()
    L = _lib.lib()
    is32 = int(tets.dtype == torch.int32)
    cap = int(max_edges) if max_edges is not None else (4 * F if 32 * 4 * F <= _WORST_CASE_BYTES else F)
    cap = max(0, min(cap, 4 * F))
    counts = (C.c_longlong * 4)()
    with torch.cuda.device(dev):
        while True:
            nbytes = L.f3dg_marching_tets_workspace_bytes(N, F, cap)
            if nbytes == 0:
                raise _lib.F3dgError(_lib.ERR_BAD_ARG, "f3dg_marching_tets_workspace_bytes")
            ws = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
            rc = L.f3dg_marching_tets_count(_stream(), _lib.ptr(ws), nbytes, N, F, cap, _lib.ptr(sdf), _lib.ptr(tets), is32, counts)
            if rc == _lib.ERR_OVERFLOW and counts[3] > cap:
                cap = int(counts[3])
                continue
            _lib.check(rc, "f3dg_marching_tets_count")
            break
        E, n_one, n_two = int(counts[0]), int(counts[1]), int(counts[2])
        interp_v = torch.empty((E, 2), dtype=torch.int64, device=dev)
        faces = torch.empty((n_one + 2 * n_two, 3), dtype=torch.int64, device=dev)
        if E > 0:
            _lib.check(L.f3dg_marching_tets_emit(_stream(), _lib.ptr(ws), nbytes, N, F, cap, _lib.ptr(tets), is32, n_one,
                                                 _lib.ptr(interp_v), _lib.ptr(faces)), "f3dg_marching_tets_emit")
    return interp_v, faces


def marching_tetrahedra(vertices, tets, sdf, scales):
    """``marching_tetrahedra`` of src/utils_tetmesh.py:141-190 (the docstring there is stale: this adapted version returns endpoint
    PAIRS, not interpolated vertices). vertices [B,N,3], tets [F,4], sdf [B,N], scales [B,N,1] ->
    ``(verts_list, scale_list, faces_list, interp_list)``, one entry per batch item:
        verts_list[b]  = (vertices[b][interp_v] [E,2,3], sdf[b][interp_v][..., None] [E,2,1])
        scale_list[b]  = scales[b][interp_v] [E,2,1]
        faces_list[b]  [n1 + 2 n2, 3] int64, interp_list[b] = interp_v [E,2] int64
    Order of interp_v and of the faces: see ``marching_tets_topology`` (the reference's, unchunked)."""
    _require_hip(vertices, tets, sdf, scales)
    if vertices.dim() != 3 or vertices.shape[-1] != 3:
        raise ValueError(f"vertices must be [B,N,3], got {tuple(vertices.shape)}")
    B, N = vertices.shape[:2]
    if tuple(sdf.shape) != (B, N):
        raise ValueError(f"sdf must be [B,N] = {(B, N)}, got {tuple(sdf.shape)}")
    if scales.dim() != 3 or tuple(scales.shape[:2]) != (B, N):
        raise ValueError(f"scales must be [B,N,1], got {tuple(scales.shape)}")
    if sdf.dtype != torch.float32:
        raise ValueError(f"sdf must be float32, got {sdf.dtype}")
    outs = []
    for b in range(B):
        interp_v, faces = marching_tets_topology(sdf[b], tets)
        flat = interp_v.reshape(-1)
        edges_to_interp = vertices[b][flat].reshape(-1, 2, 3)
        edges_to_interp_sdf = sdf[b][flat].reshape(-1, 2, 1)
        verts_scales = scales[b][flat].reshape(-1, 2, 1)
        outs.append(((edges_to_interp, edges_to_interp_sdf), verts_scales, faces, interp_v))
    return list(zip(*outs))


def _faces_arg(faces, who):
    _require_hip(faces)
    if faces.dim() != 2 or faces.shape[1] != 3 or faces.dtype not in (torch.int64, torch.int32):
        raise ValueError(f"{who}: faces must be [F,3] int64 or int32, got {tuple(faces.shape)} {faces.dtype}")
    return faces.contiguous()


def _components_raw(faces, N):
    """f3dg_mesh_components: (face_component [F] int32 root ids or -1, component_faces [N] int32, (C, largest, degenerate, rounds))."""
    F, dev = int(faces.shape[0]), faces.device
    if N <= 0:
        raise ValueError(f"mesh components: the mesh needs at least one vertex (got {N})")
    L = _lib.lib()
    nbytes = L.f3dg_mesh_components_workspace_bytes(N, F)
    if nbytes == 0:
        raise _lib.F3dgError(_lib.ERR_UNSUPPORTED, "f3dg_mesh_components_workspace_bytes")
    counts = (C.c_longlong * 4)()
    with torch.cuda.device(dev):
        ws = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
        face_root = torch.empty((F,), dtype=torch.int32, device=dev)
        root_faces = torch.empty((N,), dtype=torch.int32, device=dev)
        _lib.check(L.f3dg_mesh_components(_stream(), _lib.ptr(ws), nbytes, N, F, _lib.ptr(faces), int(faces.dtype == torch.int32),
                                          _lib.ptr(face_root), _lib.ptr(root_faces), counts), "f3dg_mesh_components")
    return face_root, root_faces, tuple(int(c) for c in counts)


def _rank_components(face_root, root_faces):
    """The dense ranking, torch glue over the C roots: (roots [C], sizes [C], rank_of_root [N] (-1 where no root), face_component [F])."""
    roots = torch.nonzero(root_faces > 0).reshape(-1)                           # ascending
    sizes, order = torch.sort(root_faces[roots].to(torch.int64), descending=True, stable=True)       # equal sizes keep the roots' order
    roots = roots[order]
    rank = torch.full((root_faces.shape[0],), -1, dtype=torch.int64, device=root_faces.device)
    rank[roots] = torch.arange(roots.shape[0], dtype=torch.int64, device=roots.device)
    fr = face_root.to(torch.int64)
    face_component = torch.where(fr >= 0, rank[fr.clamp(min=0)], fr)
    return roots, sizes, rank, face_component


@torch.no_grad()
def mesh_components(faces, n_vertices):
    """The connected components of the mesh ``faces`` [F,3] (int64 or int32, on a HIP device) over ``n_vertices`` vertices
    (f3dg_mesh_components, csrc/f3dg_mesh_clean.hip; the definition is include/f3dg.h's). Two faces are connected when they share a
    vertex ID (vertex connectivity, not edge adjacency; no welding of coincident vertices); a face with two equal ids is degenerate
    and belongs to no component; a face with an id outside [0, n_vertices) raises. Returns a dict:
        face_component [F] int64      the dense index of the face's component, -1 for a degenerate face
        component_sizes [C] int64     faces per component
        component_roots [C] int64     the least vertex id of each component
        n_degenerate, rounds          the degenerate faces, and the hook / compress / verify rounds the library needed
    Components are ordered by size, largest first, and by root ascending among equal sizes. Every output is a function of the input
    alone: bit-reproducible."""
    faces = _faces_arg(faces, "mesh_components")
    face_root, root_faces, counts = _components_raw(faces, int(n_vertices))
    roots, sizes, _, face_component = _rank_components(face_root, root_faces)
    return {"face_component": face_component, "component_sizes": sizes, "component_roots": roots, "n_degenerate": counts[2], "rounds": counts[3]}


def clean_mesh(vertices, faces, vertex_colors=None, *, min_faces=None, keep_largest=None, min_fraction=None):
    """Drop the small connected components ("floaters") of a mesh and renumber what is left (f3dg_mesh_components, f3dg_mesh_compact_count /
    _emit). ``vertices`` [N,3], ``faces`` [F,3] int64 or int32, ``vertex_colors`` [N,...] or None, all on one HIP device. A component
    (``mesh_components``) is kept iff it has at least ``min_faces`` faces AND is among the ``keep_largest`` first of the ranking AND has
    at least ``min_fraction`` of the largest component's faces -- each criterion only where it is given; with all three None every
    component is kept and only degenerate faces and unreferenced vertices go. Returns a dict:
        vertices [n,3], vertex_colors [n,...] or None     gathered by ``vertex_ids`` with torch indexing: differentiable
        faces [f,3] int64                                 the kept faces in their input order, in the new numbering
        vertex_ids [n] int64                              the old id of each new vertex, ascending
        face_component [f] int64, component_sizes [K]     the kept faces' component and the kept components' sizes (the kept ones are
                                                          always the first K of the ranking, so the indices are ``mesh_components``')"""
    _require_hip(vertices)
    faces = _faces_arg(faces, "clean_mesh")
    if vertices.dim() != 2 or faces.device != vertices.device:
        raise ValueError(f"clean_mesh: vertices must be [N,C] on the device of faces, got {tuple(vertices.shape)} on {vertices.device}")
    N, F, dev = int(vertices.shape[0]), int(faces.shape[0]), vertices.device
    if vertex_colors is not None:
        _require_hip(vertex_colors)
        if vertex_colors.shape[0] != N or vertex_colors.device != dev:
            raise ValueError(f"clean_mesh: vertex_colors must hold one row per vertex ({N}) on {dev}, got {tuple(vertex_colors.shape)}")
    with torch.no_grad():
        if N == 0:
            if F:
                raise ValueError("clean_mesh: faces over an empty vertex set")
            face_root = torch.empty((0,), dtype=torch.int32, device=dev)
            sizes = face_component = vertex_ids = torch.empty((0,), dtype=torch.int64, device=dev)
            keep_sizes, faces_out = sizes, torch.empty((0, 3), dtype=torch.int64, device=dev)
        else:
            face_root, root_faces, _ = _components_raw(faces, N)
            roots, sizes, _, face_component = _rank_components(face_root, root_faces)
            keep = torch.ones_like(sizes, dtype=torch.bool)
            if min_faces is not None:
                keep &= sizes >= int(min_faces)
            if keep_largest is not None:
                keep &= torch.arange(sizes.shape[0], device=dev) < int(keep_largest)
            if min_fraction is not None and sizes.shape[0]:
                keep &= sizes.to(torch.float64) >= float(min_fraction) * sizes[0].to(torch.float64)
            keep_root = torch.zeros((N,), dtype=torch.uint8, device=dev)
            keep_root[roots[keep]] = 1
            keep_sizes = sizes[keep]
            L = _lib.lib()
            nbytes = L.f3dg_mesh_compact_workspace_bytes(N, F)
            if nbytes == 0:
                raise _lib.F3dgError(_lib.ERR_UNSUPPORTED, "f3dg_mesh_compact_workspace_bytes")
            counts = (C.c_longlong * 2)()
            is32 = int(faces.dtype == torch.int32)
            with torch.cuda.device(dev):
                ws = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
                _lib.check(L.f3dg_mesh_compact_count(_stream(), _lib.ptr(ws), nbytes, N, F, _lib.ptr(faces), is32, _lib.ptr(face_root),
                                                     _lib.ptr(keep_root), counts), "f3dg_mesh_compact_count")
                nf, nv = int(counts[0]), int(counts[1])
                faces_out = torch.empty((nf, 3), dtype=torch.int64, device=dev)
                vertex_ids = torch.empty((nv,), dtype=torch.int64, device=dev)
                if nf > 0:
                    _lib.check(L.f3dg_mesh_compact_emit(_stream(), _lib.ptr(ws), nbytes, N, F, _lib.ptr(faces), is32, _lib.ptr(face_root),
                                                        _lib.ptr(keep_root), nf, nv, _lib.ptr(faces_out), _lib.ptr(vertex_ids)),
                               "f3dg_mesh_compact_emit")
            fr = face_root.to(torch.int64)
            face_component = face_component[(fr >= 0) & (keep_root[fr.clamp(min=0)] != 0)]
    return {"vertices": vertices[vertex_ids], "faces": faces_out, "vertex_colors": None if vertex_colors is None else vertex_colors[vertex_ids],
            "vertex_ids": vertex_ids, "face_component": face_component, "component_sizes": keep_sizes}


def _no_grad_input(t, who, name):
    if torch.is_tensor(t) and t.requires_grad:
        raise NotImplementedError(f"{who} produces no gradient for `{name}`: detach it (the smoothed mesh is data)")


def _vertices_arg(vertices, faces, who):
    _require_hip(vertices)
    if vertices.dim() != 2 or vertices.shape[1] != 3 or vertices.dtype != torch.float32 or vertices.device != faces.device:
        raise ValueError(f"{who}: vertices must be [N,3] float32 on the device of faces, got {tuple(vertices.shape)} {vertices.dtype} on {vertices.device}")
    return vertices.contiguous()


@torch.no_grad()
def mesh_adjacency(faces, n_vertices):
    """The vertex adjacency of the mesh ``faces`` [F,3] (int64 or int32, on a HIP device) over ``n_vertices`` vertices
    (f3dg_mesh_adjacency, csrc/f3dg_mesh_smooth.hip; the definition is include/f3dg.h's). Returns a dict:
        nbr_start [N+1] int32, nbr [2E] int32     the CSR of every vertex's distinct neighbours, ascending
        boundary [N] bool                         the vertex has an edge with exactly one face
        n_edges, n_boundary_vertices, n_degenerate, max_row     E, the flagged vertices, the faces with two equal ids (they contribute
                                                  nothing), the incidence entries of the longest row (two per incident face)
        faces, n_vertices, workspace              what ``vertex_normals`` needs to read the sorted incidence rows again
    A face with an id outside [0, n_vertices) raises. One blocking host read. Every output is a function of the input alone."""
    faces = _faces_arg(faces, "mesh_adjacency")
    N, F, dev = int(n_vertices), int(faces.shape[0]), faces.device
    if N <= 0:
        raise ValueError(f"mesh_adjacency: the mesh needs at least one vertex (got {N})")
    L = _lib.lib()
    nbytes = L.f3dg_mesh_adjacency_workspace_bytes(N, F)
    if nbytes == 0:
        raise _lib.F3dgError(_lib.ERR_UNSUPPORTED, "f3dg_mesh_adjacency_workspace_bytes")
    counts = (C.c_longlong * 4)()
    with torch.cuda.device(dev):
        ws = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
        nbr_start = torch.empty((N + 1,), dtype=torch.int32, device=dev)
        nbr = torch.empty((6 * F,), dtype=torch.int32, device=dev)
        boundary = torch.empty((N,), dtype=torch.uint8, device=dev)
        _lib.check(L.f3dg_mesh_adjacency(_stream(), _lib.ptr(ws), nbytes, N, F, _lib.ptr(faces), int(faces.dtype == torch.int32),
                                         _lib.ptr(nbr_start), _lib.ptr(nbr), _lib.ptr(boundary), counts), "f3dg_mesh_adjacency")
    two_e = int(counts[0])
    return {"nbr_start": nbr_start, "nbr": nbr[:two_e].clone(), "boundary": boundary.to(torch.bool), "n_edges": two_e // 2,
            "n_boundary_vertices": int(counts[1]), "n_degenerate": int(counts[2]), "max_row": int(counts[3]),
            "faces": faces, "n_vertices": N, "workspace": ws}


def _adjacency_for(adjacency, faces, N, who):
    if adjacency is None:
        return mesh_adjacency(faces, N)
    if adjacency["n_vertices"] != N or adjacency["nbr_start"].device != faces.device:
        raise ValueError(f"{who}: the adjacency was built for {adjacency['n_vertices']} vertices on {adjacency['nbr_start'].device}, "
                         f"the mesh has {N} on {faces.device}")
    return adjacency


@torch.no_grad()
def smooth_mesh(vertices, faces, iterations=10, lam=0.5, mu=-0.53, pin_boundary=True, pinned=None, adjacency=None):
    """Taubin lambda|mu smoothing of ``vertices`` [N,3] float32 over the mesh ``faces`` [F,3] (f3dg_mesh_smooth; the definition is
    include/f3dg.h's): ``iterations`` times a step with ``lam`` followed by a step with ``mu`` (``mu == 0``: Laplacian smoothing, one step
    per iteration), every step in float64 over the distinct neighbours of a vertex with uniform weights, rounded to float32 once.
    ``pin_boundary``: vertices with a boundary edge stay where they are (the open rim of a TSDF mesh curls otherwise); ``pinned`` [N] bool
    or uint8: further vertices that stay (OR-ed with the boundary). ``adjacency``: a ``mesh_adjacency`` of the same mesh, built here
    otherwise. Returns {"vertices": [N,3] float32 (a new tensor), "adjacency": the dict}. The result is data: an input that requires grad
    raises; bit-reproducible."""
    _no_grad_input(vertices, "smooth_mesh", "vertices")
    faces = _faces_arg(faces, "smooth_mesh")
    vertices = _vertices_arg(vertices, faces, "smooth_mesh")
    N, dev = int(vertices.shape[0]), vertices.device
    lam, mu, iterations = float(lam), float(mu), int(iterations)
    if not (0.0 < lam <= 1.0) or not (mu == 0.0 or mu < -lam) or iterations < 0:
        raise ValueError(f"smooth_mesh: needs 0 < lam <= 1, mu == 0 or mu < -lam, and iterations >= 0 (got {lam}, {mu}, {iterations})")
    if N == 0:
        return {"vertices": vertices.clone(), "adjacency": adjacency}
    adjacency = _adjacency_for(adjacency, faces, N, "smooth_mesh")
    pin = None
    if pinned is not None:
        _require_hip(pinned)
        if pinned.shape != (N,) or pinned.device != dev:
            raise ValueError(f"smooth_mesh: pinned must be [{N}] on {dev}, got {tuple(pinned.shape)} on {pinned.device}")
        pin = pinned != 0
    if pin_boundary:
        pin = adjacency["boundary"] if pin is None else pin | adjacency["boundary"]
    pin = None if pin is None else pin.to(torch.uint8).contiguous()
    with torch.cuda.device(dev):
        out, scratch = torch.empty_like(vertices), torch.empty_like(vertices)
        _lib.check(_lib.lib().f3dg_mesh_smooth(_stream(), N, _lib.ptr(adjacency["nbr_start"]), _lib.ptr(adjacency["nbr"]), _lib.ptr(pin),
                                               _lib.ptr(vertices), lam, mu, iterations, _lib.ptr(scratch), _lib.ptr(out)), "f3dg_mesh_smooth")
    return {"vertices": out, "adjacency": adjacency}


@torch.no_grad()
def vertex_normals(vertices, faces, adjacency=None):
    """Area-weighted unit vertex normals [N,3] float32 of the mesh (f3dg_mesh_vertex_normals; the definition is include/f3dg.h's): the
    float64 sum of the cross products of a vertex's faces in a canonical order, normalised; (0, 0, 0) for a vertex without a face or
    with a zero or non-finite sum. ``adjacency``: a ``mesh_adjacency`` of THESE faces (its workspace holds the sorted incidence rows),
    built here otherwise. The result is data: an input that requires grad raises; bit-reproducible."""
    _no_grad_input(vertices, "vertex_normals", "vertices")
    faces = _faces_arg(faces, "vertex_normals")
    vertices = _vertices_arg(vertices, faces, "vertex_normals")
    N, F, dev = int(vertices.shape[0]), int(faces.shape[0]), vertices.device
    if N == 0:
        return torch.empty((0, 3), dtype=torch.float32, device=dev)
    adjacency = _adjacency_for(adjacency, faces, N, "vertex_normals")
    if int(adjacency["faces"].shape[0]) != F or adjacency["faces"].dtype != faces.dtype:
        raise ValueError("vertex_normals: the adjacency was built on other faces")
    ws = adjacency["workspace"]
    with torch.cuda.device(dev):
        normals = torch.zeros((N, 3), dtype=torch.float32, device=dev)
        _lib.check(_lib.lib().f3dg_mesh_vertex_normals(_stream(), _lib.ptr(ws), ws.numel(), N, F, _lib.ptr(faces), int(faces.dtype == torch.int32),
                                                       _lib.ptr(vertices), _lib.ptr(normals)), "f3dg_mesh_vertex_normals")
    return normals


@torch.no_grad()
def simplify_mesh(vertices, faces, cell_size=None, *, grid_resolution=None, origin=None, placement="quadric", vertex_colors=None,
                  adjacency=None):
    """Reduce the mesh ``vertices`` [N,3] float32 / ``faces`` [F,3] (int64 or int32) by uniform-grid vertex clustering
    (f3dg_mesh_simplify_count / _emit, csrc/f3dg_mesh_simplify.hip; the definition is include/f3dg.h's): the vertices of one grid cell
    become one vertex, faces whose corners no longer lie in three distinct cells go, of the faces that name the same three cells the
    first stays (whatever the winding), and the result is compacted. Exactly one of ``cell_size`` (world units) and ``grid_resolution``
    (the cell is the longest side of the vertices' box divided by it, in float64) must be given; ``origin`` (three numbers) is the
    grid's corner, the per-axis minimum of the vertices when None (one host read). ``placement``:
        'root'       the cell's least vertex id, copied bit for bit. With a small cell this is grid welding: positions equal to the bit
                     always merge, positions within ``cell_size`` of each other merge unless a cell boundary runs between them
        'mean'       the members' mean
        'quadric'    the minimiser of the regularised quadric of the members' faces, within one cell of the mean (the mean otherwise):
                     planar regions stay at the mean, edges and corners are kept sharp
    ``vertex_colors`` [N,C] float32 (C <= 64) are averaged over the members. ``adjacency``: a ``mesh_adjacency`` of THESE faces (only
    'quadric' reads it), built here otherwise. Returns a dict:
        vertices [n,3], faces [f,3] int64, vertex_colors [n,C] or None
        vertex_map [N] int64         the new id of every old vertex, -1 where no surviving face uses its cell
        cluster_root [n] int64, cluster_size [n] int64     the least old id and the number of old vertices of every new vertex
        counts                       dict: clusters, used_clusters (n), degenerate, collapsed, duplicate, kept (f) faces -- the four sum
                                     to F --, max_cluster
    Not edge-collapse decimation: no error bound, no topology or manifold preservation. The result is data: an input that requires
    grad raises; bit-reproducible. A non-finite vertex, a vertex more than 2^21 cells from ``origin`` (or below it) and a face with an
    id outside [0, N) raise. One blocking host read in the library."""
    if placement not in _lib.SIMPLIFY_PLACEMENT:
        raise ValueError(f"simplify_mesh: placement must be one of {sorted(_lib.SIMPLIFY_PLACEMENT)}, got {placement!r}")
    if (cell_size is None) == (grid_resolution is None):
        raise ValueError("simplify_mesh: give exactly one of cell_size and grid_resolution")
    if cell_size is not None and not (float(cell_size) > 0.0 and math.isfinite(float(cell_size))):
        raise ValueError(f"simplify_mesh: cell_size must be positive and finite, got {cell_size}")
    if grid_resolution is not None and not 1 <= int(grid_resolution) < (1 << 21):
        raise ValueError(f"simplify_mesh: grid_resolution must be in [1, 2^21), got {grid_resolution}")
    if origin is not None:
        origin = [float(x) for x in origin]
        if len(origin) != 3 or not all(math.isfinite(x) for x in origin):
            raise ValueError(f"simplify_mesh: origin must be three finite numbers, got {origin}")
    _no_grad_input(vertices, "simplify_mesh", "vertices")
    _no_grad_input(vertex_colors, "simplify_mesh", "vertex_colors")
    faces = _faces_arg(faces, "simplify_mesh")
    vertices = _vertices_arg(vertices, faces, "simplify_mesh")
    N, F, dev = int(vertices.shape[0]), int(faces.shape[0]), vertices.device
    Cn = 0
    if vertex_colors is not None:
        _require_hip(vertex_colors)
        if vertex_colors.dim() != 2 or vertex_colors.shape[0] != N or vertex_colors.dtype != torch.float32 or vertex_colors.device != dev \
                or not 1 <= vertex_colors.shape[1] <= _lib.SIMPLIFY_MAX_ATTRS:
            raise ValueError(f"simplify_mesh: vertex_colors must be [{N},C] float32 with 1 <= C <= {_lib.SIMPLIFY_MAX_ATTRS} on {dev}, got "
                             f"{tuple(vertex_colors.shape)} {vertex_colors.dtype} on {vertex_colors.device}")
        vertex_colors = vertex_colors.contiguous()
        Cn = int(vertex_colors.shape[1])
    i64 = lambda *shape: torch.empty(shape, dtype=torch.int64, device=dev)
    if N == 0:
        if F:
            raise ValueError("simplify_mesh: faces over an empty vertex set")
        return {"vertices": vertices.clone(), "faces": i64(0, 3), "vertex_colors": None if vertex_colors is None else vertex_colors.clone(),
                "vertex_map": i64(0), "cluster_root": i64(0), "cluster_size": i64(0), "counts": dict.fromkeys(_lib.SIMPLIFY_COUNTS, 0)}
    if origin is None or grid_resolution is not None:
        box = torch.stack([vertices.amin(dim=0), vertices.amax(dim=0)]).double().cpu()
        lo, hi = box[0].tolist(), box[1].tolist()
        if not all(math.isfinite(a) and math.isfinite(b) for a, b in zip(lo, hi)):
            raise ValueError("simplify_mesh: a vertex coordinate is not finite")
        if origin is None:
            origin = lo
    if grid_resolution is not None:
        cell = max(b - a for a, b in zip(lo, hi)) / int(grid_resolution)
        if not cell > 0.0:
            raise ValueError("simplify_mesh: grid_resolution needs vertices that span a box (all of them coincide)")
    else:
        cell = float(cell_size)
    L = _lib.lib()
    nbytes = L.f3dg_mesh_simplify_workspace_bytes(N, F)
    if nbytes == 0:
        raise _lib.F3dgError(_lib.ERR_UNSUPPORTED, "f3dg_mesh_simplify_workspace_bytes")
    counts = (C.c_longlong * 8)()
    is32 = int(faces.dtype == torch.int32)
    with torch.cuda.device(dev):
        ws = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
        _lib.check(L.f3dg_mesh_simplify_count(_stream(), _lib.ptr(ws), nbytes, N, F, _lib.ptr(vertices), _lib.ptr(faces), is32,
                                              (C.c_double * 3)(*origin), cell, counts), "f3dg_mesh_simplify_count")
        n, f = int(counts[1]), int(counts[5])
        out_v = torch.empty((n, 3), dtype=torch.float32, device=dev)
        out_c = torch.empty((n, Cn), dtype=torch.float32, device=dev) if Cn else None
        out_f, vertex_map, cluster_root, cluster_size = i64(f, 3), torch.full((N,), -1, dtype=torch.int64, device=dev), i64(n), i64(n)
        if n > 0:
            adj_ws = None
            if placement == "quadric":
                adjacency = _adjacency_for(adjacency, faces, N, "simplify_mesh")
                if int(adjacency["faces"].shape[0]) != F or adjacency["faces"].dtype != faces.dtype:
                    raise ValueError("simplify_mesh: the adjacency was built on other faces")
                adj_ws = adjacency["workspace"]
            _lib.check(L.f3dg_mesh_simplify_emit(_stream(), _lib.ptr(ws), nbytes, N, F, _lib.ptr(vertices), _lib.ptr(faces), is32,
                                                 _lib.SIMPLIFY_PLACEMENT[placement], Cn, _lib.ptr(vertex_colors), _lib.ptr(adj_ws),
                                                 0 if adj_ws is None else adj_ws.numel(), n, f, _lib.ptr(out_v), _lib.ptr(out_f), _lib.ptr(out_c),
                                                 _lib.ptr(vertex_map), _lib.ptr(cluster_root), _lib.ptr(cluster_size)), "f3dg_mesh_simplify_emit")
    return {"vertices": out_v, "faces": out_f, "vertex_colors": out_c, "vertex_map": vertex_map, "cluster_root": cluster_root,
            "cluster_size": cluster_size, "counts": {k: int(c) for k, c in zip(_lib.SIMPLIFY_COUNTS, counts)}}


def _simplify_step(vertices, faces, vertex_colors, simplify_cell, simplify_placement):
    """The opt-in simplification of both mesh routes, between the clean-up and the smoothing: ``simplify_mesh``'s dict."""
    return simplify_mesh(vertices.detach(), faces, simplify_cell, placement=simplify_placement,
                         vertex_colors=None if vertex_colors is None else vertex_colors.detach())


def _smooth_and_normals(vertices, faces, smooth_iterations, smooth_lambda, smooth_mu, want_normals):
    """The tail of both mesh routes: (vertices, normals or None) after the opt-in smoothing and normals."""
    adjacency = None
    if smooth_iterations is not None:
        r = smooth_mesh(vertices.detach(), faces, iterations=smooth_iterations, lam=smooth_lambda, mu=smooth_mu)
        vertices, adjacency = r["vertices"], r["adjacency"]
    normals = vertex_normals(vertices.detach(), faces, adjacency=adjacency) if want_normals else None
    return vertices, normals


def _focal_pair(fov, H, W):
    """fx, fy in pixels as ``TSDFVolume.integrate`` forms them: ``fov`` in degrees (``cfg['model']['fov']``) or a pair ``(fx, fy)``."""
    if isinstance(fov, (tuple, list)):
        return float(fov[0]), float(fov[1])
    FoV = float(fov) * math.pi / 180
    return W / (2 * math.tan(FoV / 2.)), H / (2 * math.tan(FoV / 2.))


def interpolate_vertex_attributes(attrs, faces, face_id, bary):
    """The rasteriser's attribute interpolation as torch operations, differentiable in ``attrs`` alone: ``attrs`` [N,C], ``faces``
    [F,3], ``face_id`` [V,H,W] (-1: empty) and ``bary`` [V,3,H,W] as ``render_mesh`` returns them -> [V,C,H,W], the three gathered
    corner rows weighted by ``bary`` and summed as ``(a0 b0 + a1 b1) + a2 b2`` in float32; 0 where the pixel is empty. It equals the
    kernel's fused output within the float32 roundings of that sum (the kernel sums in float64 and rounds once)."""
    _require_hip(attrs, faces, face_id, bary)
    if attrs.dim() != 2 or face_id.dim() != 3 or bary.dim() != 4 or bary.shape[1] != 3:
        raise ValueError(f"interpolate_vertex_attributes: attrs [N,C], face_id [V,H,W], bary [V,3,H,W]; got {tuple(attrs.shape)}, "
                         f"{tuple(face_id.shape)}, {tuple(bary.shape)}")
    hit = face_id >= 0
    corners = faces.to(torch.int64)[face_id.clamp(min=0).to(torch.int64)]        # [V,H,W,3]
    w = bary.detach().permute(0, 2, 3, 1)                                        # [V,H,W,3]
    out = (attrs[corners[..., 0]] * w[..., 0:1] + attrs[corners[..., 1]] * w[..., 1:2]) + attrs[corners[..., 2]] * w[..., 2:3]
    return (out * hit[..., None].to(out.dtype)).permute(0, 3, 1, 2)


def render_mesh(vertices, faces, world_views, fov, resolution, *, vertex_colors=None, vertex_normals=None, cull='none', z_near=0.01):
    """Draw the mesh ``vertices`` [N,3] float32 / ``faces`` [F,3] (int64 or int32) from the cameras ``world_views`` [V,4,4] (or
    [V,1,4,4]; the renderer's row-vector convention) with the exact z-buffered rasteriser (f3dg_mesh_raster, csrc/f3dg_mesh_raster.hip;
    the definition is include/f3dg.h's). ``fov`` in degrees as ``cfg['model']['fov']`` or a pair ``(fx, fy)`` in pixels, as
    ``TSDFVolume.integrate`` takes it; ``resolution`` an int or ``(H, W)``; ``cull`` 'none', 'back' or 'front' (front: counter-clockwise
    in world space seen from outside); a face with a corner at or behind ``z_near`` is dropped, not clipped. Returns a dict:
        face_id [V,H,W] int32 (-1: empty), depth [V,H,W], alpha [V,H,W] (1.0 where a face is), bary [V,3,H,W]
        color [V,3,H,W] or None      ``vertex_colors`` [N,3] interpolated perspective-correctly
        normal [V,3,H,W] or None     ``vertex_normals`` [N,3] interpolated, renormalised; 0 where empty or of zero length (world space)
        counts                       dict: rasterised, near, guard, degenerate, culled (pairs; they sum to V F), large, covered (pixels)
    Geometry is data: ``vertices`` that require grad raise. Attributes that require grad go through
    ``interpolate_vertex_attributes`` (differentiable in them alone) instead of the kernel's fused output. One blocking host read;
    every output is a function of the inputs alone: bit-reproducible. A face with an id outside [0, N) raises."""
    _no_grad_input(vertices, "render_mesh", "vertices")
    _require_hip(world_views)
    faces = _faces_arg(faces, "render_mesh")
    vertices = _vertices_arg(vertices, faces, "render_mesh")
    if cull not in _lib.RASTER_CULL:
        raise ValueError(f"render_mesh: cull must be one of {sorted(_lib.RASTER_CULL)}, got {cull!r}")
    H, W = (int(resolution[0]), int(resolution[1])) if isinstance(resolution, (tuple, list)) else (int(resolution), int(resolution))
    N, F, dev = int(vertices.shape[0]), int(faces.shape[0]), vertices.device
    wv = world_views.detach().reshape(-1, 4, 4).to(torch.float32).contiguous()
    V = int(wv.shape[0])
    if N <= 0 or V <= 0 or wv.device != dev:
        raise ValueError(f"render_mesh: needs at least one vertex and one camera on {dev} (got {N} vertices, {V} cameras on {wv.device})")
    fx, fy = _focal_pair(fov, H, W)
    sets = []
    for name, a in (("vertex_colors", vertex_colors), ("vertex_normals", vertex_normals)):
        if a is not None:
            _require_hip(a)
            if tuple(a.shape) != (N, 3) or a.dtype != torch.float32 or a.device != dev:
                raise ValueError(f"render_mesh: {name} must be [{N},3] float32 on {dev}, got {tuple(a.shape)} {a.dtype} on {a.device}")
            sets.append(a)
    fused = [a for a in sets if not a.requires_grad]
    attrs = torch.cat(fused, dim=1).contiguous() if fused else None             # C = 3 or 6: both sets travel in one call
    Cn = 0 if attrs is None else int(attrs.shape[1])
    L = _lib.lib()
    nbytes = L.f3dg_mesh_raster_workspace_bytes(V, F, H, W)
    if nbytes == 0:
        raise _lib.F3dgError(_lib.ERR_UNSUPPORTED, "f3dg_mesh_raster_workspace_bytes")
    counts = (C.c_longlong * 7)()
    with torch.no_grad(), torch.cuda.device(dev):
        ws = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
        face_id = torch.empty((V, H, W), dtype=torch.int32, device=dev)
        depth = torch.empty((V, H, W), dtype=torch.float32, device=dev)
        bary = torch.empty((V, 3, H, W), dtype=torch.float32, device=dev)
        attrs_out = torch.empty((V, Cn, H, W), dtype=torch.float32, device=dev) if Cn else None
        _lib.check(L.f3dg_mesh_raster(_stream(), _lib.ptr(ws), nbytes, N, F, _lib.ptr(vertices), _lib.ptr(faces), int(faces.dtype == torch.int32),
                                      V, _lib.ptr(wv), fx, fy, H, W, float(z_near), _lib.RASTER_CULL[cull], Cn, _lib.ptr(attrs),
                                      _lib.ptr(face_id), _lib.ptr(depth), _lib.ptr(bary), _lib.ptr(attrs_out), counts), "f3dg_mesh_raster")
    planes, at = {}, 0
    for name, a in (("color", vertex_colors), ("normal", vertex_normals)):
        if a is None:
            planes[name] = None
        elif a.requires_grad:
            planes[name] = interpolate_vertex_attributes(a, faces, face_id, bary)
        else:
            planes[name] = attrs_out[:, at:at + 3]
            at += 3
    if planes["normal"] is not None:
        n = planes["normal"]
        length = n.norm(dim=1, keepdim=True)
        planes["normal"] = torch.where(length > 0, n / length.clamp(min=torch.finfo(torch.float32).tiny), torch.zeros_like(n))
    names = ("rasterised", "near", "guard", "degenerate", "culled", "large", "covered")
    return {"face_id": face_id, "depth": depth, "alpha": (face_id >= 0).to(torch.float32), "bary": bary, "color": planes["color"],
            "normal": planes["normal"], "counts": {k: int(c) for k, c in zip(names, counts)}}


@torch.no_grad()
def mesh_depth_agreement(mesh_depth, mesh_alpha, render_depth, render_alpha, alpha_min=0.5):
    """How far the depth of a drawn mesh (``render_mesh``'s ``depth`` / ``alpha``) lies from the depth the Gaussian rasteriser composited
    (``render_views``' ``rendered_depth`` / ``rendered_alpha``), over the pixels both cover (alpha >= ``alpha_min``): a dict of ``mean``
    and ``max`` |mesh depth - rendered depth| (NaN where no pixel is covered by both) and the counts ``n_both``, ``n_mesh``,
    ``n_render``. All maps [V,H,W] or [V,1,H,W]. One host read."""
    _require_hip(mesh_depth, mesh_alpha, render_depth, render_alpha)
    md, rd = mesh_depth.reshape(-1).double(), render_depth.reshape(-1).double()
    if md.shape != rd.shape or mesh_alpha.numel() != md.numel() or render_alpha.numel() != md.numel():
        raise ValueError("mesh_depth_agreement: the four maps must hold the same pixels")
    m, r = mesh_alpha.reshape(-1) >= alpha_min, render_alpha.reshape(-1) >= alpha_min
    both = m & r
    d = torch.where(both, (md - rd).abs(), torch.zeros_like(md))
    nb = both.sum()
    stats = torch.stack([d.sum() / nb, torch.where(nb > 0, d.max(), d.sum() / nb), nb.double(), m.sum().double(), r.sum().double()]).cpu().tolist()
    return {"mean": stats[0], "max": stats[1], "n_both": int(stats[2]), "n_mesh": int(stats[3]), "n_render": int(stats[4])}


@torch.no_grad()
def _mean_edge_length(vertices, faces):
    """The mean length of the three edges of every face, float64 (an edge shared by two faces counts twice). One host read."""
    if faces.shape[0] == 0:
        return 0.0
    p = vertices.double()[faces.to(torch.int64)]                                # [F,3,3]
    return float((p - p.roll(-1, dims=1)).norm(dim=2).mean())


def bake_vertex_colors(vertices, faces, images, world_views, fov, *, vertex_normals=None, alpha=None, alpha_min=0.5, depth_tol=None,
                       cos_min=0.1, mode='blend', cull='none', z_near=0.01, visibility=None):
    """Colour the vertices of a mesh from the views (f3dg_mesh_bake_colors, csrc/f3dg_mesh_bake.hip; the definition is include/f3dg.h's):
    every vertex of ``vertices`` [N,3] float32 is projected into every view of ``images`` [V,C,H,W] float32 (1 <= C <= 8; the resolution
    is taken from it) under ``world_views`` [V,4,4] (or [V,1,4,4]) and ``fov`` (degrees or a pair ``(fx, fy)``, as ``render_mesh`` takes
    them), tested against the mesh's own z-buffer, sampled bilinearly and combined over the views in ascending order. A (view, vertex)
    sample is used unless the vertex is at or behind ``z_near``, projects outside the image, lands on a pixel no face covers, lies more
    than ``depth_tol`` behind that pixel's depth (occluded), faces the camera with a cosine below ``cos_min`` (only with
    ``vertex_normals`` [N,3]; its weight is then the squared cosine, 1 otherwise), or touches a tap with ``alpha`` [V,H,W] (or
    [V,1,H,W]) below ``alpha_min`` or with a non-finite colour. ``mode``: 'blend' (the weighted mean of the used samples) or 'best' (the
    sample of the largest weight, the earliest view at a tie). ``depth_tol=None`` takes the mean edge length of the mesh (float64 in
    torch: one more host read). ``visibility``: a ``render_mesh`` result of this mesh from these cameras at this resolution to reuse;
    when None, ``render_mesh(vertices, faces, world_views, fov, (H, W), cull=cull, z_near=z_near)`` is called. Returns a dict:
        vertex_colors [N,C], weight [N]     the colour and the weight it carries (0 where no view saw the vertex)
        n_used [N] int32, best_view [N] int32 (-1: none)
        counts                               dict of (view, vertex) pairs: near, outside, uncovered, occluded, grazing, masked, used (they
                                             sum to V N), and vertices_seen
        visibility                           the ``render_mesh`` result that was used
    Geometry and frames are data: ``vertices`` or ``images`` that require grad raise. One blocking host read; every output is a function
    of the inputs alone: bit-reproducible."""
    _no_grad_input(vertices, "bake_vertex_colors", "vertices")
    _no_grad_input(images, "bake_vertex_colors", "images")
    _require_hip(images, world_views)
    faces = _faces_arg(faces, "bake_vertex_colors")
    vertices = _vertices_arg(vertices, faces, "bake_vertex_colors")
    if mode not in _lib.BAKE_MODE:
        raise ValueError(f"bake_vertex_colors: mode must be one of {sorted(_lib.BAKE_MODE)}, got {mode!r}")
    N, dev = int(vertices.shape[0]), vertices.device
    if images.dim() != 4 or images.dtype != torch.float32 or images.device != dev or not 1 <= images.shape[1] <= 8:
        raise ValueError(f"bake_vertex_colors: images must be [V,C,H,W] float32 with 1 <= C <= 8 on {dev}, got {tuple(images.shape)} "
                         f"{images.dtype} on {images.device}")
    images = images.contiguous()
    V, Cn, H, W = (int(s) for s in images.shape)
    wv = world_views.detach().reshape(-1, 4, 4).to(torch.float32).contiguous()
    if N <= 0 or int(wv.shape[0]) != V or wv.device != dev:
        raise ValueError(f"bake_vertex_colors: needs at least one vertex and one camera per image on {dev} (got {N} vertices, {V} images, "
                         f"{int(wv.shape[0])} cameras on {wv.device})")
    planes = {}
    for name, a, shape in (("vertex_normals", vertex_normals, (N, 3)), ("alpha", alpha, (V, H, W))):
        if a is not None:
            _require_hip(a)
            a = a.detach()
            if name == "alpha" and a.dim() == 4 and a.shape[1] == 1:
                a = a[:, 0]
            if tuple(a.shape) != shape or a.dtype != torch.float32 or a.device != dev:
                raise ValueError(f"bake_vertex_colors: {name} must be {list(shape)} float32 on {dev}, got {tuple(a.shape)} {a.dtype} on {a.device}")
            a = a.contiguous()
        planes[name] = a
    if visibility is None:
        visibility = render_mesh(vertices, faces, wv, fov, (H, W), cull=cull, z_near=z_near)
    face_id, depth = visibility["face_id"], visibility["depth"]
    if tuple(face_id.shape) != (V, H, W) or tuple(depth.shape) != (V, H, W) or face_id.dtype != torch.int32 or depth.dtype != torch.float32 \
            or face_id.device != dev or depth.device != dev:
        raise ValueError(f"bake_vertex_colors: visibility must hold face_id int32 and depth float32 of shape {[V, H, W]} on {dev}")
    face_id, depth = face_id.contiguous(), depth.contiguous()
    if depth_tol is None:
        depth_tol = _mean_edge_length(vertices, faces)
    fx, fy = _focal_pair(fov, H, W)
    L = _lib.lib()
    nbytes = L.f3dg_mesh_bake_workspace_bytes(V, N, H, W)
    if nbytes == 0:
        raise _lib.F3dgError(_lib.ERR_UNSUPPORTED, "f3dg_mesh_bake_workspace_bytes")
    counts = (C.c_longlong * 8)()
    with torch.no_grad(), torch.cuda.device(dev):
        ws = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
        colors = torch.empty((N, Cn), dtype=torch.float32, device=dev)
        weight = torch.empty((N,), dtype=torch.float32, device=dev)
        n_used = torch.empty((N,), dtype=torch.int32, device=dev)
        best_view = torch.empty((N,), dtype=torch.int32, device=dev)
        _lib.check(L.f3dg_mesh_bake_colors(_stream(), _lib.ptr(ws), nbytes, N, _lib.ptr(vertices), _lib.ptr(planes["vertex_normals"]), V,
                                           _lib.ptr(wv), fx, fy, H, W, float(z_near), Cn, _lib.ptr(images), _lib.ptr(face_id), _lib.ptr(depth),
                                           _lib.ptr(planes["alpha"]), float(alpha_min), float(depth_tol), float(cos_min),
                                           _lib.BAKE_MODE[mode], _lib.ptr(colors), _lib.ptr(weight), _lib.ptr(n_used), _lib.ptr(best_view),
                                           counts), "f3dg_mesh_bake_colors")
    return {"vertex_colors": colors, "weight": weight, "n_used": n_used, "best_view": best_view,
            "counts": {k: int(c) for k, c in zip(_lib.BAKE_COUNTS, counts)}, "visibility": visibility}


def _color_from_views(vertices, faces, normals, render, world_views, fov, depth_tol):
    """The tail of both mesh routes: ``bake_vertex_colors`` of the rendered frames (``render_views(..., channels="rgb_depth_alpha",
    epilogue=False)``) onto the final vertices."""
    return bake_vertex_colors(vertices.detach().contiguous(), faces, render["render"].detach().contiguous(), world_views, fov,
                              vertex_normals=normals, alpha=render["rendered_alpha"].detach(), depth_tol=depth_tol)


def build_rotation(r):
    """visualize.py:42-63: rotation matrices [P,3,3] of (unnormalised) quaternions [P,4] (w, x, y, z), in its float32 operation order."""
    norm = torch.sqrt(r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1] + r[:, 2] * r[:, 2] + r[:, 3] * r[:, 3])
    q = r / norm[:, None]
    R = torch.zeros((q.size(0), 3, 3), device=r.device, dtype=r.dtype)
    r, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    R[:, 0, 0] = 1 - 2 * (y * y + z * z)
    R[:, 0, 1] = 2 * (x * y - r * z)
    R[:, 0, 2] = 2 * (x * z + r * y)
    R[:, 1, 0] = 2 * (x * y + r * z)
    R[:, 1, 1] = 1 - 2 * (x * x + z * z)
    R[:, 1, 2] = 2 * (y * z - r * x)
    R[:, 2, 0] = 2 * (x * z - r * y)
    R[:, 2, 1] = 2 * (y * z + r * x)
    R[:, 2, 2] = 1 - 2 * (x * x + y * y)
    return R


def fov2focal(fov, pixels):
    return pixels / (2 * math.tan(fov / 2))


@torch.no_grad()
def frustum_mask(points, world_views, near=0.02, far=1e6, fov=60, resolution=256):
    """visualize.py:72-117: True where a point projects into the image of at least one context view with near <= depth <= far.
    world_views [V,4,4] (or [V,1,4,4]) are the transposed view matrices the renderer takes. As in the reference the image is
    ``resolution`` = 256 pixels square and the focal length is ``fov2focal(fov, 256)``, i.e. ``fov`` is read in radians there."""
    H = W = int(resolution)
    focal = fov2focal(fov, resolution)
    V = world_views.reshape(-1, 4, 4).shape[0]
    intrinsics = torch.tensor([[focal, 0, W / 2], [0, focal, H / 2], [0, 0, 1]], dtype=torch.float32, device=points.device).expand(V, 3, 3)
    view_matrices = world_views.reshape(-1, 4, 4).transpose(1, 2)
    homo_points = torch.cat([points, torch.ones_like(points[:, 0]).unsqueeze(-1)], dim=-1)
    view_points = torch.einsum("vbc,nc->vnb", view_matrices, homo_points)[:, :, :3]
    uv_points = torch.einsum("vbc,vnc->vnb", intrinsics, view_points)
    z = uv_points[:, :, -1:]
    uv_points = uv_points[:, :, :2] / z
    u, v = uv_points[:, :, 0], uv_points[:, :, 1]
    depth = view_points[:, :, -1]
    cull_near_fars = (depth >= near) & (depth <= far)
    return torch.any(cull_near_fars & (u >= 0) & (u <= W - 1) & (v >= 0) & (v <= H - 1), dim=0)


@torch.no_grad()
def tetra_points(world_views, near, far, fov, rotation, xyz, scale, return_unmasked=False):
    """``get_tetra_points`` (visualize.py:120-144): the point set that is tetrahedralised. Every Gaussian contributes the eight corners
    of its box, ``xyz + R (+-3 s)``, then all centres follow; the per-point scale is the largest axis of 3 s; points outside every
    context view (``frustum_mask``) are dropped. Returns (points [n,3], points_scale [n,1]).

    The reference takes the corner order from ``trimesh.creation.box()``; that order is NOT pinned here (trimesh is not a dependency):
    the corners are in binary counting order with x slowest, (-,-,-) (-,-,+) (-,+,-) ... (+,+,+). Another corner order relabels the
    tetrahedra and moves no vertex of the mesh. ``return_unmasked``: also return the 9 P points, their scales and the mask."""
    _require_hip(world_views, rotation, xyz, scale)
    rots = build_rotation(rotation)
    scale3 = torch.sqrt(torch.square(scale) + 0) * 3.
    signs = torch.tensor([[-1. if not (k >> (2 - a)) & 1 else 1. for k in range(8)] for a in range(3)], dtype=torch.float32, device=xyz.device)
    vertices = signs.unsqueeze(0).repeat(xyz.shape[0], 1, 1)              # [P,3,8]
    vertices = vertices * scale3.unsqueeze(-1)
    vertices = torch.bmm(rots, vertices).squeeze(-1) + xyz.unsqueeze(-1)
    vertices = vertices.permute(0, 2, 1).reshape(-1, 3).contiguous()
    vertices = torch.cat([vertices, xyz], dim=0)
    smax = scale3.max(dim=-1, keepdim=True)[0]
    vertices_scale = torch.cat([smax.repeat(1, 8).reshape(-1, 1), smax], dim=0)
    vertex_mask = frustum_mask(vertices, world_views, near, far, fov)
    out = (vertices[vertex_mask], vertices_scale[vertex_mask])
    return out + (vertices, vertices_scale, vertex_mask) if return_unmasked else out


@torch.no_grad()
def bisect_level_set(sweep, end_points, end_sdf, n_steps=8):
    """The binary search of visualize.py:480-516 on the edges marching tetrahedra returned: ``end_points`` [E,2,3], ``end_sdf`` [E,2,1]
    (one end on either side of the level set), ``sweep(points [n,3]) -> final_alpha [n]`` (an ``AlphaSweep``). Every step evaluates
    sdf = (1 - sweep(mid)) - 0.5 at the midpoint (l + r) / 2 and moves the LEFT end there when the midpoint's sdf has the strict sign
    of the left end's, the RIGHT end otherwise -- a midpoint sdf of exactly 0 moves the right end, as in the reference. Returns the
    final midpoints [E,3]. torch.where instead of the reference's boolean-mask assignments: no host synchronisation per step, and the
    inputs are left untouched (the reference moves the ends inside ``end_points``)."""
    left_points, right_points = end_points[:, 0, :], end_points[:, 1, :]
    left_sdf, right_sdf = end_sdf[:, 0, :], end_sdf[:, 1, :]
    if end_points.shape[0] == 0:
        return (left_points + right_points) / 2
    for _ in range(int(n_steps)):
        mid_points = (left_points + right_points) / 2
        alpha = 1 - sweep(mid_points.contiguous())
        mid_sdf = (alpha - 0.5).reshape(-1, 1)
        ind_low = ((mid_sdf < 0) & (left_sdf < 0)) | ((mid_sdf > 0) & (left_sdf > 0))
        left_sdf = torch.where(ind_low, mid_sdf, left_sdf)
        right_sdf = torch.where(ind_low, right_sdf, mid_sdf)
        left_points = torch.where(ind_low, mid_points, left_points)
        right_points = torch.where(ind_low, right_points, mid_points)
    return (left_points + right_points) / 2


@torch.no_grad()
def extract_mesh_tsdf(pc, bs, world_views, full_projs, camera_centers, bg, cfg, resolution=256, bounds=None, trunc=None, alpha_min=0.5,
                      min_component_faces=None, keep_largest=None, smooth_iterations=None, smooth_lambda=0.5, smooth_mu=-0.53,
                      vertex_normals=False, color_from_views=False, simplify_cell=None, simplify_placement="quadric"):
    """The TSDF route to a coloured mesh of image ``bs`` of the Gaussian dict ``pc`` -- no tetrahedralisation from outside, nothing but
    this package (the semantics are this project's: ``f3dgaus_amd.tsdf``). All cameras are rendered in one
    launch sequence (``render_views(..., channels="rgb_depth_alpha", epilogue=False)``), depth, alpha and colour are fused into a
    volume whose longest side has ``resolution`` voxels (cubic voxels; the other sides as many as the box needs), and the zero level
    set is triangulated. ``bounds`` = ((x0, y0, z0), (x1, y1, z1)) in world space; None takes the box of ``pc["xyz"][bs]`` padded by
    the truncation distance (one host read). ``trunc`` defaults to four voxels. Returns ``TSDFVolume.extract``'s dict, ready for
    ``ply.save_mesh_ply(path, m["vertices"], m["faces"], (m["vertex_colors"].clamp(0, 1) * 255).round().to(torch.uint8))``.

    ``min_component_faces`` / ``keep_largest`` (opt-in; with both None the dict is exactly ``extract``'s): ``clean_mesh`` with ``min_faces``
    / ``keep_largest`` on the extracted mesh. ``vertices`` / ``faces`` / ``vertex_colors`` are then the cleaned ones and ``components``
    holds ``vertex_ids`` (rows of ``interp_v``), ``face_component`` and ``component_sizes``.

    ``simplify_cell`` (opt-in, after the clean-up and before everything below, which then acts on the simplified mesh):
    ``simplify_mesh`` with that cell size in world units (a few voxels; ``origin`` the vertices' minimum) and ``simplify_placement``.
    ``vertices`` / ``faces`` / ``vertex_colors`` are then the simplified ones and ``simplify`` holds ``vertex_map`` (from the cleaned
    mesh's ids, or the extracted mesh's without a clean-up), ``cluster_root`` and ``counts``.

    ``smooth_iterations`` (opt-in, after the clean-up): ``vertices`` becomes ``smooth_mesh``'s with ``smooth_lambda`` / ``smooth_mu`` and a
    pinned boundary. ``vertex_normals`` (opt-in, last): the dict gains ``vertex_normals`` [n,3], ready for
    ``ply.save_mesh_ply(..., vertex_normals=m["vertex_normals"])``. With the defaults the dict is exactly what it was without them.

    ``color_from_views`` (opt-in, last of all): the rendered frames are baked onto the FINAL vertices (``bake_vertex_colors`` with the
    rendered alpha, the final normals if they were asked for, and ``depth_tol`` of two voxels). ``vertex_colors`` becomes the baked colour
    where a view saw the vertex and stays the volume's elsewhere; the dict gains ``vertex_colors_tsdf`` (the volume's colours) and
    ``color_views`` [n] int32 (the views that coloured each vertex)."""
    from .gaussian_renderer import render_views
    from .tsdf import TSDFVolume
    xyz = pc["xyz"][bs]
    _require_hip(xyz, world_views)
    resolution = int(resolution)
    if resolution < 2:
        raise ValueError(f"extract_mesh_tsdf: resolution {resolution} must be at least 2")
    if bounds is None:
        box = torch.stack([xyz.detach().min(dim=0)[0], xyz.detach().max(dim=0)[0]]).double().cpu()
        lo, hi = box[0].tolist(), box[1].tolist()
    else:
        lo, hi = [float(v) for v in bounds[0]], [float(v) for v in bounds[1]]
    if not all(math.isfinite(a) and math.isfinite(b) and b > a for a, b in zip(lo, hi)):
        raise ValueError(f"extract_mesh_tsdf: empty or non-finite bounds {lo} .. {hi}")
    longest = max(b - a for a, b in zip(lo, hi))
    if bounds is not None:
        voxel = longest / (resolution - 1)
    else:
        # the padded box is longest + 2 trunc wide and spans resolution - 1 voxel edges; a default trunc is four of those edges
        if trunc is None and resolution < 10:
            raise ValueError(f"extract_mesh_tsdf: resolution {resolution} leaves no room for the default padding of four voxels a side")
        voxel = longest / (resolution - 9) if trunc is None else (longest + 2 * float(trunc)) / (resolution - 1)
        pad = 4 * voxel if trunc is None else float(trunc)
        lo, hi = [a - pad for a in lo], [b + pad for b in hi]
    dims = tuple(max(2, int(math.ceil((b - a) / voxel - 1e-9)) + 1) for a, b in zip(lo, hi))
    vol = TSDFVolume(lo, voxel, dims, trunc=trunc, device=xyz.device)
    out = render_views(pc, bs, world_views, full_projs, camera_centers, bg, cfg, channels="rgb_depth_alpha", epilogue=False)
    vol.integrate(out["rendered_depth"], world_views.reshape(-1, 4, 4), cfg['model']['fov'], color=out["render"].contiguous(),
                  alpha=out["rendered_alpha"], alpha_min=alpha_min)
    m = vol.extract()
    if min_component_faces is not None or keep_largest is not None:
        c = clean_mesh(m["vertices"], m["faces"], m["vertex_colors"], min_faces=min_component_faces, keep_largest=keep_largest)
        m.update(vertices=c["vertices"], faces=c["faces"], vertex_colors=c["vertex_colors"],
                 components={k: c[k] for k in ("vertex_ids", "face_component", "component_sizes")})
    if simplify_cell is not None:
        s = _simplify_step(m["vertices"], m["faces"], m["vertex_colors"], simplify_cell, simplify_placement)
        m.update(vertices=s["vertices"], faces=s["faces"], vertex_colors=s["vertex_colors"],
                 simplify={k: s[k] for k in ("vertex_map", "cluster_root", "counts")})
    if smooth_iterations is not None or vertex_normals:
        v, n = _smooth_and_normals(m["vertices"], m["faces"], smooth_iterations, smooth_lambda, smooth_mu, vertex_normals)
        m["vertices"] = v
        if n is not None:
            m["vertex_normals"] = n
    if color_from_views and m["vertices"].shape[0]:
        b = _color_from_views(m["vertices"], m["faces"], m.get("vertex_normals"), out, world_views, cfg['model']['fov'], 2 * voxel)
        m["vertex_colors_tsdf"], m["color_views"] = m["vertex_colors"], b["n_used"]
        m["vertex_colors"] = torch.where((b["n_used"] > 0)[:, None], b["vertex_colors"], m["vertex_colors"])
    elif color_from_views:
        m["vertex_colors_tsdf"], m["color_views"] = m["vertex_colors"], torch.zeros((0,), dtype=torch.int32, device=xyz.device)
    return m


@torch.no_grad()
def extract_mesh(pc, bs, points, points_scale, cells, world_views, full_projs, camera_centers, bg, cfg, n_binary_steps=8, sweep=None,
                 min_component_faces=None, keep_largest=None, smooth_iterations=None, smooth_lambda=0.5, smooth_mu=-0.53, vertex_normals=False,
                 color_from_views=False, simplify_cell=None, simplify_placement="quadric"):
    """visualize.py:447-546 for image ``bs`` of the Gaussian dict ``pc``: alpha of ``points`` [n,3] over all cameras (one ``AlphaSweep``,
    built here unless one is handed in), marching tetrahedra of ``cells`` [F,4] (any tetrahedralisation of ``points``; the reference's
    is CGAL on the host) on sdf = alpha - 0.5, ``n_binary_steps`` bisection steps, and the scale filter
    ``|left - right| <= 3 (left_scale + right_scale)`` on the INITIAL edge ends (``points_scale`` [n,1]). Returns a dict:
        vertices [E,3], faces [nf,3] int64, keep [E] bool                      the unfiltered mesh and the filter
        vertices_filtered, faces_filtered                                      the kept vertices and the faces whose three corners
                                                                               are kept, re-indexed (what update_vertices /
                                                                               update_faces leave, :545-546)
    With ``min_component_faces`` or ``keep_largest`` set (opt-in; the keys above are untouched) the dict also carries ``vertices_clean`` /
    ``faces_clean``: ``clean_mesh`` with ``min_faces`` / ``keep_largest`` on ``vertices_filtered`` / ``faces_filtered``.
    ``simplify_cell`` (opt-in, after the clean-up): ``vertices_simplified`` / ``faces_simplified``, ``simplify_mesh`` with that cell size
    (world units) and ``simplify_placement`` on the last mesh above (the clean one if there is one, the filtered one otherwise), and
    ``simplify`` (``vertex_map`` from that mesh's ids, ``cluster_root``, ``counts``). Everything below then acts on the simplified mesh.
    ``smooth_iterations`` (opt-in, after the clean-up): ``vertices_smooth``, ``smooth_mesh`` with ``smooth_lambda`` / ``smooth_mu`` and a
    pinned boundary on the last mesh above (the simplified, the clean or the filtered one, in that order; its faces are that mesh's).
    ``vertex_normals`` (opt-in, last): ``vertex_normals`` of that mesh, on the smoothed vertices if it was smoothed.
    ``color_from_views`` (opt-in, last of all; what the dead texturing branch of visualize.py:520-537 would have done): the cameras are
    rendered once (``render_views(..., channels="rgb_depth_alpha", epilogue=False)``) and baked onto that last mesh
    (``bake_vertex_colors`` with the rendered alpha and the normals if they were asked for); the dict gains ``vertex_colors`` [n,3] (0 where
    no view saw the vertex) and ``color_views`` [n] int32."""
    from .gaussian_renderer import AlphaSweep, render_views
    _require_hip(points, points_scale, cells)
    own = sweep is None
    if own:
        sweep = AlphaSweep(pc, bs, world_views, full_projs, camera_centers, bg, cfg, max_points=points.shape[0])
    alpha = 1 - sweep(points)
    sdf = (alpha - 0.5)[None]
    verts_list, scale_list, faces_list, _ = marching_tetrahedra(points[None], cells, sdf, points_scale[None])
    end_points, end_sdf = verts_list[0]
    end_scales = scale_list[0]
    faces = faces_list[0]
    E = end_points.shape[0]
    distance = torch.norm(end_points[:, 0, :] - end_points[:, 1, :], dim=-1)
    scale = end_scales[:, 0, 0] + end_scales[:, 1, 0]
    if own and E > points.shape[0]:         # more crossing edges than points: the sweep's per-point arrays were sized for the points
        sweep = AlphaSweep(pc, bs, world_views, full_projs, camera_centers, bg, cfg, max_points=E)
    vertices = bisect_level_set(sweep, end_points, end_sdf, n_binary_steps)
    keep = distance <= 3 * scale
    face_mask = keep[faces].all(dim=1)
    new_index = torch.cumsum(keep.to(torch.int64), 0) - 1
    out = {"vertices": vertices, "faces": faces, "keep": keep,
           "vertices_filtered": vertices[keep], "faces_filtered": new_index[faces[face_mask]]}
    if min_component_faces is not None or keep_largest is not None:
        c = clean_mesh(out["vertices_filtered"], out["faces_filtered"], min_faces=min_component_faces, keep_largest=keep_largest)
        out["vertices_clean"], out["faces_clean"] = c["vertices"], c["faces"]
    mesh = "clean" if "vertices_clean" in out else "filtered"            # the mesh the opt-in steps below act on
    if simplify_cell is not None:
        s = _simplify_step(out["vertices_" + mesh], out["faces_" + mesh], None, simplify_cell, simplify_placement)
        out["vertices_simplified"], out["faces_simplified"] = s["vertices"], s["faces"]
        out["simplify"] = {k: s[k] for k in ("vertex_map", "cluster_root", "counts")}
        mesh = "simplified"
    if smooth_iterations is not None or vertex_normals:
        last = mesh
        v, n = _smooth_and_normals(out["vertices_" + last], out["faces_" + last], smooth_iterations, smooth_lambda, smooth_mu, vertex_normals)
        if smooth_iterations is not None:
            out["vertices_smooth"] = v
        if n is not None:
            out["vertex_normals"] = n
    if color_from_views:
        v, f = out["vertices_" + ("smooth" if "vertices_smooth" in out else mesh)], out["faces_" + mesh]
        if v.shape[0]:
            frames = render_views(pc, bs, world_views, full_projs, camera_centers, bg, cfg, channels="rgb_depth_alpha", epilogue=False)
            b = _color_from_views(v, f, out.get("vertex_normals"), frames, world_views, cfg['model']['fov'], None)
            out["vertex_colors"], out["color_views"] = b["vertex_colors"], b["n_used"]
        else:
            out["vertex_colors"] = torch.zeros((0, 3), dtype=torch.float32, device=v.device)
            out["color_views"] = torch.zeros((0,), dtype=torch.int32, device=v.device)
    return out
