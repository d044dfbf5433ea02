"""Truth for the mesh clean-up (f3dg_mesh_components / f3dg_mesh_compact_count / _emit, f3dgaus_amd.mesh.mesh_components / clean_mesh): a
plain numpy restatement of the definition in include/f3dg.h, a breadth-first search it is checked against, and the cases the tests share.

Definition (faces [F,3] over N vertices):
    degenerate   a face with two equal ids: no component, label -1, always dropped
    connected    two non-degenerate faces that share a vertex id (vertex connectivity), transitively
    label        the least vertex id among the vertices of the component's faces
    sizes        component_faces[root] = number of faces (duplicates count), 0 at every other index
    ranking      components by size descending, root ascending among equals
    kept face    label >= 0 and keep_root[label] != 0;  kept vertex: used by a kept face
    compaction   kept faces in input order, ids replaced by the rank of the vertex among the kept vertices; vertex_ids ascending
Only integers: every comparison in the tests is exact."""
import numpy as np


def components(faces, N):
    """Union-find over vertex ids -> (labels [F] int64 (-1 degenerate), component_faces [N] int64, n_degenerate)."""
    faces = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    assert faces.size == 0 or (faces.min() >= 0 and faces.max() < N)
    parent = list(range(N))

    def find(x):
        r = x
        while parent[r] != r:
            r = parent[r]
        while parent[x] != r:
            parent[x], x = r, parent[x]
        return r

    def union(a, b):
        a, b = find(a), find(b)
        if a != b:
            parent[max(a, b)] = min(a, b)                   # the lesser id stays the root: the root is the least id of its tree
    deg = (faces[:, 0] == faces[:, 1]) | (faces[:, 1] == faces[:, 2]) | (faces[:, 0] == faces[:, 2])
    for (a, b, c), d in zip(faces.tolist(), deg.tolist()):
        if not d:
            union(a, b)
            union(a, c)
    labels = np.array([-1 if d else find(a) for (a, _, _), d in zip(faces.tolist(), deg.tolist())], dtype=np.int64).reshape(-1)
    sizes = np.bincount(labels[labels >= 0], minlength=N).astype(np.int64)
    return labels, sizes, int(deg.sum())


def components_bfs(faces, N):
    """The same labels by a breadth-first search over the face-vertex incidence (no union-find): labels [F] int64."""
    faces = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    deg = (faces[:, 0] == faces[:, 1]) | (faces[:, 1] == faces[:, 2]) | (faces[:, 0] == faces[:, 2])
    at = [[] for _ in range(N)]
    for f, (row, d) in enumerate(zip(faces.tolist(), deg.tolist())):
        if not d:
            for v in row:
                at[v].append(f)
    labels = np.full(len(faces), -1, dtype=np.int64)
    seen = np.zeros(len(faces), dtype=bool)
    for f0 in range(len(faces)):
        if deg[f0] or seen[f0]:
            continue
        seen[f0] = True
        queue, members, least = [f0], [], N
        while queue:
            f = queue.pop()
            members.append(f)
            for v in faces[f].tolist():
                least = min(least, v)
                for g in at[v]:
                    if not seen[g]:
                        seen[g] = True
                        queue.append(g)
                at[v] = []                                  # every face at v is queued now
        labels[members] = least
    return labels


def ranking(sizes):
    """(roots [C], sizes [C]) by size descending, root ascending among equals."""
    roots = np.flatnonzero(sizes > 0)
    order = np.argsort(-sizes[roots], kind="stable")
    return roots[order], sizes[roots][order]


def dense(labels, roots):
    """labels (root ids, -1) -> indices into the ranking (-1 stays)."""
    rank = {int(r): i for i, r in enumerate(roots.tolist())}
    return np.array([rank[int(l)] if l >= 0 else -1 for l in labels.tolist()], dtype=np.int64).reshape(-1)


def compact(faces, N, labels, keep_root):
    """(faces_out [f,3] int64, vertex_ids [n] int64, kept [F] bool)."""
    faces = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    keep_root = np.asarray(keep_root).astype(bool)
    kept = (labels >= 0) & keep_root[np.maximum(labels, 0)]
    used = np.zeros(N, dtype=bool)
    used[faces[kept].reshape(-1)] = True
    vertex_ids = np.flatnonzero(used).astype(np.int64)
    new = np.cumsum(used) - 1
    return new[faces[kept]].astype(np.int64).reshape(-1, 3), vertex_ids, kept


def select(sizes_ranked, min_faces=None, keep_largest=None, min_fraction=None):
    """[C] bool over the ranking: the criteria of clean_mesh, ANDed where given."""
    keep = np.ones(len(sizes_ranked), dtype=bool)
    if min_faces is not None:
        keep &= sizes_ranked >= min_faces
    if keep_largest is not None:
        keep &= np.arange(len(sizes_ranked)) < keep_largest
    if min_fraction is not None and len(sizes_ranked):
        keep &= sizes_ranked.astype(np.float64) >= min_fraction * float(sizes_ranked[0])
    return keep


def clean(faces, N, **criteria):
    """clean_mesh's integer outputs: dict of faces, vertex_ids, face_component (dense, kept faces), component_sizes (kept)."""
    labels, sizes, _ = components(faces, N)
    roots, ranked = ranking(sizes)
    keep = select(ranked, **criteria)
    keep_root = np.zeros(N, dtype=np.uint8)
    keep_root[roots[keep]] = 1
    faces_out, vertex_ids, kept = compact(faces, N, labels, keep_root)
    return {"faces": faces_out, "vertex_ids": vertex_ids, "face_component": dense(labels, roots)[kept], "component_sizes": ranked[keep]}


# ------------------------------------------------------------------------------------------------ the shared cases
STRIP = 4099


def independent(n, offset=0):
    """n triangles that share nothing: (faces [n,3], N = 3 n + offset)."""
    return (np.arange(3 * n, dtype=np.int64).reshape(n, 3) + offset), 3 * n + offset


def strip(n_faces, order="ascending", seed=0, offset=0):
    """A triangle strip of n_faces faces over n_faces + 2 vertices (face i = positions i, i+1, i+2, every other one flipped), the
    positions mapped to vertex ids ascending, descending or by a seeded random permutation: (faces, N)."""
    n = n_faces + 2
    ids = {"ascending": np.arange(n), "descending": np.arange(n)[::-1].copy(), "random": np.random.default_rng(seed).permutation(n)}[order]
    i = np.arange(n_faces)
    pos = np.stack([i, np.where(i % 2 == 0, i + 1, i + 2), np.where(i % 2 == 0, i + 2, i + 1)], 1)
    return ids[pos].astype(np.int64) + offset, n + offset


def mixed(seed=7):
    """1,000 disjoint triangles and one 4,099-face strip (random vertex ids, above the triangles'), the face order shuffled."""
    tri, n0 = independent(1000)
    st, N = strip(STRIP, "random", seed, offset=n0)
    faces = np.concatenate([tri, st])
    return faces[np.random.default_rng(seed + 1).permutation(len(faces))], N


def oddities():
    """Duplicate faces, the four degenerate patterns, unreferenced vertices (0, 7, 8, 19 .. 24), a component joined by one vertex."""
    faces = np.array([[1, 2, 3], [3, 2, 1], [1, 2, 3],                  # duplicates, one of them reversed
                      [4, 4, 5], [4, 5, 4], [4, 5, 5], [6, 6, 6],       # a,a,b  a,b,a  a,b,b  a,a,a: vertices 4 .. 6 are used by nothing else
                      [9, 10, 11], [11, 12, 13],                        # two faces that share vertex 11 only
                      [2, 2, 9],                                        # degenerate: does NOT join the two components it touches
                      [16, 15, 14], [17, 18, 14]], dtype=np.int64)
    return faces, 25


def small_cases():
    """name -> (faces, N): every case of the GPU suite small enough for the breadth-first search."""
    out = {"one triangle": (np.array([[0, 1, 2]], dtype=np.int64), 3),
           "two sharing a vertex": (np.array([[0, 1, 2], [2, 3, 4]], dtype=np.int64), 5),
           "two disjoint": (np.array([[3, 4, 5], [0, 1, 2]], dtype=np.int64), 6),
           "oddities": oddities(), "mixed": mixed(),
           "empty": (np.zeros((0, 3), dtype=np.int64), 4)}
    for n in (63, 64, 65, 257):
        out[f"{n} independent"] = independent(n)
    for order in ("ascending", "descending", "random"):
        out[f"strip {order}"] = strip(STRIP, order, seed=3)
    return out
