"""The mesh clean-up's truth checked against itself (no GPU): the union-find equals a breadth-first search on every shared case, labels
are least vertex ids, compaction is idempotent, and the ranking's order rule."""
import numpy as np
import pytest

import mesh_clean_truth as M

CASES = M.small_cases()


@pytest.mark.parametrize("name", sorted(CASES))
def test_union_find_equals_breadth_first_search(name):
    faces, N = CASES[name]
    labels, sizes, n_deg = M.components(faces, N)
    assert np.array_equal(labels, M.components_bfs(faces, N))
    assert sizes.sum() + n_deg == len(faces) and sizes.shape == (N,)
    for root in np.flatnonzero(sizes):
        members = faces[labels == root]
        assert members.min() == root and len(members) == sizes[root]          # the label is the least vertex id of the component
    assert (labels[labels >= 0] <= faces[labels >= 0].min(1)).all()


def test_expected_structure_of_the_cases():
    assert M.components(*CASES["two sharing a vertex"])[1].tolist() == [2, 0, 0, 0, 0]
    assert M.components(*CASES["two disjoint"])[0].tolist() == [3, 0]
    for order in ("ascending", "descending", "random"):
        labels, sizes, _ = M.components(*CASES[f"strip {order}"])
        assert (labels == 0).all() and sizes[0] == M.STRIP and np.count_nonzero(sizes) == 1
    labels, sizes, n_deg = M.components(*M.oddities())
    assert labels.tolist() == [1, 1, 1, -1, -1, -1, -1, 9, 9, -1, 14, 14] and n_deg == 5
    roots, ranked = M.ranking(sizes)
    assert roots.tolist() == [1, 9, 14] and ranked.tolist() == [3, 2, 2]       # equal sizes: the lesser root first
    _, sizes, _ = M.components(*M.mixed())
    roots, ranked = M.ranking(sizes)
    assert len(roots) == 1001 and ranked[0] == M.STRIP and (ranked[1:] == 1).all() and (np.diff(roots[1:]) > 0).all()


def test_the_criteria_keep_exactly_the_strip():
    faces, N = M.mixed()
    want = M.clean(faces, N, keep_largest=1)
    assert len(want["faces"]) == M.STRIP and len(want["vertex_ids"]) == M.STRIP + 2 and want["component_sizes"].tolist() == [M.STRIP]
    for criteria in (dict(min_faces=2), dict(min_fraction=0.5), dict(min_faces=1, keep_largest=1)):
        got = M.clean(faces, N, **criteria)
        assert all(np.array_equal(got[k], want[k]) for k in want), criteria
    everything = M.clean(faces, N)
    assert len(everything["faces"]) == len(faces) and len(everything["component_sizes"]) == 1001
    assert len(M.clean(faces, N, keep_largest=0)["faces"]) == 0 and len(M.clean(faces, N, min_faces=M.STRIP + 1)["vertex_ids"]) == 0


@pytest.mark.parametrize("name", ["oddities", "mixed", "strip random", "empty"])
def test_compaction_is_idempotent_and_consistent(name):
    faces, N = CASES[name]
    once = M.clean(faces, N)
    n = len(once["vertex_ids"])
    assert np.array_equal(once["vertex_ids"][once["faces"]], faces[M.components(faces, N)[0] >= 0])      # old ids come back through vertex_ids
    assert (np.diff(once["vertex_ids"]) > 0).all()
    twice = M.clean(once["faces"], max(n, 1))
    assert np.array_equal(twice["faces"], once["faces"]) and np.array_equal(twice["vertex_ids"], np.arange(n))
    assert np.array_equal(twice["component_sizes"], once["component_sizes"]) and np.array_equal(twice["face_component"], once["face_component"])
