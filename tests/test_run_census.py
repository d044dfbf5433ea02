"""The run-structure scenes of helpers.make_run_scene contain what they are for (CPU only: the float64 forward's blend record,
fwd_truth.run_census). The segmented scans of csrc/f3dg_segscan.h change behaviour at runs of 16, 32 and 64 lanes (the row_bcast
steps), at runs that straddle a 64-pair batch, at more than F3DG_B5_STAGE = 6 runs ending in one batch (several staging rounds), at
lists longer than the 128-entry ring, and at partial quadrants; test_run_scenes_gpu.py runs both kernels on these scenes."""
import numpy as np
import pytest

from fwd_truth import render_fp64, run_census
from helpers import make_run_scene


def _census(name, view=0):
    sc = make_run_scene(name)
    _, rec = render_fp64(sc, view, blended=True)
    return sc, run_census(rec, sc["W"], sc["H"])


def test_wall_has_full_quadrant_runs_and_long_lists():
    _, c = _census("wall")
    rl = c["run_lengths"]
    assert np.mean(rl == 64) >= 0.25                         # entries that cover whole quadrants
    assert np.median(c["entries"]) >= 150 and c["entries"].max() >= 300     # hundreds of contributing entries per quadrant
    assert c["pairs"].max() >= 64 * 128                      # the ring of 128 wraps many times
    assert c["pairs_per_pixel"].max() >= 150                 # long per-pixel scans: T stays above 1e-4 deep into the list


def test_confetti_has_short_runs_many_ending_per_batch():
    _, c = _census("confetti")
    rl = c["run_lengths"]
    assert np.mean(rl <= 4) >= 0.98 and rl.max() <= 16
    assert c["max_runs_ending"] > 6                          # more than F3DG_B5_STAGE runs end in one batch
    assert c["pairs_per_pixel"].max() <= 8


@pytest.mark.parametrize("name", ["mixed", "odd"])
def test_mixed_scenes_cover_every_run_length(name):
    sc, c = _census(name)
    rl = c["run_lengths"]
    assert np.array_equal(np.unique(rl), np.arange(1, 65)), [n for n in range(1, 65) if not (rl == n).any()]
    for n in (15, 16, 17, 31, 32, 33, 63, 64):               # both sides of the row_bcast:15 / 31 steps and of a full wave
        assert (rl == n).sum() >= 20, n
    assert c["straddling"] >= 1000                           # runs cut by a batch boundary
    assert c["max_runs_ending"] > 6
    assert c["entries"].max() >= 300
    if name == "odd":
        assert sc["W"] % 8 and sc["H"] % 8 and sc["W"] % 16 and sc["H"] % 16
        assert c["partial"] > 0 and sc["viewmatrix"].shape[0] == 3
        for v in (1, 2):                                     # the other views hold long runs and long lists too
            _, rec = render_fp64(sc, v, blended=True)
            cv = run_census(rec, sc["W"], sc["H"])
            assert (cv["run_lengths"] == 64).sum() >= 100 and cv["entries"].max() >= 200
