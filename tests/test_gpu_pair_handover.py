"""The pair path of the fused twist walk (N = 512): built rows go to the transform in registers, through an exchange with
its own slot permutation (tests/pair_handover_cases.py; the lane and slot maps themselves are modelled in
tests/test_pair_handover_host.py).

The rise walk keeps the panel hand-over, so "forced twist walk == forced rise walk, bit for bit" holds the new path
against the old arithmetic in every case: over pieces that cut pairs at either half, and under masks whose 64-bin groups
of a row are live every way (all, ends only, middle only, single bins, one side, none); a few candidates per case are also held against
the float64 CPU oracle at the 2e-5 of the other sweep tests.  Several segments send q through HBM, and every score of such
a case is derived from the stored q: at N = 512 the store is always the compact one (the full form exists at N = 1024
only, which has no pair path), so that is the form the three-segment cases compare.
"""
import numpy as np
import pytest

import helicon_amd as H
from helicon_amd.grid import build_grid
from oracle import path_b as O
from tests import pair_handover_cases as C

pytestmark = pytest.mark.gpu

N = C.N
TOL = 2e-5


def engine():
    eng = H.SweepEngine(N)
    eng.set_geometry(apix=C.APIX, helical_diameter=C.DIAMETER, ball_radius=C.BALL)
    return eng


def images(segments):
    return C.oracle_image() if segments == 1 else np.stack([C.oracle_image(seed=s) for s in range(segments)])


def grid_of(twists):
    return build_grid(twists, C.RISES8, (1,), tube_length=float(N)).params


def both_walks(eng, grid):
    out = {}
    for walk in ("rises", "twists"):
        eng.set_fused_walk(walk)
        out[walk] = eng.sweep(grid)
        assert (eng.last_first_pass, eng.last_fused_walk) == ("fused", walk)
    eng.set_fused_walk("auto")
    assert np.isfinite(out["rises"]).all() and out["rises"].std() > 0
    assert np.array_equal(out["rises"], out["twists"])
    assert np.array_equal(np.argmax(out["rises"], axis=1), np.argmax(out["twists"], axis=1))
    return out["twists"]


def check_oracle(imgs, mask, grid, scores, picks, log=True):
    for s, img in enumerate(np.asarray(imgs).reshape(-1, N, N)):
        ref = O.sweep_cpu(img, grid[picks, :3], mask, apix=C.APIX, helical_diameter=C.DIAMETER, ball_radius=C.BALL, log=log)
        err = np.abs(scores[s, picks] - ref)
        print(f"segment {s}: max |score - oracle| over {len(picks)} candidates = {err.max():.3e}")
        np.testing.assert_allclose(scores[s, picks], ref, rtol=0, atol=TOL)


def picks_of(runs, segments):
    """The truth, the last candidate (the odd tail's, or a B half) and, with one segment, a B half's first rise."""
    truth = (2 if runs == 5 else 1) * 8 + 3
    return sorted({truth, runs * 8 - 1} | ({8} if segments == 1 else set()))


@pytest.mark.parametrize("log", [True, False], ids=["log", "linear"])
@pytest.mark.parametrize("segments", [1, 3])
@pytest.mark.parametrize("n_twists", [5, 4])
def test_walks_agree_and_match_the_oracle(n_twists, segments, log):
    twists = C.TWISTS5 if n_twists == 5 else C.TWISTS4
    grid, imgs, mask = grid_of(twists), images(segments), O.radial_band_mask(N, N)
    with engine() as eng:
        eng.set_reference(imgs, mask, log=log)
        scores = both_walks(eng, grid)
    assert scores.shape == (segments, n_twists * 8)
    check_oracle(imgs, mask, grid, scores, picks_of(n_twists, segments), log=log)
    if segments == 1 and log:
        assert int(np.argmax(scores[0])) == (2 if n_twists == 5 else 1) * 8 + 3   # the truth leads


@pytest.mark.parametrize("segments", [1, 3])
def test_piece_edges_give_the_unpieced_bits(segments):
    """Five runs: pieces of 3 (runs 0-2 end at the first run of a pair, runs 3-4 begin at the second of one), of 1 (one-run
    pieces at even and at odd runs: every pair is built twice, once for either half) and of 5 (the whole odd-length group,
    whose last run's partner is the table's zeroed one).  A half that is not the piece's own is built, swapped and dropped;
    every cut gives the bits of the schedule's own cut and of the rise walk."""
    grid = grid_of(C.TWISTS5)
    with engine() as eng:
        eng.set_reference(images(segments))
        whole = both_walks(eng, grid)
        eng.set_fused_walk("twists")
        for piece in (3, 1, 5):
            eng.set_fused_piece(piece)
            got = eng.sweep(grid)
            assert (eng.last_first_pass, eng.last_fused_walk) == ("fused", "twists")
            assert np.array_equal(got, whole), piece
        eng.set_fused_piece(0)
        eng.set_fused_walk("auto")


@pytest.mark.parametrize("segments", [1, 3])
@pytest.mark.parametrize("name", list(C.MASKS))
def test_masks_that_branch_the_live_groups_every_way(name, segments):
    mask = C.MASKS[name]()
    grid, imgs = grid_of(C.TWISTS4), images(segments)
    with engine() as eng:
        eng.set_reference(imgs, mask)
        scores = both_walks(eng, grid)
    check_oracle(imgs, mask, grid, scores, picks_of(4, segments) if segments == 1 else [11, 31])
