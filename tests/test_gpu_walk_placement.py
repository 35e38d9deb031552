"""Where the twist walk's workgroups stand in the launch (sweep_plan.h: twist_walk_place; the host side of the map is
tests/test_walk_place_host.py): block 0 at the head of each region and over all XCDs, the other blocks in eighths.

Placement changes no arithmetic; what it can break is coverage.  A (ky block, layer) pair the map skipped would leave the
partial sums of the context's previous sweep in place, one it hit twice is harmless — so every list is swept right after a
DIFFERENT list of the same shape on the same context (that one under the rise walk, whose placement is another map and
leaves no sum of an earlier sweep behind), and EVERY candidate is then held against the rise walk of the same list: bit for bit where the twist walk's arithmetic is the rise walk's (N = 128, 256; forced
"twists"), within 2e-5 — the project's bound between pipelines — for the packed walk at N = 512.  The lists and piece sizes
make the map's every branch run: both regions, a region A that is no multiple of eight layers, no region A at all (below one
round of slots), and pieces of 1, 3 and 16 runs (all of it region A); the masks leave 1, 3, 5 and all ky blocks.  The scores
must not depend on the piece size.  The float64 oracle (0.6 s per candidate at N = 512) takes a sample of at most 6
candidates per mask: both ends of the list, the truth, and candidates of region B.
"""
import numpy as np
import pytest

import helicon_amd as H
from helicon_amd.grid import build_grid
from oracle import path_b as O

pytestmark = pytest.mark.gpu

PIPE_TOL = 2e-5
# (rises, twists, forced piece sizes; 0 = the schedule's own cut)
LISTS = [(24, 34, (0,)), (17, 16, (0,)), (40, 18, (1, 3, 16))]
# r_hi of the radial band -> live ky blocks of eight rows (block 0 is always live); None: the default band, every block
BANDS = {None: None, 8: 1, 24: 3, 40: 5}


def engine(n):
    eng = H.SweepEngine(n)
    eng.set_geometry(apix=1.0, helical_diameter=0.4 * n, ball_radius=2.0)
    return eng


def noisy(eng, truth, seed=0):
    clean = eng.simulate(*truth)
    return (clean + np.random.default_rng(seed).normal(0, 0.5 * clean.std(), clean.shape)).astype(np.float32)


def lists_of(n, n_rises, n_twists):
    """The list under test and a different one of the same shape (another twist and rise on every candidate)."""
    twists, rises = 2.0 + 0.25 * np.arange(n_twists), 4.0 + 0.05 * np.arange(n_rises)
    grid = build_grid(twists, rises, (1,), tube_length=float(n)).params
    other = build_grid(twists + 0.11, rises + 0.013, (1,), tube_length=float(n)).params
    assert grid.shape == other.shape == (n_rises * n_twists, 4)
    return grid, other


def sweep_after_another(eng, walk, grid, other, piece=0):
    """`grid` under `walk`, right after `other` under the RISE walk: its map is not the one under test, so it fills every
    partial sum with the other list's (under the walk under test, a workgroup skipped now would have been skipped then too,
    and the sums in its place would be those of an earlier, complete sweep of this very list)."""
    try:
        eng.set_fused_walk("rises")
        stale = eng.sweep(other)
        assert (eng.last_first_pass, eng.last_fused_walk) == ("fused", "rises")
        eng.set_fused_walk(walk)
        eng.set_fused_piece(piece)
        scores = eng.sweep(grid)
        info = (eng.last_first_pass, eng.last_fused_walk, eng.last_fused_packed)
    finally:
        eng.set_fused_piece(0)
        eng.set_fused_walk("auto")
    assert not np.array_equal(stale, scores)   # the first list's sums are not the second's: left in place they would show
    return scores, info


def run_band(n, walk, expect, r_hi, exact):
    mask = None if r_hi is None else O.radial_band_mask(n, n, r_hi=r_hi)
    truth = (2.0 + 0.25 * 5, 4.0 + 0.05 * 9, 1)
    oracle_picks = {}
    with engine(n) as eng:
        img = noisy(eng, truth)
        eng.set_reference(img, mask)
        blocks = eng.fused_walk_footprint(4.0)["ky_blocks"]
        assert blocks == (BANDS[r_hi] if BANDS[r_hi] is not None else n // 16), blocks
        for n_rises, n_twists, pieces in LISTS:
            grid, other = lists_of(n, n_rises, n_twists)
            ref, ref_info = sweep_after_another(eng, "rises", grid, other)
            assert ref_info == ("fused", "rises", False)
            assert np.isfinite(ref).all() and ref.std() > 0
            first = None
            for piece in pieces:
                got, info = sweep_after_another(eng, walk, grid, other, piece)
                assert info == expect, (info, n_rises, n_twists, piece)
                assert got.shape == ref.shape == (1, len(grid)) and np.isfinite(got).all()
                err = float(np.abs(got - ref).max())
                print(f"n={n} r_hi={r_hi} {n_rises} rises x {n_twists} twists, piece {piece}: max |{walk} - rises| = {err:.3e}")
                if exact:
                    assert np.array_equal(got, ref), (n_rises, n_twists, piece, err)
                else:
                    np.testing.assert_allclose(got, ref, rtol=0, atol=PIPE_TOL)
                    assert int(np.argmax(got)) == int(np.argmax(ref))
                if first is None:
                    first = got
                assert np.array_equal(got, first), (n_rises, n_twists, piece)   # the same bits whatever the piece size
            oracle_picks[(n_rises, n_twists)] = (grid, first)
    # the oracle's sample: candidate = twist index x rises + rise index; the last rises of 24 are region B's
    grid, got = oracle_picks[(24, 34)]
    at_truth = int(np.flatnonzero((grid[:, 0] == truth[0]) & (grid[:, 1] == truth[1]))[0])
    picks = sorted({0, len(grid) - 1, at_truth, 17 * 24 + 23})
    grid2, got2 = oracle_picks[(40, 18)]
    picks2 = [0, 9 * 40 + 21]
    for g, s, p in ((grid, got, picks), (grid2, got2, picks2)):
        ref = O.sweep_cpu(img, g[p, :3], O.radial_band_mask(n, n) if mask is None else mask, apix=1.0,
                          helical_diameter=0.4 * n, ball_radius=2.0)
        print(f"n={n} r_hi={r_hi}: max |score - oracle| over {len(p)} candidates = {float(np.abs(s[0, p] - ref).max()):.3e}")
        np.testing.assert_allclose(s[0, p], ref, rtol=0, atol=PIPE_TOL)


@pytest.mark.parametrize("r_hi", list(BANDS), ids=[f"blocks_{BANDS[k] or 'all'}" for k in BANDS])
def test_packed_walk_at_512_covers_every_candidate(r_hi):
    run_band(512, "packed", ("fused", "twists", True), r_hi, exact=False)


@pytest.mark.parametrize("r_hi", list(BANDS), ids=[f"blocks_{BANDS[k] or 'all'}" for k in BANDS])
@pytest.mark.parametrize("n", [128, 256])
def test_twist_walk_is_the_rise_walk_bit_for_bit(n, r_hi):
    run_band(n, "twists", ("fused", "twists", False), r_hi, exact=True)
