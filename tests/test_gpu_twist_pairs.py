"""The twist walk at N = 512 builds two consecutive runs (twists) per pass over the factor rows, from a table that keeps
two runs to an entry; every other size keeps the one-run loop, so every case here is N = 512.

A candidate's arithmetic is the rise walk's, sum for sum, so each case sweeps its list with the walk forced to rises and
to twists and asks for `array_equal` scores and equal arg-maxes; `last_fused_walk` says that the twist loop ran.  At
most 6 candidates per case (first, last, both sides of pair and piece boundaries) are held against the float64 CPU
oracle at the 2e-5 of tests/test_gpu_twist_walk.py.  `oracle.path_b.sweep_cpu` has no argument for an explicit
asymmetric unit: the two-unit case holds its sample against the engine's per-candidate transform pipeline, as that file
does.

What the cases cover: a workgroup's piece of runs may begin at the second run of a pair and end at the first of one
(the other half is built and dropped), a table group of an odd number of runs ends on a zeroed partner, and a launch may
begin at an odd run of its table group.
"""
import numpy as np
import pytest

import helicon_amd as H
from helicon_amd.grid import build_grid
from oracle import path_b as O

pytestmark = pytest.mark.gpu

N = 512
PIPE_TOL = 2e-5
RISES8 = 4.0 + 0.05 * np.arange(8)


def engine(units=None, ball_radius=2.0):
    eng = H.SweepEngine(N)
    eng.set_geometry(apix=1.0, helical_diameter=0.4 * N, ball_radius=ball_radius,
                     units=None if units is None else np.asarray(units, dtype=np.float64))
    return eng


def noisy(eng, truth, seed=0):
    clean = eng.simulate(*truth)
    return (clean + np.random.default_rng(seed).normal(0, 0.5 * clean.std(), clean.shape)).astype(np.float32)


def both_walks(eng, grid):
    out = {}
    for walk in ("rises", "twists"):
        eng.set_fused_walk(walk)
        out[walk] = eng.sweep(grid)
        out[walk + "_info"] = (eng.last_first_pass, eng.last_fused_walk)
    eng.set_fused_walk("auto")
    return out


def check_same(r):
    assert r["rises_info"] == ("fused", "rises")
    assert r["twists_info"] == ("fused", "twists")
    assert np.isfinite(r["rises"]).all() and r["rises"].std() > 0
    assert np.array_equal(r["rises"], r["twists"])
    assert np.array_equal(np.argmax(r["rises"], axis=1), np.argmax(r["twists"], axis=1))


def sample(runs, run_len, cap=6):
    """At most `cap` candidates: the first and the last of the list, then runs 1 and 2 (the second half of the first pair,
    the first half of the second), the last run's first rise and the run before it."""
    picks = [0, runs * run_len - 1, min(1, runs - 1) * run_len + 1, min(2, runs - 1) * run_len + run_len - 2,
             (runs - 1) * run_len, max(runs - 2, 0) * run_len + 3]
    return sorted(set(picks[:cap]))


def check_oracle(imgs, mask, grid, scores, picks, ball_radius=2.0):
    for s, img in enumerate(np.asarray(imgs).reshape(-1, N, N)):
        ref = O.sweep_cpu(img, grid[picks, :3], O.radial_band_mask(N, N) if mask is None else mask, apix=1.0,
                          helical_diameter=0.4 * N, ball_radius=ball_radius)
        err = np.abs(scores[s, picks] - ref)
        print(f"segment {s}: max |score - oracle| over {len(picks)} candidates = {err.max():.3e}")
        np.testing.assert_allclose(scores[s, picks], ref, rtol=0, atol=PIPE_TOL)


def run_case(twists, rises=RISES8, mask=None, segments=1, piece=0, ball_radius=2.0, cap=6):
    grid = build_grid(twists, rises, (1,), tube_length=float(N)).params
    runs, run_len = len(twists), len(rises)
    with engine(ball_radius=ball_radius) as eng:
        truth = (float(twists[len(twists) // 2]), float(rises[len(rises) // 2]), 1)
        imgs = noisy(eng, truth) if segments == 1 else np.stack([noisy(eng, truth, seed=s) for s in range(segments)])
        eng.set_reference(imgs, mask)
        eng.set_fused_piece(piece)
        r = both_walks(eng, grid)
        eng.set_fused_piece(0)
    check_same(r)
    check_oracle(imgs, mask, grid, r["twists"], sample(runs, run_len, cap // segments), ball_radius)
    return r


@pytest.mark.parametrize("n_twists", [1, 2, 3, 5])
def test_b_absent_one_whole_pair_and_odd_tails(n_twists):
    """2 twists: one whole pair; 3 and 5: whole pairs and a last run whose partner is the table's zeroed one.  1 twist: a
    list of one run has no factor sets to share between runs, so `choose_walk` (which this form leaves as it is) gives it
    to the rise walk whatever walk is asked for; the case keeps every other assertion and says which loop ran.  A pair
    whose second run is absent is reached by the odd tails here and by the single-run pieces below."""
    if n_twists == 1:
        grid = build_grid(np.array([2.0]), RISES8, (1,), tube_length=float(N)).params
        with engine() as eng:
            img = noisy(eng, (2.0, 4.2, 1))
            eng.set_reference(img)
            r = both_walks(eng, grid)
        assert r["rises_info"] == ("fused", "rises") and r["twists_info"] == ("fused", "rises")
        assert np.array_equal(r["rises"], r["twists"])
        assert np.array_equal(np.argmax(r["rises"], axis=1), np.argmax(r["twists"], axis=1))
        check_oracle(img, None, grid, r["twists"], sample(1, 8))
        return
    run_case(2.0 + 0.25 * np.arange(n_twists))


@pytest.mark.parametrize("piece", [3, 1])
def test_pieces_that_begin_at_odd_runs_and_single_run_pieces(piece):
    """7 twists in pieces of 3 (runs 0-2, 3-5, 6: the second piece begins at the second run of a pair and ends at the first
    of one) and of 1 (every piece one run: each pair is built twice, once for either half)."""
    run_case(2.0 + 0.25 * np.arange(7), piece=piece)


def test_radial_band_of_13_ky_blocks():
    r = run_case(2.0 + 0.25 * np.arange(9), mask=O.radial_band_mask(N, N, r_hi=100))
    assert r["twists"].shape == (1, 72)


def test_two_segments_compact_q():
    """q goes through HBM (compact at this size): both halves of a pair store theirs, and the fifth run has no partner."""
    run_case(2.0 + 0.25 * np.arange(5), segments=2)


def test_two_units_csym_1_and_2_in_one_grid():
    """Csym 1 and 2, three twists each: six runs in one table group, and the table's row count changes with the unit count
    (two units: even row counts; the one-unit cases have odd ones)."""
    units = ((102.4, 0.0, -3.0), (80.0, 1.0, 4.5))
    grid = build_grid(2.0 + 0.25 * np.arange(3), 8.0 + 0.05 * np.arange(8), (1, 2), tube_length=float(N)).params
    with engine(units) as eng:
        eng.set_reference(noisy(eng, (2.25, 8.2, 2)))
        r = both_walks(eng, grid)
        picks = sample(6, 8)
        eng.set_table_path(0)
        ref = eng.sweep(grid[picks])[0]
        assert eng.last_first_pass == "transform" and eng.last_fused_walk == "none"
    check_same(r)
    np.testing.assert_allclose(r["twists"][0, picks], ref, rtol=0, atol=PIPE_TOL)


def test_long_table_with_the_factor_rows_at_their_limit():
    """Ball radius 1 (rpx = 5, slack 1e-3), rises from 1.0 A: tests/test_gpu_shared_factors.py's arithmetic gives
    kg = floor((3 + 2 * 5 + 0.002) / 1.0) + 2 = 15 of the factor buffer's 16 rows and 2 * 262 + 1 = 525 -> 532 staged table
    rows (8.5 KB per wavefront and pair: nine copy instructions, the last one partly filled), and the compute unit holds
    as many workgroups of the twist walk as of the rise walk, so a forced twist walk runs.  Two candidates against the
    oracle (1025 lattice rows each)."""
    twists, rises = 3.0 + 0.25 * np.arange(3), 1.0 + 0.01 * np.arange(8)
    grid = build_grid(twists, rises, (1,), tube_length=float(N)).params
    with engine(ball_radius=1.0) as eng:
        img = noisy(eng, (3.25, 1.04, 1))
        eng.set_reference(img)
        f = eng.fused_walk_footprint(1.0)
        print("footprint", f)
        assert (f["kg"], f["rows"]) == (15, 532) and f["per_cu_twists"] >= f["per_cu_rises"] > 0
        r = both_walks(eng, grid)
    check_same(r)
    check_oracle(img, None, grid, r["twists"], [len(grid) - 1, 8 + 1], ball_radius=1.0)
