"""The packed pair walk of the fused sweep at N = 512: one row transform for the two runs of a pair.

On a centrosymmetric lattice (tests/test_packed_pairs_host.py: the identity and the gate) rows A and B of a pair go through one
transform.  The arithmetic of a candidate is then NOT the twist walk's: every case forces "packed", asserts through
`last_fused_packed` that the form ran (a silent fallback would pass everything here), and holds the scores against the forced
twist walk and against the float64 CPU oracle at 2e-5, the project's tolerance between pipelines (both walks are already held
to the oracle at it), with equal arg-maxes.  `max |packed - twists|` is printed, not asserted (the float32 CPU model gives
about 1e-8).  What is bit-exact: the same list swept twice, and the same list under any cut of the workgroups' pieces —
pairs are counted from the first run of the table group, never from the piece.  Oracle samples are at most 6 candidates (0.6 s
each at this size).
"""
import numpy as np
import pytest

import helicon_amd as H
from helicon_amd.grid import build_grid
from oracle import path_b as O

pytestmark = pytest.mark.gpu

N = 512
PIPE_TOL = 2e-5
RISES = 4.0 + 0.05 * np.arange(16)


def engine(units=None, ball_radius=2.0):
    eng = H.SweepEngine(N)
    eng.set_geometry(apix=1.0, helical_diameter=0.4 * N, ball_radius=ball_radius,
                     units=None if units is None else np.asarray(units, dtype=np.float64))
    return eng


def noisy(eng, truth, seed=0):
    clean = eng.simulate(*truth)
    return (clean + np.random.default_rng(seed).normal(0, 0.5 * clean.std(), clean.shape)).astype(np.float32)


def forced(eng, grid, walk):
    eng.set_fused_walk(walk)
    try:
        scores = eng.sweep(grid)
        return scores, (eng.last_first_pass, eng.last_fused_walk, eng.last_fused_packed)
    finally:
        eng.set_fused_walk("auto")


def packed_and_twists(eng, grid):
    """Both forms of one list; the packed form must have run."""
    tw, tw_info = forced(eng, grid, "twists")
    pk, pk_info = forced(eng, grid, "packed")
    assert tw_info == ("fused", "twists", False)
    assert pk_info == ("fused", "twists", True)
    return pk, tw


def check(pk, tw, img, grid, picks, mask=None, log=True, ball_radius=2.0, what=""):
    assert pk.shape == tw.shape == (1, len(grid)) and np.isfinite(pk).all() and pk.std() > 0
    print(f"{what}: max |packed - twists| over {len(grid)} candidates = {float(np.abs(pk - tw).max()):.3e}")
    np.testing.assert_allclose(pk, tw, rtol=0, atol=PIPE_TOL)
    assert int(np.argmax(pk)) == int(np.argmax(tw))
    assert len(picks) <= 6
    ref = O.sweep_cpu(img, grid[picks, :3], O.radial_band_mask(N, N) if mask is None else mask, apix=1.0,
                      helical_diameter=0.4 * N, ball_radius=ball_radius, log=log)
    print(f"{what}: max |packed - oracle| over {len(picks)} candidates = {float(np.abs(pk[0, picks] - ref).max()):.3e}")
    np.testing.assert_allclose(pk[0, picks], ref, rtol=0, atol=PIPE_TOL)


def run_case(twists, rises=RISES, csyms=(1,), mask=None, log=True, ball_radius=2.0, n_picks=4, what=""):
    grid = build_grid(twists, rises, csyms, tube_length=float(N)).params
    runs, run_len = len(grid) // len(rises), len(rises)
    truth = (float(twists[len(twists) // 2]), float(rises[len(rises) // 2]), int(csyms[-1]))
    with engine(ball_radius=ball_radius) as eng:
        img = noisy(eng, truth)
        eng.set_reference(img, mask, log=log)
        pk, tw = packed_and_twists(eng, grid)
    at_truth = int(np.flatnonzero((grid[:, 0] == truth[0]) & (grid[:, 1] == truth[1]) & (grid[:, 2] == truth[2]))[0])
    # the first A, the first B, the truth, the last run (the partner of nothing when the runs are odd), the ends
    picks = sorted(set([0, run_len + 1, at_truth, runs * run_len - 1, (runs - 1) * run_len + 3, run_len - 1][:n_picks]))
    check(pk, tw, img, grid, picks, mask=mask, log=log, ball_radius=ball_radius, what=what)
    return pk, tw


@pytest.mark.parametrize("log", [True, False], ids=["log", "linear"])
def test_default_band(log):
    run_case(2.0 + 0.25 * np.arange(8), log=log, n_picks=6, what=f"default band, log={log}")


def test_csym_2_and_3_in_one_grid():
    run_case(2.0 + 0.25 * np.arange(4), csyms=(2, 3), what="csym 2 and 3")


def test_ball_radius_4_puts_more_into_column_0():
    run_case(2.0 + 0.25 * np.arange(5), rises=3.2 + 0.05 * np.arange(16), ball_radius=4.0, what="ball radius 4")


def test_all_ones_mask_weighs_the_row_that_keeps_two_transforms():
    """ky = 0 and ky = N/2 share one complex row of two real sequences: its wavefront keeps the two transforms."""
    run_case(2.0 + 0.25 * np.arange(4), mask=np.ones((N, N), dtype=bool), what="all-ones mask")


def test_radial_band_of_13_ky_blocks():
    run_case(2.0 + 0.25 * np.arange(6), mask=O.radial_band_mask(N, N, r_hi=100), what="r_hi = 100")


def test_pairing_does_not_depend_on_the_pieces():
    """17 twists: an odd number of runs (the last run's partner is the table's zero run), in pieces of 1, 3 and 16 runs, so
    pieces begin at a B and end at an A whose other half is computed and not stored."""
    twists = 2.0 + 0.25 * np.arange(17)
    grid = build_grid(twists, RISES, (1,), tube_length=float(N)).params
    with engine() as eng:
        img = noisy(eng, (float(twists[8]), float(RISES[8]), 1))
        eng.set_reference(img)
        pk, tw = packed_and_twists(eng, grid)
        again, info = forced(eng, grid, "packed")
        assert info == ("fused", "twists", True) and np.array_equal(again, pk)
        for piece in (1, 3, 16):
            eng.set_fused_piece(piece)
            try:
                got, info = forced(eng, grid, "packed")
            finally:
                eng.set_fused_piece(0)
            assert info == ("fused", "twists", True), piece
            assert np.array_equal(got, pk), (piece, float(np.abs(got - pk).max()))
    check(pk, tw, img, grid, [0, 16 + 1, 15 * 16 + 5, 16 * 16, 17 * 16 - 1], what="17 runs")


def fallback_case(grid, units=None, segments=1, expect_walk="twists"):
    with engine(units) as eng:
        imgs = noisy(eng, (2.5, 4.4, 1)) if segments == 1 else np.stack([noisy(eng, (2.5, 4.4, 1), seed=s) for s in range(segments)])
        eng.set_reference(imgs)
        tw, tw_info = forced(eng, grid, "twists")
        pk, pk_info = forced(eng, grid, "packed")
    assert pk_info == tw_info and pk_info[2] is False
    assert expect_walk is None or pk_info[:2] == ("fused", expect_walk)
    assert np.isfinite(tw).all() and tw.std() > 0
    assert np.array_equal(pk, tw)


def test_falls_back_when_one_run_has_a_rot():
    grid = build_grid(2.0 + 0.25 * np.arange(6), RISES, (1,), tube_length=float(N)).params
    grid[32:48, 3] = 7.5           # a whole run: the list stays whole runs and still walks twists
    fallback_case(grid)


def test_falls_back_when_one_candidate_has_a_rot():
    grid = build_grid(2.0 + 0.25 * np.arange(6), RISES, (1,), tube_length=float(N)).params
    grid[37, 3] = 7.5              # (the list is no longer whole runs: whatever takes it, it is not the packed form)
    fallback_case(grid, expect_walk=None)


def test_falls_back_with_two_units():
    grid = build_grid(2.0 + 0.25 * np.arange(5), 8.0 + 0.05 * np.arange(16), (1,), tube_length=float(N)).params
    fallback_case(grid, units=((102.4, 0.0, -3.0), (80.0, 1.0, 4.5)))


def test_falls_back_with_two_segments():
    grid = build_grid(2.0 + 0.25 * np.arange(6), RISES, (1,), tube_length=float(N)).params
    fallback_case(grid, segments=2)


def test_auto_at_the_benchmark_geometry():
    """8 twists x 16 rises fill one round of workgroups either way, 8 + 4 candidate-times against 16 + 4: auto walks twists,
    and packs the pairs ("One transform per pair": the measurement that decided it)."""
    grid = build_grid(1.0 + 0.05 * np.arange(8), 4.5 + 0.02 * np.arange(16), (1,), tube_length=float(N)).params
    with engine() as eng:
        eng.set_reference(noisy(eng, (1.2, 4.74, 1)))
        auto = eng.sweep(grid)
        info = (eng.last_first_pass, eng.last_fused_walk, eng.last_fused_packed)
        print(f"auto: {info}")
        assert info == ("fused", "twists", True)
        pk, pk_info = forced(eng, grid, "packed")
        assert pk_info == info and np.array_equal(auto, pk)
