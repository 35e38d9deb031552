"""The packed pair walk's six sums of a pair on their way through the wavefront's exchange buffer (helicon_hip.hip:
part_b_packed; the slot, bank and store maps on the host: tests/test_packed_reduce_host.py).

Every lane stores its six sums, 48 lanes read eight floats each back, six lanes store a double.  What can go wrong is a
slot dropped or counted twice, and a store lane that is on or off when it should not be.  Masks that put a row's whole
weight into ONE lane of its transform make a single slot carry the sum: lanes that only write (48, 63), the first and last
part of a group of eight (0, 7, 8, 47), both sides of the 48-lane cut.  A store lane wrongly off must meet stale sums, not
its own: one case sweeps the list right after a different list of the same shape under the RISE walk, on the same context
(tests/test_gpu_walk_placement.py).  Pieces of 1, 3 and 16 runs of 17 begin at a B, end at an A and leave an odd last run.

Every case forces "packed" and asserts through `last_fused_packed` that the form ran; every candidate is held to the forced
twist walk at 2e-5 — the project's tolerance between pipelines (tests/test_gpu_packed_pairs.py) — with equal arg-max, and at
most 6 picks per case to the float64 oracle at 2e-5.  The same list under any cut is bit-equal.

What no case here can see is a B store lane that is ON past the end (`ca + 1 <= nc`): at a piece's end it stores the next
piece's first run with the very bits that piece stores, and at an odd last run it stores the table's zero run one run past
the launch's candidates, where nothing reads it (measured: a library with that predicate passes all ten cases).  That end
of the predicate is held by tests/test_packed_reduce_host.py alone.
"""
import numpy as np
import pytest

import helicon_amd as H
from helicon_amd.grid import build_grid
from oracle import path_b as O
from tests import packed_reduce_cases as P

pytestmark = pytest.mark.gpu

N = 512
PIPE_TOL = 2e-5
RISES = 4.0 + 0.05 * np.arange(16)
TWISTS8, TWISTS17 = 2.0 + 0.25 * np.arange(8), 2.0 + 0.25 * np.arange(17)


def engine():
    eng = H.SweepEngine(N)
    eng.set_geometry(apix=1.0, helical_diameter=0.4 * N, ball_radius=2.0)
    return eng


def noisy(eng, truth, seed=0):
    clean = eng.simulate(*truth)
    return (clean + np.random.default_rng(seed).normal(0, 0.5 * clean.std(), clean.shape)).astype(np.float32)


def forced(eng, grid, walk, piece=0):
    eng.set_fused_walk(walk)
    eng.set_fused_piece(piece)
    try:
        scores = eng.sweep(grid)
        return scores, (eng.last_first_pass, eng.last_fused_walk, eng.last_fused_packed)
    finally:
        eng.set_fused_piece(0)
        eng.set_fused_walk("auto")


def packed(eng, grid, piece=0):
    pk, info = forced(eng, grid, "packed", piece)
    assert info == ("fused", "twists", True), (info, piece)
    return pk


def twists(eng, grid):
    tw, info = forced(eng, grid, "twists")
    assert info == ("fused", "twists", False), info
    return tw


def hold(pk, tw, img, grid, picks, mask=None, log=True, what=""):
    assert pk.shape == tw.shape == (1, len(grid)) and np.isfinite(pk).all() and pk.std() > 0
    print(f"{what}: max |packed - twists| over {len(grid)} candidates = {float(np.abs(pk - tw).max()):.3e}")
    np.testing.assert_allclose(pk, tw, rtol=0, atol=PIPE_TOL)
    assert int(np.argmax(pk)) == int(np.argmax(tw))
    assert len(picks) <= 6
    ref = O.sweep_cpu(img, grid[picks, :3], O.radial_band_mask(N, N) if mask is None else mask, apix=1.0,
                      helical_diameter=0.4 * N, ball_radius=2.0, log=log)
    print(f"{what}: max |packed - oracle| over {len(picks)} candidates = {float(np.abs(pk[0, picks] - ref).max()):.3e}, "
          f"oracle std {float(ref.std()):.3e}")
    assert np.isfinite(ref).all() and ref.std() > 0       # the mask leaves a score that tells candidates apart
    np.testing.assert_allclose(pk[0, picks], ref, rtol=0, atol=PIPE_TOL)


def grid_of(tw_list):
    grid = build_grid(tw_list, RISES, (1,), tube_length=float(N)).params
    truth = (float(tw_list[len(tw_list) // 2]), float(RISES[8]), 1)
    return grid, truth


def one_list(tw_list, mask=None, log=True, picks=(0, 17, -1), what=""):
    grid, truth = grid_of(tw_list)
    with engine() as eng:
        img = noisy(eng, truth)
        eng.set_reference(img, mask, log=log)
        tw = twists(eng, grid)
        pk = packed(eng, grid)
    hold(pk, tw, img, grid, sorted({p % len(grid) for p in picks}), mask=mask, log=log, what=what)


@pytest.mark.parametrize("t0", [0, 7, 8, 47, 48, 63])
def test_all_weight_in_one_lane(t0):
    one_list(TWISTS8, mask=P.single_lane_mask(N, t0, O.radial_band_mask(N, N)), what=f"lane {t0}")


def test_all_ones_mask():
    one_list(TWISTS8, mask=np.ones((N, N), dtype=bool), what="all-ones mask")


def test_linear_spectrum():
    one_list(TWISTS8, log=False, what="linear spectrum")


def test_pieces_of_1_3_and_16_runs_of_17_are_the_uncut_sweep():
    grid, truth = grid_of(TWISTS17)
    with engine() as eng:
        img = noisy(eng, truth)
        eng.set_reference(img)
        tw = twists(eng, grid)
        pk = packed(eng, grid)
        for piece in (1, 3, 16):
            got = packed(eng, grid, piece)
            assert np.array_equal(got, pk), (piece, float(np.abs(got - pk).max()))
    hold(pk, tw, img, grid, [0, 16 + 1, 15 * 16 + 5, 16 * 16, 17 * 16 - 1], what="17 runs")


def test_a_store_lane_that_is_off_meets_another_lists_sums():
    grid, truth = grid_of(TWISTS17)
    other = build_grid(TWISTS17 + 0.11, RISES + 0.013, (1,), tube_length=float(N)).params
    with engine() as eng:
        img = noisy(eng, truth)
        eng.set_reference(img)
        tw = twists(eng, grid)
        for piece in (0, 3):
            stale, info = forced(eng, other, "rises")
            assert info[:2] == ("fused", "rises")
            pk = packed(eng, grid, piece)
            assert not np.array_equal(stale, pk)
            print(f"piece {piece}: max |packed - twists| = {float(np.abs(pk - tw).max()):.3e}")
            np.testing.assert_allclose(pk, tw, rtol=0, atol=PIPE_TOL)
            assert int(np.argmax(pk)) == int(np.argmax(tw))
    hold(pk, tw, img, grid, [0, 16 * 16 + 2, 17 * 16 - 1], what="after another list")
