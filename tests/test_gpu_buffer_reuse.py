"""Holders whose device buffers grow and are then under-filled: a small list, a large one, the small one again on ONE
context, scorer or search, each result against the same list on a fresh holder.  The buffers only grow (device_mem.h),
so the third call runs in buffers sized for the second; what it computes must not depend on that.

Both sides of every comparison are the library itself, and every case here is bit-exact (np.array_equal / ==): a sweep's
sums have one order whatever the size of the buffers they are written to, and the batched scorer's result does not
depend on the run (tests/test_gpu_path_a_batch.py holds it to the same)."""
import numpy as np
import pytest

import helicon_amd as H
from helicon_amd.grid import build_grid
from helicon_amd.solver import lsq_reconstruct_batch
from helicon_amd.symmetry_search import SymmetrySearch
from oracle import path_b as O

pytestmark = pytest.mark.gpu

APIX = 2.0


def images(ny, nx, count):
    d, br = 0.4 * ny * APIX, 2 * APIX
    clean = O.simulate_helical_projection(1, 29.0, 10.0, 1, d, br, 0, 0, ny, nx, APIX)
    rng = np.random.default_rng(3)
    return np.stack([(clean + rng.normal(0, 0.5 * clean.std(), clean.shape)).astype(np.float32) for _ in range(count)]), d, br


def lists(nx):
    """16 candidates, 400 candidates in whole runs (20 twists x 20 rises), the 16 again."""
    small = build_grid(np.arange(27.0, 31.0, 1.0), np.arange(9.0, 11.0, 0.5), (1,), tube_length=nx * APIX).params
    large = build_grid(np.arange(20.0, 40.0, 1.0), np.arange(8.0, 13.0, 0.25), (1,), tube_length=nx * APIX).params
    assert len(small) == 16 and len(large) == 400
    return [small, large, small]


def three_steps(make_engine, prepare, shape, segments):
    """small, large, small on one engine; each against a fresh engine."""
    ny, nx = shape
    imgs, d, br = images(ny, nx, segments)

    def engine():
        eng = make_engine()
        eng.set_geometry(apix=APIX, helical_diameter=d, ball_radius=br)
        prepare(eng)
        eng.set_reference(imgs)
        return eng

    with engine() as reused:
        for step, params in enumerate(lists(nx)):
            got = reused.sweep(params)
            with engine() as fresh:
                want = fresh.sweep(params)
            assert got.shape == (segments, len(params)) and np.isfinite(got).all()
            assert np.array_equal(got, want), (shape, segments, step, float(np.abs(got - want).max()))
            assert got.std() > 0


@pytest.mark.parametrize("segments", [1, 2])
def test_square_context_reused_across_growth(segments):
    """One hh_ctx at 32 x 32: candidate staging, run tables, column factors, moments grow with the 400 and are under-filled
    by the 16; with two segments so do the masked q, the covariance numerators and the summed moments."""
    three_steps(lambda: H.SweepEngine(32), lambda eng: None, (32, 32), segments)


@pytest.mark.parametrize("segments", [1, 2])
def test_general_context_reused_across_growth(segments):
    """The general-size holder (hh_gen) at 24 x 40."""
    three_steps(lambda: H.SweepEngine((24, 40)), lambda eng: None, (24, 40), segments)


@pytest.mark.parametrize("segments", [1, 2])
def test_zoomed_filtered_context_reused_across_growth(segments):
    """The zoom's holder (hh_zoom) with a spectrum filter at 32 x 32 on a 24 x 24 plane (fewer than 8 tiles): the batch's q,
    the y pass and the moments of the filter grow and are under-filled."""
    def prepare(eng):
        eng.set_zoom((8, 8), (24, 24))
        eng.set_filter(0.4, 0.05)
    three_steps(lambda: H.SweepEngine(32), prepare, (32, 32), segments)


def test_symmetry_search_reused_across_growth():
    """hh_hs_search on a 16^3 map: the list's device copy and its scores grow from 6 to 150 candidates and back."""
    rng = np.random.default_rng(11)
    z, y, x = np.meshgrid(np.arange(16), np.arange(16), np.arange(16), indexing="ij")
    r = np.hypot(y - 8, x - 8)
    vol = (np.exp(-0.5 * ((r - 4.0) / 1.5) ** 2) * (1.0 + 0.5 * np.cos(np.arctan2(y - 8, x - 8) * 2 + 0.6 * z))).astype(np.float32)
    vol += rng.normal(0, 0.05, vol.shape).astype(np.float32)

    def params(n):
        tw = np.linspace(20.0, 50.0, n)
        return np.stack([tw, 3.0 + 0.01 * np.arange(n), np.ones(n)], axis=1)

    with SymmetrySearch(vol, 1.0) as reused:
        for step, n in enumerate((6, 150, 6)):
            got = reused.search(params(n))
            with SymmetrySearch(vol, 1.0) as fresh:
                want = fresh.search(params(n))
            assert got.shape == (n,) and np.isfinite(got).all() and got.std() > 0
            assert np.array_equal(got, want), (step, float(np.abs(got - want).max()))


@pytest.mark.parametrize("interpolation", ["nn", "linear"])
def test_batched_scorer_created_and_destroyed_three_times(interpolation):
    """hh_pab_create / hh_pab_destroy three times in one process (4 candidates, a 16 x 32 image): every set-up temporary
    and every buffer of the object is released and made again; the scores are the same each time."""
    img = images(16, 32, 1)[0][0]
    kw = dict(reconstruct_diameter_2d_pixel=16, reconstruct_diameter_3d_pixel=16, reconstruct_length_2d_pixel=32,
              reconstruct_length_3d_pixel=6)
    cands = [(29.0, 2.0, 1), (31.0, 2.5, 1), (58.0, 4.0, 2), (27.5, 1.7, 1)]
    runs = []
    for _ in range(3):
        stats = {}
        res = lsq_reconstruct_batch(img, 1.0, cands, interpolation=interpolation, stats=stats, **kw)
        assert stats.get("path") != "hh_pa" and stats["launches"] > 0, stats    # the group solver, not one by one
        runs.append(res)
    for k in range(len(cands)):
        assert np.isfinite(runs[0][k][1])
        assert runs[0][k][1] == runs[1][k][1] == runs[2][k][1], (interpolation, k, [r[k][1] for r in runs])
        np.testing.assert_array_equal(runs[0][k][0][0], runs[1][k][0][0])
        np.testing.assert_array_equal(runs[0][k][0][0], runs[2][k][0][0])
