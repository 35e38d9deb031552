"""The fused sweep's twist walk: a workgroup owns (rise, ky block) and walks the runs, against the rise walk of the same list.

The arithmetic of a candidate is the same in both walks (same factors, same table values, same order of operations), so
every case sweeps one list with the walk forced to rises and to twists and asks for `array_equal` scores and equal
arg-maxes; `last_fused_walk` says which loop ran — without it a silent fallback would pass.  A sample of at most 12
candidates (first, last, both sides of piece boundaries of the twist walk's schedule) is held against the float64 CPU
oracle at 2e-5, the tolerance tests/test_gpu_shared_factors.py holds the fused pass to against the other pipelines.
`oracle.path_b.sweep_cpu` has no argument for an explicit asymmetric unit: the two-unit case holds its sample against
the engine's per-candidate transform pipeline instead, as that file does.
"""
import ctypes as C

import numpy as np
import pytest

import helicon_amd as H
from helicon_amd import _lib
from helicon_amd.grid import build_grid
from oracle import path_b as O

pytestmark = pytest.mark.gpu

PIPE_TOL = 2e-5


def engine(n, units=None, ball_radius=2.0):
    eng = H.SweepEngine(n)
    eng.set_geometry(apix=1.0, helical_diameter=0.4 * n, ball_radius=ball_radius,
                     units=None if units is None else np.asarray(units, dtype=np.float64))
    return eng


def noisy(eng, truth, seed=0):
    clean = eng.simulate(*truth)
    return (clean + np.random.default_rng(seed).normal(0, 0.5 * clean.std(), clean.shape)).astype(np.float32)


def twist_schedule(eng, runs, run_len, rise_min):
    """The twist walk's own cut of `runs` runs of `run_len` rises: (runs_a = rises of the first region, cpw_a, cpw_b)."""
    f = eng.fused_walk_footprint(rise_min)
    out = (C.c_int64 * 15)()
    rc = _lib.lib().hh_fused_walk_choice(runs, run_len, f["ky_blocks"], f["per_cu_rises"] * f["compute_units"],
                                         f["per_cu_twists"] * f["compute_units"], 2, out)
    assert rc == 0 and out[0] == 2
    return int(out[9]), int(out[11]), int(out[13])


def sample(runs, run_len, rises_a, cpw_a, cpw_b, cap=12):
    """At most `cap` <= 12 candidates (the float64 oracle takes 0.6 s per candidate at N = 512): first, last, and the two
    runs either side of the first and last piece boundary of each schedule region (a region's rise: its first)."""
    picks = [0, runs * run_len - 1]
    for rise, cpw in ((min(rises_a, run_len - 1), cpw_b), (0, cpw_a)):
        bounds = [k for k in range(cpw, runs, cpw)] if cpw > 0 else []
        for k in ([bounds[0], bounds[-1]] if len(bounds) > 1 else bounds):
            picks += [(k - 1) * run_len + rise, k * run_len + rise]
    picks += [run_len - 1, (runs - 1) * run_len]
    return sorted(set(picks[:cap]))


def both_walks(eng, grid):
    out = {}
    for walk in ("rises", "twists"):
        eng.set_fused_walk(walk)
        out[walk] = eng.sweep(grid)
        out[walk + "_info"] = (eng.last_first_pass, eng.last_fused_walk)
    eng.set_fused_walk("auto")
    return out


def check_same(r, expect_twists=True):
    assert r["rises_info"] == ("fused", "rises")
    assert r["twists_info"] == ("fused", "twists" if expect_twists else "rises")
    assert np.isfinite(r["rises"]).all() and r["rises"].std() > 0
    assert np.array_equal(r["rises"], r["twists"])
    assert np.array_equal(np.argmax(r["rises"], axis=1), np.argmax(r["twists"], axis=1))


def check_oracle(n, imgs, mask, grid, scores, picks, log=True):
    for s, img in enumerate(np.asarray(imgs).reshape(-1, n, n)):
        ref = O.sweep_cpu(img, grid[picks, :3], O.radial_band_mask(n, n) if mask is None else mask, apix=1.0,
                          helical_diameter=0.4 * n, ball_radius=2.0, log=log)
        err = np.abs(scores[s, picks] - ref)
        print(f"n={n} segment {s}: max |score - oracle| over {len(picks)} candidates = {err.max():.3e}")
        np.testing.assert_allclose(scores[s, picks], ref, rtol=0, atol=PIPE_TOL)


def run_case(n, twists, rises, csyms=(1,), mask=None, segments=1, piece=0, ball_radius=2.0):
    grid = build_grid(twists, rises, csyms, tube_length=float(n)).params
    runs, run_len = len(grid) // len(rises), len(rises)
    with engine(n, ball_radius=ball_radius) as eng:
        truth = (float(twists[len(twists) // 2]), float(rises[len(rises) // 2]), int(csyms[-1]))
        imgs = noisy(eng, truth) if segments == 1 else np.stack([noisy(eng, truth, seed=s) for s in range(segments)])
        eng.set_reference(imgs, mask)
        eng.set_fused_piece(piece)
        r = both_walks(eng, grid)
        eng.set_fused_piece(0)
        rises_a, cpw_a, cpw_b = twist_schedule(eng, runs, run_len, float(np.min(rises)))
        if piece:
            rises_a, cpw_a, cpw_b = run_len, piece, piece
    check_same(r)
    check_oracle(n, imgs, mask, grid, r["twists"], sample(runs, run_len, rises_a, cpw_a, cpw_b, cap=(6 if n == 512 else 12) // segments))
    return r


def test_more_workgroups_than_slots_at_512():
    """24 twists x 20 rises, default mask: 20 x 32 = 640 workgroups of whole run lists > 512 resident, so the schedule has
    both regions (whole rounds of 24-run workgroups, then rises cut into pieces that begin in mid-list)."""
    run_case(512, 2.0 + 0.25 * np.arange(24), 4.0 + 0.05 * np.arange(20))


def test_two_twists_prefetch_has_a_first_and_a_last_candidate_only():
    run_case(512, np.array([2.0, 2.5]), 4.0 + 0.05 * np.arange(16))


def test_a_piece_of_one_run_prefetches_nothing():
    """17 twists in pieces of 16: every rise's second workgroup has a single run."""
    run_case(512, 2.0 + 0.25 * np.arange(17), 4.0 + 0.05 * np.arange(16), piece=16)


def test_radial_band_of_13_ky_blocks():
    mask = O.radial_band_mask(512, 512, r_hi=100)
    r = run_case(512, 2.0 + 0.25 * np.arange(8), 4.0 + 0.05 * np.arange(16), mask=mask)
    assert r["twists"].shape == (1, 128)


def test_two_segments_compact_q():
    """Two segments: q goes through HBM.  At N <= 512 q is always compact; the full form exists at N = 1024 only, where the
    rise walk runs (test_sizes_without_a_twist_walk_report_rises)."""
    run_case(512, 2.0 + 0.25 * np.arange(6), 4.0 + 0.05 * np.arange(16), segments=2)


@pytest.mark.parametrize("n, n_twists", [(256, 6), (64, 4)])
def test_smaller_sizes_copy_several_rows_per_wavefront(n, n_twists):
    run_case(n, 20.0 + 1.0 * np.arange(n_twists), (4.0 if n == 256 else 6.0) + 0.05 * np.arange(16))


@pytest.mark.parametrize("segments", [1, 2])
def test_sizes_without_a_twist_walk_report_rises(segments):
    """N = 1024 keeps the rise walk (SPLIT rows): a forced twist walk falls back and says so; two segments there store
    the full q."""
    n = 1024
    grid = build_grid(2.0 + 0.25 * np.arange(4), 9.0 + 0.05 * np.arange(16), (1,), tube_length=float(n)).params
    with engine(n) as eng:
        imgs = noisy(eng, (2.5, 9.4, 1)) if segments == 1 else np.stack([noisy(eng, (2.5, 9.4, 1), seed=s) for s in range(2)])
        eng.set_reference(imgs)
        r = both_walks(eng, grid)
        auto = eng.sweep(grid)
        assert eng.last_fused_walk == "rises"
    check_same(r, expect_twists=False)
    assert np.array_equal(auto, r["rises"])


def test_two_units_csym_1_and_2_in_one_grid():
    """A two-unit asymmetric unit (even table row counts; the one-unit cases have odd ones) with csym 1 and 2."""
    n, units = 512, ((102.4, 0.0, -3.0), (80.0, 1.0, 4.5))
    twists, rises = 2.0 + 0.25 * np.arange(5), 8.0 + 0.05 * np.arange(16)
    grid = build_grid(twists, rises, (1, 2), tube_length=float(n)).params
    with engine(n, units) as eng:
        eng.set_reference(noisy(eng, (2.5, 8.4, 2)))
        r = both_walks(eng, grid)
        picks = sample(10, 16, 16, 10, 10)
        eng.set_table_path(0)
        ref = eng.sweep(grid[picks])[0]
        assert eng.last_first_pass == "transform" and eng.last_fused_walk == "none"
    check_same(r)
    np.testing.assert_allclose(r["twists"][0, picks], ref, rtol=0, atol=PIPE_TOL)


def test_a_run_with_one_different_rise_walks_rises():
    """Per-candidate factor sets: no workgroup can keep one set, so auto and a forced twist walk both walk rises, and the
    scores are those of the forced rise walk."""
    grid = build_grid(2.0 + 0.25 * np.arange(4), 4.0 + 0.05 * np.arange(16), (1,), tube_length=512.0).params
    grid[16 + 5, 1] += 0.01
    with engine(512) as eng:
        eng.set_reference(noisy(eng, (2.5, 4.4, 1)))
        r = both_walks(eng, grid)
        auto = eng.sweep(grid)
        assert eng.last_fused_walk == "rises" and eng.last_factor_sets == len(grid)
    check_same(r, expect_twists=False)
    assert np.array_equal(auto, r["rises"])


def test_footprint_that_loses_a_resident_workgroup_walks_rises():
    """Double-buffered table rows cost 16 B per table row and ky instead of 8, a single factor set saves kg x 2 KB: where
    the rows outweigh the set (a narrow ball: few rows per column group, a long table) the twist walk's workgroup can
    be the larger one.  The rise is the largest on a 0.01 grid at which the compute unit holds fewer twist-walking than
    rise-walking workgroups, by the library's own footprint report; there auto and a forced twist walk both walk rises."""
    n, ball = 512, 0.8
    with engine(n, ball_radius=ball) as eng:
        eng.set_reference(noisy(eng, (2.5, 2.0, 1)))
        found = None
        for rise in np.arange(4.0, 0.5, -0.01):
            f = eng.fused_walk_footprint(float(rise))
            if f["per_cu_rises"] > 0 and f["per_cu_twists"] < f["per_cu_rises"]:
                found = (float(rise), f)
                break
        assert found is not None, "no rise of the scan loses a workgroup"
        rise, f = found
        print("footprint", rise, f)
        assert f["lds_twists"] > f["lds_rises"]
        grid = build_grid(2.0 + 0.25 * np.arange(4), rise + 0.01 * np.arange(16), (1,), tube_length=float(n)).params
        r = both_walks(eng, grid)
        auto = eng.sweep(grid)
        assert eng.last_fused_walk == "rises" and eng.last_factor_sets == 16
    check_same(r, expect_twists=False)
    assert np.array_equal(auto, r["rises"])


def test_auto_walks_twists_with_one_segment_and_rises_with_several():
    """Auto: 8 twists x 16 rises in one round of workgroups (8 + 4 candidate-times against 16 + 4) take the twist walk; with several segments (q stores, measured slower on the twist walk)
    it keeps the rise walk.  (The three-twist rule needs a full device: tests/test_twist_walk_host.py.)"""
    n = 64
    rises = 6.0 + 0.05 * np.arange(16)
    grid = build_grid(20.0 + 1.0 * np.arange(8), rises, (1,), tube_length=float(n)).params
    with engine(n) as eng:
        imgs = np.stack([noisy(eng, (24.0, 6.4, 1), seed=s) for s in range(2)])
        eng.set_reference(imgs[0])
        one = eng.sweep(grid)
        assert (eng.last_first_pass, eng.last_fused_walk) == ("fused", "twists")
        eng.set_fused_walk("rises")
        assert np.array_equal(eng.sweep(grid), one) and eng.last_fused_walk == "rises"
        eng.set_fused_walk("auto")
        eng.set_reference(imgs)
        two = eng.sweep(grid)
        assert (eng.last_first_pass, eng.last_fused_walk) == ("fused", "rises")
    np.testing.assert_allclose(two[0], one[0], rtol=0, atol=2e-6)   # tests/test_gpu_shared_factors.py: SEG_TOL
