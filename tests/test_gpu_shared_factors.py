"""The fused sweep with one set of column factors per rise (a list whose runs all carry the same rise column) and with
run tables trimmed to the rows the image can reach.

The column factors depend on the rise alone, so sharing them must not move a single bit: every case here compares the
shared form against the per-candidate form of the same arithmetic (`array_equal`), and `last_factor_sets` says which
form ran — without it a silent fallback would pass.  Agreement with the other pipelines is held to the 2e-5 of the
existing parity tests, the several-segment form to 2e-6.
"""
import functools

import numpy as np
import pytest

import helicon_amd as H
from helicon_amd.grid import build_grid

pytestmark = pytest.mark.gpu

PIPE_TOL = 2e-5
SEG_TOL = 2e-6

# (n, apix, units (r, azimuth, z) or None, csyms, twists, rises): 6 twists x 16 rises each
CASES = {
    "n64": (64, 2.0, None, (1,), np.arange(25.0, 31.0), 8.0 + 0.25 * np.arange(16)),
    "n128_two_units_csym": (128, 2.0, ((51.2, 0.0, -3.0), (40.0, 1.0, 4.5)), (1, 2, 3), np.arange(25.0, 31.0),
                            9.0 + 0.25 * np.arange(16)),
}


def engine(n, apix, units=None, ball_radius=None):
    eng = H.SweepEngine(n)
    eng.set_geometry(apix=apix, helical_diameter=0.4 * n * apix, ball_radius=2 * apix if ball_radius is None else ball_radius,
                     units=None if units is None else np.asarray(units, dtype=np.float64))
    return eng


def noisy(eng, truth, seed=0):
    clean = eng.simulate(*truth)
    return (clean + np.random.default_rng(seed).normal(0, 0.5 * clean.std(), clean.shape)).astype(np.float32)


def reversed_run(params, run_len, run):
    """The same candidates with one run's rises reversed, and where each of them sits in the original list."""
    out, src = params.copy(), np.arange(len(params))
    sl = slice(run * run_len, (run + 1) * run_len)
    out[sl], src[sl] = params[sl][::-1], src[sl][::-1]
    return out, src


@functools.lru_cache(maxsize=None)
def swept(case, log):
    """Every sweep the tests of one case need, computed once: list A (twist-major), list B (one run reversed), A on
    the run-table and on the transform pipeline."""
    n, apix, units, csyms, twists, rises = CASES[case]
    grid = build_grid(twists, rises, csyms, tube_length=n * apix).params
    b_list, src = reversed_run(grid, len(rises), 2)
    with engine(n, apix, units) as eng:
        eng.set_reference(noisy(eng, (float(twists[3]), float(rises[7]), int(csyms[-1]))), log=log)
        a = eng.sweep(grid)[0]
        a_info = (eng.last_first_pass, eng.last_factor_sets)
        b = eng.sweep(b_list)[0]
        b_info = (eng.last_first_pass, eng.last_factor_sets)
        eng.set_table_path(1)
        tables = eng.sweep(grid)[0]
        assert eng.last_first_pass == "run_tables" and eng.last_factor_sets == 0
        eng.set_table_path(0)
        transform = eng.sweep(grid)[0]
        assert eng.last_first_pass == "transform" and eng.last_factor_sets == 0
    return dict(grid=grid, src=src, a=a, a_info=a_info, b=b, b_info=b_info, tables=tables, transform=transform)


@pytest.mark.parametrize("log", [True, False], ids=["log", "linear"])
@pytest.mark.parametrize("case", list(CASES))
def test_shared_factors_are_bit_identical_to_per_candidate_factors(case, log):
    r = swept(case, log)
    run_len = 16
    assert r["a_info"] == ("fused", run_len)               # one set per rise
    assert r["b_info"] == ("fused", len(r["grid"]))        # one run differs: every candidate its own set
    assert np.isfinite(r["a"]).all() and r["a"].std() > 0
    assert np.array_equal(r["b"], r["a"][r["src"]])


@pytest.mark.parametrize("log", [True, False], ids=["log", "linear"])
@pytest.mark.parametrize("case", list(CASES))
def test_shared_factors_agree_with_the_other_pipelines(case, log):
    r = swept(case, log)
    for name in ("tables", "transform"):
        np.testing.assert_allclose(r["a"], r[name], rtol=0, atol=PIPE_TOL, err_msg=name)
        assert int(np.argmax(r["a"])) == int(np.argmax(r[name])), name


def test_several_segments_on_a_shared_grid():
    """EPI_QSTORE: three segments against a shared grid; every segment's row equals its one-segment sweep."""
    n, apix, _, _, twists, rises = CASES["n64"]
    grid = build_grid(twists, rises, (1,), tube_length=n * apix).params
    with engine(n, apix) as eng:
        imgs = np.stack([noisy(eng, (28.0, 9.75, 1), seed=s) for s in range(3)])
        eng.set_reference(imgs)
        multi = eng.sweep(grid)
        assert eng.last_first_pass == "fused" and eng.last_factor_sets == 16 and multi.shape == (3, 96)
        for s in range(3):
            eng.set_reference(imgs[s])
            single = eng.sweep(grid)[0]
            assert eng.last_factor_sets == 16
            np.testing.assert_allclose(multi[s], single, rtol=0, atol=SEG_TOL, err_msg=f"segment {s}")


def test_n1024_split_rows_on_a_shared_grid():
    n, apix = 1024, 1.0
    grid = build_grid(np.array([2.38, 2.40]), 9.5 + 0.01 * np.arange(-4, 4), (2,), tube_length=n * apix).params
    with engine(n, apix) as eng:
        eng.set_reference(noisy(eng, (2.40, 9.5, 2), seed=3))
        fused = eng.sweep(grid)[0]
        assert eng.last_first_pass == "fused" and eng.last_factor_sets == 8
        eng.set_table_path(0)
        transform = eng.sweep(grid)[0]
        assert eng.last_first_pass == "transform"
    np.testing.assert_allclose(fused, transform, rtol=0, atol=PIPE_TOL)
    assert int(np.argmax(fused)) == int(np.argmax(transform))


def long_list(n_twists, n_rises):
    rises = np.linspace(6.0, 14.0, n_rises)
    p = np.empty((n_twists * n_rises, 4))
    p[:, 0] = np.repeat(27.0 + np.arange(n_twists), n_rises)
    p[:, 1] = np.tile(rises, n_twists)
    p[:, 2], p[:, 3] = 1.0, 0.0
    return p


def test_two_launches_of_one_whole_run_each_share_one_factor_buffer():
    """2 twists x 70,000 rises at N = 32: a launch holds at most 131,072 candidates, so one run each.  The second
    launch reads the factors the first one's sweep computed from run 0."""
    p = long_list(2, 70000)
    with engine(32, 2.0) as eng:
        eng.set_reference(noisy(eng, (28.0, 10.0, 1)))
        both = eng.sweep(p)[0]
        assert eng.last_first_pass == "fused" and eng.last_factor_sets == 70000
        alone = eng.sweep(p[70000:])[0]
        assert eng.last_first_pass == "fused" and eng.last_factor_sets == 70000   # a single run: its own candidates' sets
    assert np.isfinite(both).all() and both.std() > 0
    assert np.array_equal(both[70000:], alone)


def test_one_run_longer_than_a_launch_keeps_per_piece_factors():
    p = long_list(1, 140000)
    with engine(32, 2.0) as eng:
        eng.set_reference(noisy(eng, (27.0, 10.0, 1)))
        whole = eng.sweep(p)[0]
        assert eng.last_first_pass == "fused" and eng.last_factor_sets == 140000
        halves = np.concatenate([eng.sweep(p[:70000])[0], eng.sweep(p[70000:])[0]])
    assert np.array_equal(whole, halves)


def test_ragged_list_shares_factors_on_its_whole_runs():
    """The list starts three candidates into a run and ends inside one: head and tail go through the transform
    pipeline, the four whole runs between them through the fused pass with one factor set per rise."""
    n, apix, _, _, twists, rises = CASES["n64"]
    grid = build_grid(twists, rises, (1,), tube_length=n * apix).params
    ragged = grid[3:5 * 16 + 9]
    with engine(n, apix) as eng:
        eng.set_reference(noisy(eng, (28.0, 9.75, 1)))
        got = eng.sweep(ragged)[0]
        assert eng.last_first_pass == "fused" and eng.last_factor_sets == 16
        eng.set_table_path(0)
        ref = eng.sweep(ragged)[0]
        assert eng.last_first_pass == "transform" and eng.last_factor_sets == 0
    np.testing.assert_allclose(got, ref, rtol=0, atol=PIPE_TOL)


def fused_fit(n, apix, rpx, slack, rise_min, trimmed):
    """plan_runs' arithmetic for one unit: (kg, rows staged per ky, LDS bytes of k_fused_pass, fits)."""
    full = int(np.ceil(n * apix / rise_min))
    ext = min(full, int(np.floor(((n // 2 + rpx) * apix + slack) * (1 + 1e-5) / rise_min)) + 1) if trimmed else full
    kg = int(np.floor(((3 + 2 * rpx) * apix + 2 * slack) / rise_min)) + 2
    rows = max(2 * ext + 1, kg)
    rows += (4 - rows % 8 + 8) % 8
    lds = 8 * (n + 4) * 8 + 8 * rows * 8 + 2 * (kg * n * 4 + (n // 4 + 4) * 4)      # KF<N>::lds, N < 1024
    return kg, rows, lds, kg <= 16 and lds <= 160 * 1024 - 1024


def check_fused_against_transform(n, apix, ball_radius, rise_min, truth_twist):
    grid = build_grid(np.array([truth_twist - 1.0, truth_twist]), rise_min + 0.01 * np.arange(8), (1,), tube_length=n * apix).params
    with engine(n, apix, ball_radius=ball_radius) as eng:
        eng.set_reference(noisy(eng, (truth_twist, rise_min + 0.04, 1)))
        fused = eng.sweep(grid)[0]
        assert eng.last_first_pass == "fused" and eng.last_factor_sets == 8
        eng.set_table_path(0)
        transform = eng.sweep(grid)[0]
    np.testing.assert_allclose(fused, transform, rtol=0, atol=PIPE_TOL)
    assert np.isfinite(fused).all() and fused.std() > 0


def test_smallest_fused_rise_at_64():
    """N = 64, apix 2, ball radius 4 (rpx = 10, slack = 1e-3): four columns span (3 + 2 rpx) apix + 2 slack = 46.002 A,
    so kg = floor(46.002 / rise) + 2 <= 16 needs rise > 46.002 / 15 = 3.0668.  At 3.07 the lattice's own table has
    2 ceil(128 / 3.07) + 1 = 85 -> 92 staged rows and the pass needs 4352 + 64 * 92 + 2 * (16 * 256 + 80) = 18,592 B of
    LDS — at this size the 16-row factor limit always binds before the 159 KB of LDS do (a table of 2,300 rows would need
    rise < 0.11 A, where kg is in the hundreds), so there is no rise at N = 64 that only the trimmed extent fuses: the
    smallest fused rise is the same before and after, and it is swept here.  The LDS-bound pair is the N = 512 test."""
    assert fused_fit(64, 2.0, 10, 1e-3, 3.07, False) == (16, 92, 18592, True)
    assert fused_fit(64, 2.0, 10, 1e-3, 3.07, True)[0::3] == (16, True)
    assert not fused_fit(64, 2.0, 10, 1e-3, 3.06, True)[3]          # kg = 17
    check_fused_against_transform(64, 2.0, 4.0, 3.07, 28.0)


@pytest.mark.parametrize("rise_min", [1.0, 0.95])
def test_rises_where_the_fused_pass_starts_to_fit_at_512(rise_min):
    """N = 512, apix 1, ball radius 1 (rpx = 5, slack = 1e-3), the smallest size at which the LDS limit of 162,816 B can
    bind while kg <= 16.  With the lattice's own extent ceil(512 / rise):
      rise 1.00: kg 15, 2 * 512 + 1 = 1025 -> 1028 rows, 33,024 + 64 * 1028 + 2 * (15 * 2048 + 528) = 161,312 B: fits;
      rise 0.95: kg 15, 2 * 539 + 1 = 1079 -> 1084 rows, 164,896 B: does not fit (run tables / transform pipeline).
    With the extent the image can reach, floor(261.001 * (1 + 1e-5) / rise) + 1:
      rise 1.00: 262 -> 525 -> 532 rows, 129,568 B;  rise 0.95: 275 -> 551 -> 556 rows, 131,104 B: both fit."""
    assert fused_fit(512, 1.0, 5, 1e-3, 1.0, False) == (15, 1028, 161312, True)
    assert fused_fit(512, 1.0, 5, 1e-3, 0.95, False) == (15, 1084, 164896, False)
    assert fused_fit(512, 1.0, 5, 1e-3, 1.0, True) == (15, 532, 129568, True)
    assert fused_fit(512, 1.0, 5, 1e-3, 0.95, True) == (15, 556, 131104, True)
    check_fused_against_transform(512, 1.0, 1.0, rise_min, 3.0)
