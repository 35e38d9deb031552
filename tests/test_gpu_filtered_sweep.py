"""The sweep on low / high-pass filtered spectra (hh_set_spectrum_filter; lib/transforms.py:771-820, lib/filters.py:314-372)
through the C ABI.

Expected scores come from the oracle alone: E = O.compute_power_spectra(img, apix, cutoff_res, output_size, log, lp, hp)[0],
the same of O.simulate_helical_projection(...) for every candidate, then O.cross_correlation_coefficient(E[mask], P[mask]).
Every comparison is at the project's score tolerance (2e-4 absolute) over EVERY candidate of the grid,
with the arg-max identical (the 512 -> 256 case states its 16 sampled candidates); the several-segment form is held to 2e-6
against single-segment sweeps, as in the zoom test."""
import ctypes as C

import numpy as np
import pytest

import helicon_amd as H
from helicon_amd import _lib
from helicon_amd.grid import build_grid
from oracle import path_b as O

pytestmark = pytest.mark.gpu

SCORE_TOL = 2e-4
TWISTS, RISES = np.arange(25.0, 33.5, 1.0), np.arange(4.0, 8.25, 0.5)
TRUTH = (29.0, 6.0)
FILTERS = [(0.0, 0.05), (0.3, 0.0), (0.3, 0.05)]


def make_image(ny, nx, apix, truth=(29.0, 6.0, 1), seed=3, **geom):
    tw, rs, cs = truth
    d, br = 0.4 * ny * apix, 2 * apix
    clean = O.simulate_helical_projection(1, tw, rs, cs, d, br, 0, 0, ny, nx, apix, **geom)
    return (clean + np.random.default_rng(seed).normal(0, 0.5 * clean.std(), clean.shape)).astype(np.float32), d, br


def oracle_scores(img, params, mask, apix, d, br, cutoff, size, lp, hp, log=True, **geom):
    ny, nx = img.shape
    e = O.compute_power_spectra(np.asarray(img, dtype=np.float64), apix, cutoff, size, log, lp, hp)[0]
    out = []
    for tw, rs, cs, rot in params:
        sim = O.simulate_helical_projection(1, tw, rs, int(cs), d, br, 0, 0, ny, nx, apix, rot=rot, **geom)
        p = O.compute_power_spectra(sim, apix, cutoff, size, log, lp, hp)[0]
        out.append(O.cross_correlation_coefficient(e[mask], p[mask]))
    return np.array(out, dtype=np.float64)


def check(got, ref, what=""):
    """Every candidate at the score tolerance, the arg-max identical."""
    err = np.abs(np.asarray(got, dtype=np.float64) - ref)
    print(f"{what}: max |score - oracle| = {err.max():.3e} over {len(ref)} candidates; "
          f"oracle best / second = {np.sort(ref)[-1]:.3f} / {np.sort(ref)[-2]:.3f}")
    assert got.shape == ref.shape
    np.testing.assert_allclose(got, ref, rtol=0, atol=SCORE_TOL, err_msg=what)
    assert int(np.argmax(got)) == int(np.argmax(ref)), what


def filtered(eng, img, mask, cutoff, size, lp, hp, params, log=True):
    eng.set_zoom(cutoff, size)
    eng.set_filter(lp, hp)
    eng.set_reference(img, mask, log=log)
    out = eng.sweep(params)
    assert eng.last_first_pass == "filtered"
    return out


@pytest.mark.parametrize("lp,hp", FILTERS)
@pytest.mark.parametrize("size", [(48, 48), (45, 63), (45, 64), (64, 45)])   # even, odd and mixed parity: the operator pairs
def test_filtered_zoomed_sweep_finds_the_truth(size, lp, hp):
    ny = nx = 64
    apix, cutoff = 2.0, (8, 8)
    img, d, br = make_image(ny, nx, apix)
    grid = build_grid(TWISTS, RISES, (1,), tube_length=nx * apix)
    mask = O.radial_band_mask(*size)
    with H.SweepEngine((ny, nx)) as eng:
        eng.set_geometry(apix=apix, helical_diameter=d, ball_radius=br)
        got = filtered(eng, img, mask, cutoff, size, lp, hp, grid.params)[0]
        assert np.array_equal(got, eng.sweep(grid.params)[0])          # two identical sweeps are bit-identical
    ref = oracle_scores(img, grid.params, mask, apix, d, br, cutoff, size, lp, hp)
    check(got, ref, f"64x64 -> {size}, lp {lp}, hp {hp}")
    assert tuple(grid.params[int(np.argmax(got)), :2]) == TRUTH         # the truth, as the oracle puts it


@pytest.mark.parametrize("lp,hp,truth", [(0.0, 0.05, True), (0.3, 0.0, False), (0.3, 0.05, False)])
def test_filter_without_a_zoom(lp, hp, truth):
    """Default sampling: the library runs the product kernel at the identity zoom; Python sets no zoom.  With lp = 0.3 the
    oracle itself does not find the truth on this image, so only the equality with its arg-max is asserted there."""
    ny = nx = 64
    apix = 2.0
    img, d, br = make_image(ny, nx, apix)
    grid = build_grid(TWISTS, RISES, (1,), tube_length=nx * apix)
    mask = O.radial_band_mask(ny, nx)
    with H.SweepEngine(ny) as eng:
        eng.set_geometry(apix=apix, helical_diameter=d, ball_radius=br)
        got = filtered(eng, img, mask, None, None, lp, hp, grid.params)[0]
        assert eng._zoom is None and eng.spectrum_shape == (ny, nx)
    check(got, oracle_scores(img, grid.params, mask, apix, d, br, None, None, lp, hp), f"64x64 default sampling, lp {lp}, hp {hp}")
    if truth:
        assert tuple(grid.params[int(np.argmax(got)), :2]) == TRUTH


def test_odd_image_side_without_a_zoom():
    ny, nx, apix = 51, 71, 2.0
    img, d, br = make_image(ny, nx, apix)
    grid = build_grid(TWISTS, RISES, (1,), tube_length=nx * apix)
    mask = O.radial_band_mask(ny, nx)
    with H.SweepEngine((ny, nx)) as eng:
        eng.set_geometry(apix=apix, helical_diameter=d, ball_radius=br)
        for lp, hp in FILTERS:
            got = filtered(eng, img, mask, None, None, lp, hp, grid.params)[0]
            check(got, oracle_scores(img, grid.params, mask, apix, d, br, None, None, lp, hp), f"51x71 no zoom, lp {lp}, hp {hp}")


def test_no_log_and_masks():
    ny = nx = 64
    apix, cutoff, size, lp, hp = 2.0, (8, 8), (48, 48), 0.3, 0.05
    ony = size[0]
    img, d, br = make_image(ny, nx, apix)
    grid = build_grid(TWISTS, RISES, (1,), tube_length=nx * apix)
    band = O.radial_band_mask(*size)
    rnd = np.random.default_rng(5).random(size) < 0.3                   # a seeded random mask: not Friedel-symmetric
    upper = np.zeros(size, dtype=bool)
    upper[: ony // 2] = True          # unshifted rows u >= ony/2 only
    with H.SweepEngine((ny, nx)) as eng:
        eng.set_geometry(apix=apix, helical_diameter=d, ball_radius=br)
        for name, mask in (("random mask", rnd), ("rows u >= ony/2", upper)):
            got = filtered(eng, img, mask, cutoff, size, lp, hp, grid.params)[0]
            check(got, oracle_scores(img, grid.params, mask, apix, d, br, cutoff, size, lp, hp), name)
        got = filtered(eng, img, band, cutoff, size, 0.0, 0.05, grid.params, log=False)[0]
        check(got, oracle_scores(img, grid.params, band, apix, d, br, cutoff, size, 0.0, 0.05, log=False), "log=False")


def test_tilt_psi_dy():
    ny = nx = 64
    apix, cutoff, size, lp, hp = 2.0, (8, 8), (48, 48), 0.0, 0.05
    geom = dict(tilt=5.0, psi=3.0, dy=1.5)
    img, d, br = make_image(ny, nx, apix, **geom)
    grid = build_grid(TWISTS, RISES, (1,), tube_length=nx * apix)
    mask = O.radial_band_mask(*size)
    with H.SweepEngine((ny, nx)) as eng:
        eng.set_geometry(apix=apix, helical_diameter=d, ball_radius=br, **geom)
        got = filtered(eng, img, mask, cutoff, size, lp, hp, grid.params)[0]
    check(got, oracle_scores(img, grid.params, mask, apix, d, br, cutoff, size, lp, hp, **geom), "tilt 5, psi 3, dy 1.5")


def test_csym_3():
    ny = nx = 64
    apix, cutoff, size, lp, hp = 2.0, (8, 8), (45, 63), 0.3, 0.05
    img, d, br = make_image(ny, nx, apix, truth=(29.0, 6.0, 3))
    grid = build_grid(TWISTS, RISES, (3,), tube_length=nx * apix)
    mask = O.radial_band_mask(*size)
    with H.SweepEngine((ny, nx)) as eng:
        eng.set_geometry(apix=apix, helical_diameter=d, ball_radius=br)
        got = filtered(eng, img, mask, cutoff, size, lp, hp, grid.params)[0]
    check(got, oracle_scores(img, grid.params, mask, apix, d, br, cutoff, size, lp, hp), "csym 3")


def test_non_square_even_view_and_three_segments():
    ny, nx, apix, cutoff, size, lp, hp = 64, 96, 2.0, (6, 10), (48, 80), 0.0, 0.05
    imgs = np.stack([make_image(ny, nx, apix, seed=s)[0] for s in range(3)])
    d, br = 0.4 * ny * apix, 2 * apix
    grid = build_grid(TWISTS, RISES, (1,), tube_length=nx * apix)
    mask = O.radial_band_mask(*size)
    with H.SweepEngine((ny, nx)) as eng:
        eng.set_geometry(apix=apix, helical_diameter=d, ball_radius=br)
        multi = filtered(eng, imgs, mask, cutoff, size, lp, hp, grid.params)
        assert multi.shape == (3, len(grid))
        for s in range(3):
            single = filtered(eng, imgs[s], mask, cutoff, size, lp, hp, grid.params)[0]
            np.testing.assert_allclose(multi[s], single, rtol=0, atol=2e-6)
    for s in (0, 2):
        check(multi[s], oracle_scores(imgs[s], grid.params, mask, apix, d, br, cutoff, size, lp, hp), f"64x96 -> 48x80, segment {s} of 3")


def test_filter_off_changes_nothing_and_a_change_drops_the_reference():
    ny = nx = 64
    apix = 2.0
    img, d, br = make_image(ny, nx, apix)
    geom = dict(apix=apix, helical_diameter=d, ball_radius=br)
    grid = build_grid(TWISTS, RISES, (1,), tube_length=nx * apix)
    for cutoff, size in ((None, None), ((8, 8), (48, 48))):
        with H.SweepEngine(ny) as fresh:                                 # an engine that never had a filter
            fresh.set_geometry(**geom)
            fresh.set_zoom(cutoff, size)
            fresh.set_reference(img)
            base = fresh.sweep(grid.params)
            first = fresh.last_first_pass
        assert first == ("zoom" if size else first) and first != "filtered"
        with H.SweepEngine(ny) as eng:
            eng.set_geometry(**geom)
            eng.set_zoom(cutoff, size)
            eng.set_reference(img)
            for lp, hp in ((0, 0), (1.0, 0.0), (0.0, -0.2), (2.0, 1.0)):   # all off: the reference stands, nothing changes
                eng.set_filter(lp, hp)
                assert eng.n_segments == 1
                assert np.array_equal(eng.sweep(grid.params), base) and eng.last_first_pass == first
            f = filtered(eng, img, None, cutoff, size, 0.0, 0.05, grid.params)
            assert not np.array_equal(f, base)
            res = H.sweep(img, TWISTS, RISES, (1,), cutoff_res=cutoff, output_size=size, high_pass_fraction=0.05, engine=eng, **geom)
            assert np.array_equal(res.scores.reshape(-1), f.reshape(-1)) and eng.last_first_pass == "filtered"
            eng.set_filter(0.0, 0.1)                                     # a change of filter drops the reference
            assert eng.n_segments == 0
            with pytest.raises(H.HeliconHipError):
                eng.sweep(grid.params)
            eng.set_filter()                                             # both off: the filter is cleared, a reference is due
            assert eng.n_segments == 0
            with pytest.raises(H.HeliconHipError):
                eng.sweep(grid.params)
            eng.set_reference(img)
            assert np.array_equal(eng.sweep(grid.params), base) and eng.last_first_pass == first
    # the module's shared engine returns to the unfiltered default sweep, bit for bit
    plain = H.sweep(img, TWISTS, RISES, (1,), **geom)
    filt = H.sweep(img, TWISTS, RISES, (1,), high_pass_fraction=0.05, **geom)
    assert not np.array_equal(filt.scores, plain.scores)
    assert np.array_equal(H.sweep(img, TWISTS, RISES, (1,), **geom).scores, plain.scores)
    assert np.array_equal(H.sweep(img, TWISTS, RISES, (1,), low_pass_fraction=1.0, high_pass_fraction=0.0, **geom).scores, plain.scores)


def test_c_abi_refusals_and_memory():
    L = _lib.lib()
    img, d, br = make_image(64, 64, 2.0)
    with H.SweepEngine(64) as eng:
        ctx = eng._ctx
        assert L.hh_set_spectrum_filter(None, 0.3, 0.05) == -1           # HH_ERR_ARG
        for args in ((float("nan"), 0.05), (0.3, float("nan"))):
            assert L.hh_set_spectrum_filter(ctx, *args) == -1, args
            assert b"hh_set_spectrum_filter" in L.hh_last_error(ctx)
        assert L.hh_set_spectrum_filter(ctx, 0.0, 0.0) == 0               # nothing to clear: fine
        assert L.hh_set_spectrum_filter(ctx, 5.0, -1.0) == 0              # outside (0, 1): off
        eng.set_geometry(apix=2.0, helical_diameter=d, ball_radius=br)
        eng.set_reference(img)
        p = np.array([[29.0, 6.0, 1.0, 0.0]])
        out = np.zeros(1, dtype=np.float32)
        before = int(L.hh_memory_bytes(ctx, None))
        assert L.hh_set_spectrum_filter(ctx, 0.0, 0.05) == 0
        # a sweep between the filter and its reference: HH_ERR_STATE
        assert L.hh_sweep(ctx, p.ctypes.data_as(C.POINTER(C.c_double)), 1, out.ctypes.data_as(C.POINTER(C.c_float))) == -3
        eng._filter = (0.0, 0.05)
        eng.set_reference(img)
        got = eng.sweep(p)
        assert eng.last_first_pass == "filtered" and L.hh_last_first_pass(ctx) == 4
        assert int(L.hh_memory_bytes(ctx, None)) > before                 # the filter's buffers are accounted for
        # an empty mask is refused and the filtered reference stands
        with pytest.raises(ValueError):
            eng.set_reference(img, np.zeros((64, 64), dtype=bool))
        assert np.array_equal(eng.sweep(p), got)
        # the same fractions again: no change, the reference stands
        assert L.hh_set_spectrum_filter(ctx, 0.0, 0.05) == 0
        assert np.array_equal(eng.sweep(p), got)


def test_tuned_size_512_to_256_high_pass():
    """The size the feature is for: 512 x 512, cutoff_res = (4 apix, 4 apix), 256 x 256, hp = 0.02; 16 candidates sampled
    across a 4 x 4 twist-major grid around the benchmark workload's truth (1.2 degrees, 4.75 A)."""
    n, apix, size, lp, hp = 512, 1.0, (256, 256), 0.0, 0.02
    cutoff = (4 * apix, 4 * apix)
    img, d, br = make_image(n, n, apix, truth=(1.2, 4.75, 1), seed=0)
    grid = build_grid(np.array([0.9, 1.2, 1.3, 2.0]), np.array([4.6, 4.75, 4.9, 6.0]), (1,), tube_length=n * apix)
    assert len(grid) == 16
    mask = O.radial_band_mask(*size)
    with H.SweepEngine(n) as eng:
        eng.set_geometry(apix=apix, helical_diameter=d, ball_radius=br)
        got = filtered(eng, img, mask, cutoff, size, lp, hp, grid.params)[0]
    check(got, oracle_scores(img, grid.params, mask, apix, d, br, cutoff, size, lp, hp), "512 -> 256, hp 0.02")
