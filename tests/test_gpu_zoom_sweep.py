"""The sweep on Fourier-zoomed spectra (hh_set_spectrum_zoom; lib/transforms.py:663-713, 771-820) through the C ABI.

Expected scores come from the oracle alone: E = O.compute_power_spectra(img, apix, cutoff_res, output_size)[0], the same of
O.simulate_helical_projection(...) for every candidate, then O.cross_correlation_coefficient(E[mask], P[mask]).  Every
comparison is at the project's score tolerance (2e-4 absolute) over EVERY candidate, with the arg-max
identical; the device's pipelines are held to 2e-5 among themselves and the several-segment form to 2e-6, as elsewhere in
the suite."""
import ctypes as C

import numpy as np
import pytest

import helicon_amd as H
from helicon_amd import _lib
from helicon_amd.grid import build_grid
from oracle import path_b as O

pytestmark = pytest.mark.gpu

SCORE_TOL = 2e-4

TWISTS, RISES = np.arange(25.0, 33.5, 1.0), np.arange(8.0, 12.5, 1.0)


def make_image(ny, nx, apix, truth=(29.0, 10.0, 1), seed=0, **geom):
    tw, rs, cs = truth
    d, br = 0.4 * ny * apix, 2 * apix
    clean = O.simulate_helical_projection(1, tw, rs, cs, d, br, 0, 0, ny, nx, apix, **geom)
    return (clean + np.random.default_rng(seed).normal(0, 0.5 * clean.std(), clean.shape)).astype(np.float32), d, br


def oracle_spectra(params, shape, apix, d, br, cutoff, size, log=True, **geom):
    ny, nx = shape
    out = []
    for tw, rs, cs, rot in params:
        sim = O.simulate_helical_projection(1, tw, rs, int(cs), d, br, 0, 0, ny, nx, apix, rot=rot, **geom)
        out.append(O.compute_power_spectra(sim, apix, cutoff, size, log=log)[0])
    return out


def oracle_scores(img, params, mask, apix, d, br, cutoff, size, log=True, spectra=None, **geom):
    e = O.compute_power_spectra(np.asarray(img, dtype=np.float64), apix, cutoff, size, log=log)[0]
    if spectra is None:
        spectra = oracle_spectra(params, img.shape, apix, d, br, cutoff, size, log=log, **geom)
    return np.array([O.cross_correlation_coefficient(e[mask], p[mask]) for p in spectra], dtype=np.float64)


def check(got, ref, what=""):
    """Every candidate at the score tolerance, the arg-max identical."""
    err = np.abs(np.asarray(got, dtype=np.float64) - ref)
    print(f"{what}: max |score - oracle| = {err.max():.3e} over {len(ref)} candidates; "
          f"oracle gap to the runner-up = {np.sort(ref)[-1] - np.sort(ref)[-2]:.3f}")
    assert got.shape == ref.shape
    np.testing.assert_allclose(got, ref, rtol=0, atol=SCORE_TOL, err_msg=what)
    assert int(np.argmax(got)) == int(np.argmax(ref)), what


def zoomed(eng, img, mask, cutoff, size, params, log=True):
    eng.set_zoom(cutoff, size)
    eng.set_reference(img, mask, log=log)
    out = eng.sweep(params)
    assert eng.last_first_pass == "zoom"
    return out


@pytest.mark.parametrize("ny,nx,cutoff,size,geom", [
    (64, 64, (8, 8), (64, 64), {}),
    (64, 64, (8, 8), (32, 32), {}),
    (64, 96, (6, 10), (48, 80), {}),
    (50, 70, (7, 9), (45, 63), {}),                                   # odd spectrum sides: no unpaired row / column
    (64, 64, (8, 8), (64, 64), dict(tilt=5.0, psi=3.0, dy=1.5)),
])
def test_zoomed_sweep_against_oracle(ny, nx, cutoff, size, geom):
    apix = 2.0
    img, d, br = make_image(ny, nx, apix, **geom)
    grid = build_grid(TWISTS, RISES, (1,), tube_length=nx * apix)
    mask = O.radial_band_mask(*size)
    with H.SweepEngine((ny, nx)) as eng:
        eng.set_geometry(apix=apix, helical_diameter=d, ball_radius=br, **geom)
        got = zoomed(eng, img, mask, cutoff, size, grid.params)[0]
        assert np.array_equal(got, eng.sweep(grid.params)[0])          # two identical sweeps are bit-identical
        # the default mask is the radial band of the zoomed plane
        eng.set_reference(img)
        assert np.array_equal(got, eng.sweep(grid.params)[0])
    ref = oracle_scores(img, grid.params, mask, apix, d, br, cutoff, size, **geom)
    check(got, ref, f"{ny}x{nx} -> {size} {geom}")
    assert tuple(grid.params[int(np.argmax(got)), :2]) == (29.0, 10.0)   # the truth, as the oracle puts it


def test_csym_3_on_odd_sides():
    ny, nx, apix, cutoff, size = 50, 70, 2.0, (7, 9), (45, 63)
    img, d, br = make_image(ny, nx, apix, truth=(29.0, 10.0, 3))
    grid = build_grid(TWISTS, RISES, (3,), tube_length=nx * apix)
    mask = O.radial_band_mask(*size)
    with H.SweepEngine((ny, nx)) as eng:
        eng.set_geometry(apix=apix, helical_diameter=d, ball_radius=br)
        got = zoomed(eng, img, mask, cutoff, size, grid.params)[0]
    check(got, oracle_scores(img, grid.params, mask, apix, d, br, cutoff, size), "csym 3")


def test_small_rises_take_more_than_one_k_slice():
    """Rises 1.5, 2, 3 A on 64 x 128: up to 343 lattice centres per candidate, several K slices and two centre chunks."""
    ny, nx, apix, cutoff, size = 64, 128, 2.0, (8, 8), (40, 100)
    img, d, br = make_image(ny, nx, apix, truth=(29.0, 2.0, 1))
    grid = build_grid(TWISTS, np.array([1.5, 2.0, 3.0]), (1,), tube_length=nx * apix)
    mask = O.radial_band_mask(*size)
    with H.SweepEngine((ny, nx)) as eng:
        eng.set_geometry(apix=apix, helical_diameter=d, ball_radius=br)
        got = zoomed(eng, img, mask, cutoff, size, grid.params)[0]
    check(got, oracle_scores(img, grid.params, mask, apix, d, br, cutoff, size), "rises 1.5 - 3")


def test_no_log_masks_order_and_skipped_candidates():
    ny, nx, apix, cutoff, size = 64, 64, 2.0, (8, 8), (64, 64)
    ony, onx = size
    img, d, br = make_image(ny, nx, apix)
    grid = build_grid(TWISTS, RISES, (1,), tube_length=nx * apix)
    band = O.radial_band_mask(*size)
    rnd = np.random.default_rng(5).random(size) < 0.3                   # a seeded random mask: not Friedel-symmetric
    upper = np.zeros(size, dtype=bool)
    upper[: ony // 2] = True          # unshifted rows u >= ony/2 only: the unpaired row (fftshifted row 0) and column 0
    spectra = oracle_spectra(grid.params, (ny, nx), apix, d, br, cutoff, size)
    with H.SweepEngine((ny, nx)) as eng:
        eng.set_geometry(apix=apix, helical_diameter=d, ball_radius=br)
        for name, mask in (("random mask", rnd), ("rows u >= ony/2", upper), ("band, rows u >= ony/2", band & upper)):
            got = zoomed(eng, img, mask, cutoff, size, grid.params)[0]
            check(got, oracle_scores(img, grid.params, mask, apix, d, br, cutoff, size, spectra=spectra), name)
        got_nolog = zoomed(eng, img, band, cutoff, size, grid.params, log=False)[0]
        check(got_nolog, oracle_scores(img, grid.params, band, apix, d, br, cutoff, size, log=False), "log=False")
        # a shuffled list gives every candidate the score of the ordered one
        got = zoomed(eng, img, band, cutoff, size, grid.params)[0]
        perm = np.random.default_rng(0).permutation(len(grid))
        np.testing.assert_allclose(eng.sweep(grid.params[perm])[0], got[perm], rtol=0, atol=2e-5)
        # the device entry point, with and without the host mirror of the list and with a row stride
        import torch

        dp = torch.as_tensor(grid.params, device="cuda")
        ds = torch.full((len(grid) + 7,), -2.0, dtype=torch.float32, device="cuda")
        eng.sweep_device(dp.data_ptr(), len(grid), ds.data_ptr())
        eng.synchronize()
        assert np.array_equal(ds[: len(grid)].cpu().numpy(), got) and float(ds[len(grid)]) == -2.0
        ds.fill_(-2.0)
        eng.sweep_device(dp.data_ptr(), len(grid), ds.data_ptr(), host_params=grid.params, ld_scores=len(grid) + 7)
        eng.synchronize()
        assert np.array_equal(ds[: len(grid)].cpu().numpy(), got) and eng.last_first_pass == "zoom"
        # an empty lattice (rise <= 0) scores 0, as in the default sweep (analysis.py:796-797)
        holes = grid.params.copy()
        holes[3, 1] = -1.0
        holes[11, 1] = float("nan")
        sc = eng.sweep(holes)[0]
        assert sc[3] == 0.0 and sc[11] == 0.0
        keep = np.ones(len(grid), dtype=bool)
        keep[[3, 11]] = False
        assert np.array_equal(sc[keep], got[keep])
    # the grid's valid = False candidates come back as -inf from sweep(), zoomed or not
    res = H.sweep(img, np.array([0.0, 29.0]), np.array([10.0, 70.0]), (1,), apix=apix, helical_diameter=d, ball_radius=br,
                  cutoff_res=cutoff, output_size=size)
    plain = H.sweep(img, np.array([0.0, 29.0]), np.array([10.0, 70.0]), (1,), apix=apix, helical_diameter=d, ball_radius=br)
    assert not res.grid.valid[[0, 1, 3]].any() and res.grid.valid[2]
    assert np.array_equal(np.isneginf(res.scores), np.isneginf(plain.scores))
    assert np.isneginf(res.scores.reshape(-1)[[0, 1, 3]]).all() and int(res.best_index[0]) == 2
    ref = oracle_scores(img, res.grid.params[2:3], band, apix, d, br, cutoff, size)
    assert abs(float(res.scores.reshape(-1)[2]) - ref[0]) < SCORE_TOL


def test_three_segments_equal_three_single_sweeps():
    ny, nx, apix, cutoff, size = 64, 96, 2.0, (6, 10), (48, 80)
    imgs = np.stack([make_image(ny, nx, apix, seed=s)[0] for s in range(3)])
    d, br = 0.4 * ny * apix, 2 * apix
    grid = build_grid(TWISTS, RISES, (1,), tube_length=nx * apix)
    mask = np.random.default_rng(2).random(size) < 0.5
    with H.SweepEngine((ny, nx)) as eng:
        eng.set_geometry(apix=apix, helical_diameter=d, ball_radius=br)
        multi = zoomed(eng, imgs, mask, cutoff, size, grid.params)
        assert multi.shape == (3, len(grid))
        for s in range(3):
            single = zoomed(eng, imgs[s], mask, cutoff, size, grid.params)[0]
            np.testing.assert_allclose(multi[s], single, rtol=0, atol=2e-6)
    check(multi[2], oracle_scores(imgs[2], grid.params, mask, apix, d, br, cutoff, size), "segment 2 of 3")


def test_footprints_wider_than_the_lds_profiles():
    """A ball radius of 7 pixels: 71-pixel footprints, past the 64 taps whose profiles the kernel keeps in LDS."""
    ny, nx, apix, cutoff, size = 64, 64, 2.0, (8, 8), (32, 32)
    d, br = 0.4 * ny * apix, 7 * apix
    clean = O.simulate_helical_projection(1, 29.0, 10.0, 1, d, br, 0, 0, ny, nx, apix)
    img = (clean + np.random.default_rng(0).normal(0, 0.5 * clean.std(), clean.shape)).astype(np.float32)
    grid = build_grid(TWISTS[::2], RISES, (1,), tube_length=nx * apix)
    mask = O.radial_band_mask(*size)
    with H.SweepEngine((ny, nx)) as eng:
        eng.set_geometry(apix=apix, helical_diameter=d, ball_radius=br)
        got = zoomed(eng, img, mask, cutoff, size, grid.params)[0]
    check(got, oracle_scores(img, grid.params, mask, apix, d, br, cutoff, size), "ball radius 7 px")


def test_tuned_size_512_to_256():
    """512 x 512 (a tuned context), cutoff_res = (4 apix, 4 apix), 256 x 256: eight candidates of a twist-major grid around
    the benchmark workload's truth (1.2 degrees, 4.75 A), under the radial band, a seeded 30 % random mask and the band's
    rows u >= ony/2 alone."""
    n, apix, size = 512, 1.0, (256, 256)
    cutoff = (4 * apix, 4 * apix)
    img, d, br = make_image(n, n, apix, truth=(1.2, 4.75, 1))
    grid = build_grid(np.array([0.9, 1.2, 1.3, 2.0]), np.array([4.6, 4.75, 4.9, 6.0]), (1,), tube_length=n * apix)
    pick = [0 * 4 + 1, 0 * 4 + 3, 1 * 4 + 0, 1 * 4 + 1, 1 * 4 + 2, 2 * 4 + 1, 3 * 4 + 0, 3 * 4 + 3]   # twist-major order kept
    params = grid.params[pick]
    truth = pick.index(1 * 4 + 1)
    band = O.radial_band_mask(*size)
    rnd = np.random.default_rng(7).random(size) < 0.3
    upper = band.copy()
    upper[size[0] // 2:] = False
    spectra = oracle_spectra(params, (n, n), apix, d, br, cutoff, size)
    with H.SweepEngine(n) as eng:
        assert not eng.general
        eng.set_geometry(apix=apix, helical_diameter=d, ball_radius=br)
        for name, mask in (("band", band), ("random 30 %", rnd), ("band, rows u >= ony/2", upper)):
            got = zoomed(eng, img, mask, cutoff, size, params)[0]
            ref = oracle_scores(img, params, mask, apix, d, br, cutoff, size, spectra=spectra)
            check(got, ref, f"512 -> 256, {name}")
            assert int(np.argmax(got)) == truth and np.sort(ref)[-1] - np.sort(ref)[-2] >= 0.07


def test_default_sampling_arguments_change_nothing_and_clearing_restores():
    ny, nx, apix = 64, 64, 2.0
    img, d, br = make_image(ny, nx, apix)
    geom = dict(apix=apix, helical_diameter=d, ball_radius=br)
    plain = H.sweep(img, TWISTS, RISES, (1,), **geom)
    grid = plain.grid
    with H.SweepEngine(ny) as eng:
        eng.set_geometry(**geom)
        eng.set_reference(img)
        base = eng.sweep(grid.params)
        first = eng.last_first_pass
        assert first != "zoom" and np.array_equal(base.reshape(-1), plain.scores.reshape(-1))
        for cutoff, size in ((None, None), ((2 * apix, 2 * apix), None), (None, (ny, nx)), ((2 * apix, 2 * apix), (ny, nx))):
            eng.set_zoom(cutoff, size)
            assert eng.n_segments == 1                                 # the reference stands: nothing was called
            assert np.array_equal(eng.sweep(grid.params), base) and eng.last_first_pass == first
            res = H.sweep(img, TWISTS, RISES, (1,), cutoff_res=cutoff, output_size=size, engine=eng, **geom)
            assert np.array_equal(res.scores, plain.scores) and eng.last_first_pass == first
        # a zoomed sweep, then the default sampling again on the same engine
        z = zoomed(eng, img, None, (8, 8), (32, 32), grid.params)
        assert not np.array_equal(z, base)
        eng.set_zoom()
        assert eng.n_segments == 0
        with pytest.raises(H.HeliconHipError):                         # HH_ERR_STATE: the zoomed reference is gone
            eng.sweep(grid.params)
        eng.set_reference(img)
        assert np.array_equal(eng.sweep(grid.params), base) and eng.last_first_pass == first
    # the same on a general-size context
    ny, nx = 50, 70
    img, d, br = make_image(ny, nx, apix)
    geom = dict(apix=apix, helical_diameter=d, ball_radius=br)
    grid = build_grid(TWISTS, RISES, (1,), tube_length=nx * apix)
    with H.SweepEngine((ny, nx)) as eng:
        eng.set_geometry(**geom)
        eng.set_reference(img)
        base = eng.sweep(grid.params)
        first = eng.last_first_pass
        zoomed(eng, img, None, (7, 9), (45, 63), grid.params)
        eng.set_zoom(None, (ny, nx))
        eng.set_reference(img)
        assert np.array_equal(eng.sweep(grid.params), base) and eng.last_first_pass == first


def test_c_abi_refusals():
    L = _lib.lib()
    img, d, br = make_image(64, 64, 2.0)
    with H.SweepEngine(64) as eng:
        ctx = eng._ctx
        for args in ((7, 64, 8.0, 8.0), (64, 1025, 8.0, 8.0), (64, 64, 0.0, 8.0), (64, 64, 8.0, -1.0), (0, 0, 8.0, 8.0),
                     (64, 64, float("nan"), 8.0), (64, 64, 8.0, float("inf")), (-8, 64, 8.0, 8.0)):
            assert L.hh_set_spectrum_zoom(ctx, *args) == -1, args        # HH_ERR_ARG
            assert b"hh_set_spectrum_zoom" in L.hh_last_error(ctx)
        assert L.hh_set_spectrum_zoom(None, 64, 64, 8.0, 8.0) == -1
        assert L.hh_set_spectrum_zoom(ctx, 0, 0, 0.0, 0.0) == 0            # nothing to clear: fine
        # a zoom before the geometry: the reference cannot be prepared (the frequencies need the pixel size)
        assert L.hh_set_spectrum_zoom(ctx, 32, 32, 8.0, 8.0) == 0
        m = np.ones((32, 32), dtype=np.uint8)
        assert L.hh_set_reference(ctx, img.ctypes.data_as(C.POINTER(C.c_float)), 1, m.ctypes.data_as(C.POINTER(C.c_uint8)), 1) == -3
        eng.set_geometry(apix=2.0, helical_diameter=d, ball_radius=br)
        # a sweep between the zoom and its reference: HH_ERR_STATE, also when a default reference was there before
        out = np.zeros(1, dtype=np.float32)
        p = np.array([[29.0, 10.0, 1.0, 0.0]])
        assert L.hh_sweep(ctx, p.ctypes.data_as(C.POINTER(C.c_double)), 1, out.ctypes.data_as(C.POINTER(C.c_float))) == -3
        # an empty mask is refused and an earlier zoomed reference stands
        eng._zoom = (32, 32, 8.0, 8.0)
        eng.set_reference(img)
        before = eng.sweep(p)
        with pytest.raises(ValueError):
            eng.set_reference(img, np.zeros((32, 32), dtype=bool))
        assert np.array_equal(eng.sweep(p), before)
        with pytest.raises(ValueError):                                     # the mask lives on the zoomed plane
            eng.set_reference(img, np.ones((64, 64), dtype=bool))
        # another pixel size changes the frequencies: the reference is dropped
        eng.set_geometry(apix=2.5, helical_diameter=d, ball_radius=br)
        assert eng.n_segments == 0
        assert L.hh_sweep(ctx, p.ctypes.data_as(C.POINTER(C.c_double)), 1, out.ctypes.data_as(C.POINTER(C.c_float))) == -3
