"""The sweep's phase score across the meridian (hh_set_spectrum_phase, hh_sweep_parts, hh_phase_map) through the C ABI.

Expected values come from tests/phase_oracle.py alone (float64 NumPy: centre-origin DFT matrices, M = q c, cosine
similarity; the amplitude part from oracle.path_b).  The amplitude and the phase score of EVERY candidate are held to the
suite's score tolerance (2e-4 absolute) with identical arg-max; the float32 floor of the phase score,
emulated with complex64 products, is 1.2e-7.  Among the device's own results: the combined score to 1e-6, the
several-segment form to 2e-6, two identical sweeps bit for bit.

Measured on an MI355X (every test prints its figures): largest |score - oracle| 4.4e-7 for the amplitude and 2.7e-7 for the
phase score under the band and random masks, 1.1e-6 for the phase score under the 29 bins of row u = ony/2 alone;
|score - mix| 3e-8; phase_map 4e-8 of max|M| and 3e-8 in c."""
import ctypes as C
import functools

import numpy as np
import pytest

import helicon_amd as H
from helicon_amd import _lib
from helicon_amd import denovo3D as D
from helicon_amd.grid import build_grid
from oracle import path_b as O

from tests import phase_oracle as P

pytestmark = pytest.mark.gpu

SCORE_TOL = 2e-4
TWISTS, RISES = np.arange(25.0, 33.5, 1.0), np.arange(8.0, 12.5, 1.0)


def make_image(ny, nx, apix, truth=(29.0, 10.0, 1), seed=0, br_px=2, **geom):
    tw, rs, cs = truth
    d, br = 0.4 * ny * apix, br_px * apix
    clean = O.simulate_helical_projection(1, tw, rs, cs, d, br, 0, 0, ny, nx, apix, **geom)
    return (clean + np.random.default_rng(seed).normal(0, 0.5 * clean.std(), clean.shape)).astype(np.float32), d, br


def check(got, ref, what):
    """Every candidate at the score tolerance, the arg-max identical."""
    err = np.abs(np.asarray(got, dtype=np.float64) - ref)
    print(f"{what}: max |score - oracle| = {err.max():.3e} over {len(ref)} candidates; "
          f"oracle gap to the runner-up = {np.sort(ref)[-1] - np.sort(ref)[-2]:.4f}")
    assert got.shape == ref.shape
    np.testing.assert_allclose(got, ref, rtol=0, atol=SCORE_TOL, err_msg=what)
    assert int(np.argmax(got)) == int(np.argmax(ref)), what


def parts(eng, img, mask, cutoff, size, params, weight=0.5, log=True):
    eng.set_zoom(cutoff, size)
    eng.set_phase_score(weight)
    eng.set_reference(img, mask, log=log)
    out = eng.sweep_parts(params)
    assert eng.last_first_pass == "phase"
    return out


def against_oracle(ny, nx, cutoff, size, mask, twists=TWISTS, rises=RISES, csym=1, log=True, br_px=2, truth=None, what="", **geom):
    apix = 2.0
    img, d, br = make_image(ny, nx, apix, truth=truth or (29.0, 10.0, csym), br_px=br_px, **geom)
    grid = build_grid(twists, rises, (csym,), tube_length=nx * apix)
    with H.SweepEngine((ny, nx)) as eng:
        eng.set_geometry(apix=apix, helical_diameter=d, ball_radius=br, **geom)
        sc, amp, ph = parts(eng, img, mask, cutoff, size, grid.params, log=log)
        again = eng.sweep_parts(grid.params)
        assert all(np.array_equal(x, y) for x, y in zip((sc, amp, ph), again))          # two sweeps are bit-identical
        assert np.array_equal(eng.sweep(grid.params), sc)                                # hh_sweep writes the combined score
    ref_amp, ref_ph = P.scores(img, grid.params, mask, apix, d, br, cutoff, size, log=log, **geom)
    check(amp[0], ref_amp, f"{what}: amplitude")
    check(ph[0], ref_ph, f"{what}: phase")
    return grid, ph[0], ref_ph


@pytest.mark.parametrize("ny,nx,cutoff,size,geom", [
    (64, 64, None, None, {}),                                          # the identity zoom: the mode without a zoom
    (64, 64, (8, 8), (32, 32), {}),
    (64, 96, (6, 10), (48, 80), {}),
    (50, 70, (7, 9), (45, 63), {}),                                    # odd sides
    (64, 64, None, None, dict(tilt=5.0, psi=3.0, dy=1.5)),
])
def test_parts_against_oracle(ny, nx, cutoff, size, geom):
    mask = O.radial_band_mask(*(size or (ny, nx)))
    grid, ph, ref_ph = against_oracle(ny, nx, cutoff, size, mask, what=f"{ny}x{nx} -> {size} {geom}", **geom)
    assert tuple(grid.params[int(np.argmax(ph)), :2]) == (29.0, 10.0)  # the truth, as the oracle puts it


def test_small_rises_take_more_than_one_k_slice():
    """Rises 1.5, 2, 3 A on 64 x 128: up to 343 lattice centres per candidate, several K slices and two centre chunks."""
    size = (40, 100)
    against_oracle(64, 128, (8, 8), size, O.radial_band_mask(*size), rises=np.array([1.5, 2.0, 3.0]), truth=(29.0, 2.0, 1),
                   what="rises 1.5 - 3")


def test_no_log():
    against_oracle(64, 64, (8, 8), (64, 64), O.radial_band_mask(64, 64), log=False, what="log=False")


def test_random_mask_with_the_unpaired_row_of_a_zoomed_plane():
    """Fftshifted row 0 is u = ony/2, whose partner -f_y is off the zoomed grid: F~ comes from the conjugate factors."""
    size = (32, 32)
    mask = np.random.default_rng(5).random(size) < 0.3
    mask[0, :] = True
    against_oracle(64, 64, (8, 8), size, mask, what="random mask + row u = ony/2")
    only = np.zeros(size, dtype=bool)
    only[0, 3:] = True
    against_oracle(64, 64, (8, 8), size, only, what="row u = ony/2 alone")


def test_csym_3_on_odd_sides():
    size = (45, 63)
    against_oracle(50, 70, (7, 9), size, O.radial_band_mask(*size), csym=3, what="csym 3")


def test_footprints_wider_than_the_lds_profiles():
    """A ball radius of 7 pixels: 71-pixel footprints, past the 64 taps whose profiles the kernel keeps in LDS."""
    size = (32, 32)
    against_oracle(64, 64, (8, 8), size, O.radial_band_mask(*size), twists=TWISTS[::2], br_px=7, what="ball radius 7 px")


def test_combined_score_weight_and_segments():
    ny, nx, apix, cutoff, size = 64, 96, 2.0, (6, 10), (48, 80)
    imgs = np.stack([make_image(ny, nx, apix, seed=s)[0] for s in range(3)])
    d, br = 0.4 * ny * apix, 2 * apix
    grid = build_grid(TWISTS, RISES, (1,), tube_length=nx * apix)
    mask = np.random.default_rng(2).random(size) < 0.5
    with H.SweepEngine((ny, nx)) as eng:
        eng.set_geometry(apix=apix, helical_diameter=d, ball_radius=br)
        multi = parts(eng, imgs, mask, cutoff, size, grid.params, weight=0.25)
        assert all(x.shape == (3, len(grid)) for x in multi)
        for w in (0.25, 1.0):
            eng.set_phase_score(w)
            assert eng.n_segments == 3                                  # changing only the weight keeps the reference
            sc, amp, ph = eng.sweep_parts(grid.params)
            assert np.array_equal(amp, multi[1]) and np.array_equal(ph, multi[2])
            mix = (1 - w) * amp.astype(np.float64) + w * ph.astype(np.float64)
            print(f"w = {w}: max |score - mix| = {np.abs(sc - mix).max():.2e}")
            np.testing.assert_allclose(sc, mix, rtol=0, atol=1e-6)
            assert np.array_equal(eng.sweep(grid.params), sc)
        assert np.array_equal(sc, ph)                                   # w = 1: the phase score alone
        for s in range(3):
            single = parts(eng, imgs[s], mask, cutoff, size, grid.params, weight=0.25)
            for a, b in zip(multi, single):
                np.testing.assert_allclose(a[s], b[0], rtol=0, atol=2e-6)
    ref_amp, ref_ph = P.scores(imgs[2], grid.params, mask, apix, d, br, cutoff, size)
    check(multi[1][2], ref_amp, "segment 2 of 3: amplitude")
    check(multi[2][2], ref_ph, "segment 2 of 3: phase")


@pytest.mark.parametrize("cutoff,size,log", [(None, None, True), ((6, 10), (48, 80), True), ((7, 9), (33, 47), False)])
def test_phase_map_against_oracle(cutoff, size, log):
    ny, nx, apix = 64, 96, 2.0
    img, d, br = make_image(ny, nx, apix)
    with H.SweepEngine((ny, nx)) as eng:
        eng.set_geometry(apix=apix, helical_diameter=d, ball_radius=br)
        eng.set_zoom(cutoff, size)
        m, c = eng.phase_map(img, log=log)
    rm, rc, ra = P.phase_map(img, apix, cutoff, size, log=log)
    assert m.shape == rm.shape == (size or (ny, nx))
    strong = ra > 1e-3 * ra.max()
    print(f"{size} log={log}: max |M - oracle| / max |M| = {np.abs(m - rm).max() / np.abs(rm).max():.2e}; "
          f"max |c - oracle| on {strong.mean():.0%} of the bins = {np.abs(c - rc)[strong].max():.2e}")
    np.testing.assert_allclose(m, rm, rtol=0, atol=1e-5 * np.abs(rm).max())
    np.testing.assert_allclose(c[strong], rc[strong], rtol=0, atol=1e-5)


@functools.lru_cache(maxsize=None)
def _table_case():
    """The issue's case: amplitudes pick a wrong candidate on a noisy, azimuthally rotated, axially shifted image."""
    n, apix = 128, 2.0
    d, br = 0.4 * n * apix, 2 * apix
    clean = np.roll(O.simulate_helical_projection(1, 29.0, 10.0, 1, d, br, 0, 0, n, n, apix, rot=40), 5, axis=1)
    img = (clean + np.random.default_rng(0).normal(0, 0.5 * clean.std(), clean.shape)).astype(np.float32)
    grid = build_grid(np.arange(28.0, 32.01, 0.5), np.array([10.0, 11.0]), (1,), tube_length=n * apix)
    mask = O.radial_band_mask(n, n)
    return img, d, br, grid, mask, P.scores(img, grid.params, mask, apix, d, br)


def test_phase_score_finds_the_truth_where_amplitudes_do_not():
    img, d, br, grid, mask, (ref_amp, ref_ph) = _table_case()
    assert len(grid) == 18
    with H.SweepEngine(128) as eng:
        eng.set_geometry(apix=2.0, helical_diameter=d, ball_radius=br)
        sc, amp, ph = parts(eng, img, mask, None, None, grid.params, weight=0.5)
    at = lambda s: tuple(grid.params[int(np.argmax(s)), :2])   # noqa: E731
    print(f"amplitude: {at(amp[0])} {amp[0].max():.4f} (truth {amp[0][int(np.argmax(ph[0]))]:.4f}); phase: {at(ph[0])} {ph[0].max():.4f} "
          f"(runner-up {np.sort(ph[0])[-2]:.4f}); w = 0.5: {at(sc[0])}, margin {np.sort(sc[0])[-1] - np.sort(sc[0])[-2]:.4f}")
    check(amp[0], ref_amp, "table case: amplitude")
    check(ph[0], ref_ph, "table case: phase")
    assert at(ref_amp) == (31.5, 11.0) and at(amp[0]) == (31.5, 11.0)                  # wrong
    assert at(ref_ph) == (29.0, 10.0) and at(ph[0]) == (29.0, 10.0)                    # the truth
    assert at(0.5 * ref_amp + 0.5 * ref_ph) == (29.0, 10.0) and at(sc[0]) == (29.0, 10.0)


def test_sweep_argument_and_mode_off_change_nothing():
    ny, nx, apix = 64, 64, 2.0
    img, d, br = make_image(ny, nx, apix)
    geom = dict(apix=apix, helical_diameter=d, ball_radius=br)
    plain = H.sweep(img, TWISTS, RISES, (1,), **geom)
    assert np.array_equal(H.sweep(img, TWISTS, RISES, (1,), phase_weight=0.0, **geom).scores, plain.scores)
    grid = plain.grid
    L = _lib.lib()
    p = np.ascontiguousarray(grid.params)
    out = np.zeros(len(grid), dtype=np.float32)
    pp, po = p.ctypes.data_as(C.POINTER(C.c_double)), out.ctypes.data_as(C.POINTER(C.c_float))
    with H.SweepEngine(ny) as eng:
        eng.set_geometry(**geom)
        eng.set_reference(img)
        base = eng.sweep(grid.params)
        first = eng.last_first_pass
        assert np.array_equal(base.reshape(-1), plain.scores.reshape(-1))
        assert L.hh_sweep_parts(eng._ctx, pp, len(grid), po, None, None) == -3          # HH_ERR_STATE: the mode is off
        eng.set_phase_score(0)                                                           # off and never on: nothing happens
        assert eng.n_segments == 1 and np.array_equal(eng.sweep(grid.params), base) and eng.last_first_pass == first
        # through sweep(): the combined score of the engine, and the shared engines come back without the mode
        res = H.sweep(img, TWISTS, RISES, (1,), phase_weight=0.5, engine=eng, **geom)
        assert eng.last_first_pass == "phase" and eng._phase == 0.5
        sc, amp, ph = eng.sweep_parts(grid.params)
        assert np.array_equal(res.scores.reshape(-1), sc[0]) and not np.array_equal(sc[0], base[0])
        shared = H.sweep(img, TWISTS, RISES, (1,), phase_weight=0.5, **geom)
        assert np.array_equal(shared.scores, res.scores) and D._engine((ny, nx), 0)._phase is None
        assert np.array_equal(H.sweep(img, TWISTS, RISES, (1,), **geom).scores, plain.scores)
        # the caller's engine keeps the mode, so a sweep without it clears it first
        res = H.sweep(img, TWISTS, RISES, (1,), engine=eng, **geom)
        assert eng._phase is None and np.array_equal(res.scores, plain.scores) and eng.last_first_pass == first


def test_c_abi_refusals_and_state():
    L = _lib.lib()
    img, d, br = make_image(64, 64, 2.0)
    p = np.array([[29.0, 10.0, 1.0, 0.0], [30.0, 10.0, 1.0, 0.0]])
    out = np.zeros(2, dtype=np.float32)
    pp, po = p.ctypes.data_as(C.POINTER(C.c_double)), out.ctypes.data_as(C.POINTER(C.c_float))
    with H.SweepEngine(64) as eng:
        ctx = eng._ctx
        eng.set_geometry(apix=2.0, helical_diameter=d, ball_radius=br)
        eng.set_reference(img)
        base = eng.sweep(p)
        for w in (float("nan"), -0.1, 1.5, float("inf")):
            assert L.hh_set_spectrum_phase(ctx, w) == -1, w                              # HH_ERR_ARG, nothing changes
            assert b"hh_set_spectrum_phase" in L.hh_last_error(ctx)
            assert np.array_equal(eng.sweep(p), base)
            with pytest.raises(ValueError):
                eng.set_phase_score(w)
        assert L.hh_set_spectrum_phase(ctx, 0.0) == 0                                    # nothing to clear: the reference stands
        assert np.array_equal(eng.sweep(p), base)
        # switching the mode on drops the reference
        assert L.hh_set_spectrum_phase(ctx, 0.5) == 0
        assert L.hh_sweep(ctx, pp, 2, po) == -3 and L.hh_sweep_parts(ctx, pp, 2, po, None, None) == -3
        eng._phase, eng.n_segments = 0.5, 0
        eng.set_reference(img)
        mixed = eng.sweep(p)
        assert eng.last_first_pass == "phase" and not np.array_equal(mixed, base)
        # a filter after the mode is refused and changes nothing; fractions that are off are no filter
        assert L.hh_set_spectrum_filter(ctx, 0.3, 0.0) == -1
        assert b"hh_set_spectrum_filter" in L.hh_last_error(ctx)
        assert L.hh_set_spectrum_filter(ctx, 0.0, 1.5) == 0
        assert np.array_equal(eng.sweep(p), mixed)
        with pytest.raises(ValueError):
            eng.set_filter(0.3, 0)
        assert eng._filter is None
        # any output of hh_sweep_parts may be NULL
        ph = np.zeros(2, dtype=np.float32)
        assert L.hh_sweep_parts(ctx, pp, 2, None, None, ph.ctypes.data_as(C.POINTER(C.c_float))) == 0
        assert np.array_equal(ph, eng.sweep_parts(p)[2][0])
        # switching it off drops the reference too; afterwards the sweep is the one that never heard of the mode
        eng.set_phase_score(0)
        assert eng.n_segments == 0 and L.hh_sweep(ctx, pp, 2, po) == -3
        eng.set_reference(img)
        assert np.array_equal(eng.sweep(p), base) and eng.last_first_pass != "phase"
        # the mode after a filter is refused and changes nothing
        eng.set_filter(0.3, 0)
        eng.set_reference(img)
        filtered = eng.sweep(p)
        assert L.hh_set_spectrum_phase(ctx, 0.5) == -1 and b"hh_set_spectrum_phase" in L.hh_last_error(ctx)
        with pytest.raises(ValueError):
            eng.set_phase_score(0.5)
        assert eng._phase is None and np.array_equal(eng.sweep(p), filtered) and eng.last_first_pass == "filtered"
