"""The zoomed, the filtered and the phase sweep on planes of several output tiles, seen line by line (tests/zoom_bands.py):
136 x 264 (2 x 3 tiles of k_zoom_sweep / k_phase_sweep with a last tile 8 lines wide both ways, 3 x 5 tiles of the filter's
x pass), 129 x 130 and 130 x 129 (a one-line last tile, mixed parity both ways), zoomed from a 96 x 176 image and as the
image's own shape (136 x 264, 129 x 131: filter and phase without a zoom).

For every (case, mode) the probe's eight candidates are swept under each of the 16 + 16 band masks of the scored plane,
against the probe's image and against its second image, and EVERY band score of EVERY candidate is held to the float64
oracle at the project's score tolerance (2e-4 absolute); tests/test_zoom_bands_host.py shows that one
misplaced line moves its band by at least ten times that.  Every sweep is repeated bit for bit.  A sweep under the union
of two bands (other tiles active, both images as two segments) agrees with the oracle under that union.  The reference
side is compared element by element: the device's zoomed power spectrum and phase map against the oracle's planes, at the
tolerances of test_power_spectrum_with_fourier_zoom_against_the_oracle and test_phase_map_against_oracle.

Measured on an MI355X (every test prints its figures; per case in DESIGN.md, "Scored-plane census"): largest
|score - oracle| over all cases, images, bands and candidates 5.9e-7 for the zoomed sweep, 1.4e-6 under lp 0.3 / hp 0.05,
6.4e-7 under hp 0.05, 8.8e-7 for the phase score (5.9e-7 amplitude, 5.0e-7 combined), 7.8e-7 under the unions; power spectrum
1.2e-7, phase map 3.8e-8 of max|M|.  With the tile decode handed tiles_u in place of tiles_v (a temporary mutation) the 14
band and union tests of the 136 x 264 planes that reach k_zoom_sweep / k_phase_sweep fail, 0.13 ... 0.98 from the oracle,
while tests/test_gpu_zoom_sweep.py, test_gpu_phase_sweep.py and test_gpu_filtered_sweep.py pass."""
import numpy as np
import pytest

import helicon_amd as H
import phase_oracle as P
import zoom_bands as ZB
from oracle import path_b as O
from tests import test_gpu_round2 as R2

pytestmark = pytest.mark.gpu

SCORE_TOL = ZB.SCORE_TOL
CASES, MODES = list(ZB.CASES), list(ZB.MODES)


def configure(eng, case, mode):
    """The engine's settings of a mode; returns what last_first_pass must then name (None: the default sampling's own
    pipelines, which no zoom, filter or phase mode touches)."""
    eng.set_zoom(case.cutoff, case.size)
    if mode == "phase":
        eng.set_phase_score(ZB.PHASE_WEIGHT)
        return "phase"
    if ZB.MODES[mode]:
        eng.set_filter(*ZB.MODES[mode])
        return "filtered"
    return "zoom" if case.size else None


def run(eng, mode, params):
    """[parts, S, G]: the score alone, or (combined, amplitude, phase) of the phase mode; repeated bit for bit."""
    if mode == "phase":
        out = np.stack(eng.sweep_parts(params))
        again = np.stack(eng.sweep_parts(params))
        assert np.array_equal(eng.sweep(params), out[0])
    else:
        out = eng.sweep(params)[None]
        again = eng.sweep(params)[None]
    assert np.array_equal(out, again), "not bit-reproducible"
    return out


def expected(name, mode, under):
    """[parts, candidates] float64 from ``under(oracle)``: as run() orders them."""
    if mode != "phase":
        return under(ZB.oracle(name, mode))[None]
    amp, ph = under(ZB.oracle(name, "zoom")), under(ZB.oracle(name, "phase"))
    return np.stack([(1 - ZB.PHASE_WEIGHT) * amp + ZB.PHASE_WEIGHT * ph, amp, ph])


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", CASES)
def test_every_band_of_the_scored_plane(name, mode):
    case = ZB.CASES[name]
    probe = ZB.probe_of(case.shape)
    o = ZB.oracle(name, mode)
    n_cand = len(probe.params)
    seen = 0
    with H.SweepEngine(case.shape) as eng:
        eng.set_geometry(**probe.geometry())
        first = configure(eng, case, mode)
        assert eng.spectrum_shape == case.plane
        for image, img in enumerate((probe.image, probe.image2)):
            for axis in (0, 1):
                got = []
                for mask in o.masks[axis]:
                    eng.set_reference(img, mask)
                    got.append(run(eng, mode, probe.params)[:, 0])
                    assert eng.last_first_pass == first if first else eng.last_first_pass not in ("zoom", "filtered", "phase")
                got = np.stack(got, axis=1)                                             # [parts, bands, candidates]
                ref = np.stack([expected(name, mode, lambda orc, b=b: orc.scores[image][axis][b]) for b in range(16)], axis=1)
                assert got.shape == ref.shape == ((3 if mode == "phase" else 1), 16, n_cand)  # no band, no candidate left out
                err = np.abs(got.astype(np.float64) - ref)
                print(f"{name} {mode} image {image} axis {axis}: max |score - oracle| = {err.max():.3e} "
                      f"(band {int(np.argmax(err.max(axis=(0, 2))))}) over 16 bands x {n_cand} candidates" +
                      (f"; combined {err[0].max():.2e}, amplitude {err[1].max():.2e}, phase {err[2].max():.2e}" if mode == "phase" else ""))
                assert np.isfinite(got).all()
                np.testing.assert_allclose(got, ref, rtol=0, atol=SCORE_TOL, err_msg=f"{name} {mode} image {image} axis {axis}")
                seen += got.shape[1] * got.shape[2]
    assert seen == 2 * 2 * 16 * n_cand


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", CASES)
def test_scores_do_not_depend_on_which_other_tiles_are_active(name, mode):
    """The union of the lowest |kx| band and the highest |ky| band (other tiles, another tile list, other places in the
    partial sums), and of two |kx| bands at the plane's two ends; both images at once as two segments."""
    case = ZB.CASES[name]
    probe = ZB.probe_of(case.shape)
    o = ZB.oracle(name, mode)
    unions = (o.masks[1][0] | o.masks[0][15], o.masks[1][2] | o.masks[1][15], o.masks[0][1] | o.masks[0][14])
    with H.SweepEngine(case.shape) as eng:
        eng.set_geometry(**probe.geometry())
        first = configure(eng, case, mode)
        for k, mask in enumerate(unions):
            eng.set_reference(np.stack([probe.image, probe.image2]), mask)
            got = run(eng, mode, probe.params)                                          # [parts, 2, candidates]
            assert eng.last_first_pass == first if first else eng.last_first_pass not in ("zoom", "filtered", "phase")
            ref = np.stack([expected(name, mode, lambda orc, s=s: orc.under(mask, s)) for s in (0, 1)], axis=1)
            assert got.shape == ref.shape and np.isfinite(got).all() and np.isfinite(ref).all()
            err = np.abs(got.astype(np.float64) - ref)
            print(f"{name} {mode} union {k}: max |score - oracle| = {err.max():.3e} over 2 segments x {got.shape[2]} candidates")
            np.testing.assert_allclose(got, ref, rtol=0, atol=SCORE_TOL, err_msg=f"{name} {mode} union {k}")
            for s, img in enumerate((probe.image, probe.image2)):                      # a segment is what the image alone gives
                eng.set_reference(img, mask)
                np.testing.assert_allclose(run(eng, mode, probe.params)[:, 0], got[:, s], rtol=0, atol=2e-6)


@pytest.mark.parametrize("name", CASES)
def test_zoomed_power_spectrum_element_by_element(name):
    """k_zoom_rows / k_zoom_cols with more than one block along v, against the oracle's plane at
    test_power_spectrum_with_fourier_zoom_against_the_oracle's tolerances (and, for the image's own shape, through its
    entry point at the default frequencies: the Python wrapper routes those to the sweep's transform)."""
    case = ZB.CASES[name]
    probe = ZB.probe_of(case.shape)
    for img in (probe.image, probe.image2):
        if case.size:
            pw, ph = H.compute_power_spectra(img, probe.apix, cutoff_res=case.cutoff, output_size=case.size)
            pw_o, ph_o = O.compute_power_spectra(img, probe.apix, cutoff_res=case.cutoff, output_size=case.size)
        else:
            pw, ph = R2._zoom_direct(img, probe.apix, ZB.NYQUIST, case.shape, True)
            pw_o, ph_o = R2._oracle_direct(img, probe.apix, ZB.NYQUIST, case.shape, True)
        assert pw.shape == ph.shape == case.plane
        strong = pw_o > 0.2                                      # the phase of a near-zero coefficient is noise
        d = np.angle(np.exp(1j * (ph - ph_o)))
        print(f"{name}: max |pwr - oracle| = {np.abs(pw - pw_o).max():.2e}; max |phase - oracle| on {strong.mean():.0%} of the bins = "
              f"{np.abs(d[strong]).max():.2e}")
        np.testing.assert_allclose(pw, pw_o, rtol=0, atol=2e-5)
        assert np.abs(d[strong]).max() < 1e-3


@pytest.mark.parametrize("name", CASES)
def test_phase_map_element_by_element(name):
    """k_phase_cols with more than one block along v, at test_phase_map_against_oracle's tolerances."""
    case = ZB.CASES[name]
    probe = ZB.probe_of(case.shape)
    with H.SweepEngine(case.shape) as eng:
        eng.set_geometry(**probe.geometry())
        eng.set_zoom(case.cutoff, case.size)
        for img in (probe.image, probe.image2):
            m, c = eng.phase_map(img)
            rm, rc, ra = P.phase_map(img, probe.apix, case.cutoff, case.size)
            assert m.shape == c.shape == rm.shape == case.plane
            strong = ra > 1e-3 * ra.max()
            print(f"{name}: max |M - oracle| / max |M| = {np.abs(m - rm).max() / np.abs(rm).max():.2e}; "
                  f"max |c - oracle| on {strong.mean():.0%} of the bins = {np.abs(c - rc)[strong].max():.2e}")
            np.testing.assert_allclose(m, rm, rtol=0, atol=1e-5 * np.abs(rm).max())
            np.testing.assert_allclose(c[strong], rc[strong], rtol=0, atol=1e-5)
