"""Host side of the pixel-size calibration (helicon_amd/pixel_size.py): the float64 yardstick against np.fft.fft2, the band and
its grid, the curve's post-processing against SciPy, the whole calibration on a planted ring with the yardstick as the
transform, and the entry points' declarations.  No GPU."""
import re
from pathlib import Path

import numpy as np
import pytest
import scipy.signal
import scipy.stats

import pixel_size_cases as Y
from helicon_amd import _lib
from helicon_amd import pixel_size as PS

ROOT = Path(__file__).resolve().parent.parent
ENTRY_POINTS = {"hh_nudft_chunk", "hh_nudft2d2", "hh_nudft_kernel_ms"}


@pytest.mark.parametrize("shape", [(6, 10), (7, 10), (6, 9), (7, 9), (12, 5)])
def test_yardstick_is_the_centred_fft_on_its_grid(shape):
    """x = 2 pi u / ny goes with the rows: on a non-square image a swapped pairing puts the points off the grid."""
    ny, nx = shape
    f = np.random.default_rng(3).standard_normal(shape)
    u, v = np.meshgrid(np.arange(ny), np.arange(nx), indexing="ij")
    got = Y.yardstick(2 * np.pi * u.ravel() / ny, 2 * np.pi * v.ravel() / nx, f).reshape(shape)
    # the centred origin: e^{+i 2 pi u (ny // 2) / ny} is (-1)^u only for an even side
    want = np.fft.fft2(f) * np.exp(2j * np.pi * (u * (ny // 2) / ny + v * (nx // 2) / nx))
    if ny % 2 == 0 and nx % 2 == 0:
        assert np.abs(want - (-1.0) ** (u + v) * np.fft.fft2(f)).max() <= 1e-12 * np.abs(want).max()
    assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()
    stack = np.stack([f, 2 * f[::-1]])
    both = Y.yardstick(2 * np.pi * u.ravel() / ny, 2 * np.pi * v.ravel() / nx, stack)
    assert both.shape == (2, ny * nx) and np.array_equal(both[0].reshape(shape), got)


def test_band_of_graphene_at_one_angstrom():
    res_low, res_high, theta_samples = PS.calibration_band(1.0, PS.STANDARDS["graphene"])
    assert res_low == pytest.approx(2.2365, abs=1e-12) and res_high == pytest.approx(2.0235, abs=1e-12)
    assert theta_samples == 3103
    R = PS.fft_resolution_range(np.zeros((8, 8)), 1.0, res_low, res_high, 100, theta_samples, return_R_only=True)
    assert R.shape == (100,) and R[0] == 1 / res_low and R[-1] == pytest.approx(1 / res_high, rel=1e-15)
    assert np.array_equal(R, np.linspace(1 / res_low, 1 / res_high, 100))
    # the defaults: from 0 to Nyquist on min(side) // 2 radii
    R = PS.fft_resolution_range(np.zeros((3, 10, 8)), 1.5, return_R_only=True)
    assert np.array_equal(R, np.linspace(0, 1 / 3.0, 4))
    assert PS.STANDARDS == dict(graphene=2.13, graphene_oxide=2.13, go=2.13, gold=2.355, ice=3.661)


def test_band_points_put_the_cosine_on_the_rows():
    X, Y_, R = PS.polar_band_points((8, 8), 1.3, 4.0, 3.0, 5, 7)
    th = np.linspace(0, np.pi, 7, endpoint=False)
    assert X.shape == Y_.shape == (35,) and R.shape == (5,)
    assert np.array_equal(X.reshape(7, 5), 2 * np.pi * 1.3 * R[None, :] * np.cos(th)[:, None])
    assert np.array_equal(Y_.reshape(7, 5), 2 * np.pi * 1.3 * R[None, :] * np.sin(th)[:, None])


def test_band_clamps_to_the_corner_and_refuses_beyond_it():
    # corner_res / half_corner_res = 0.85, so the band passes the corner without being refused only when it is wider than
    # the default: +-20 % at 1.25 A / pixel (corner 1.768 A, refusal below 2.071 A)
    apix = 1.25
    corner = 2 * apix / np.sqrt(2)
    half_corner = 1.0 / (1 / (2 * apix) * (1 + np.sqrt(2)) / 2)
    assert half_corner < 2.13 and 2.13 * 0.8 < corner
    res_low, res_high, theta_samples = PS.calibration_band(apix, 2.13, search_range=0.2)
    assert res_high == corner and res_low == 2.13 * 1.2
    assert PS.calibration_band(apix, 2.13)[1] == 2.13 * 0.95      # the default band stays inside
    assert theta_samples == int(np.pi / ((1 / res_high - 1 / res_low) / 99 / (1 / 2.13))) + 1
    with pytest.raises(ValueError, match="beyond the limit"):
        PS.calibration_band(2.0, 2.13)          # half_corner_res = 3.31 A
    with pytest.raises(ValueError, match="beyond the limit"):
        PS.calibrate_pixel_size(np.zeros((8, 8), np.float32), 2.0, standard="graphene")
    with pytest.raises(ValueError):
        PS.calibrate_pixel_size(np.zeros((8, 8), np.float32), 1.0, standard="granite")
    with pytest.raises(ValueError):
        PS.calibrate_pixel_size(np.zeros((8, 8), np.float32), 1.0)


def test_curve_post_processing_matches_scipy():
    rng = np.random.default_rng(9)
    for n in (100, 37):
        v = rng.gamma(2.0, 3.0, n).astype(np.float32)
        got = PS.curve_from_ring_maximum(v)
        w = v.astype(np.float64)
        w -= np.median(w)
        assert got.dtype == np.float64 and np.array_equal(got, w / scipy.stats.median_abs_deviation(w))
    with np.errstate(all="ignore"):
        flat = PS.curve_from_ring_maximum(np.full(10, 3.0, np.float32))
    assert np.isnan(flat).all()                       # 0 / 0, as in the reference: no special case


def test_counts_weight_the_mean_curve():
    rng = np.random.default_rng(4)
    rings = {1: rng.gamma(2.0, 1.0, 100), 3: rng.gamma(2.0, 1.0, 100)}

    def ring(x, y, f, group):
        assert group == 100 and x.size == y.size == 100 * 3103
        return rings[len(f)]

    stacks = [np.zeros((1, 8, 8), np.float32), np.zeros((3, 8, 8), np.float32)]
    res = PS.calibrate_pixel_size(stacks, 1.0, standard="go", _ring_maximum=ring)
    c1, c3 = PS.curve_from_ring_maximum(rings[1]), PS.curve_from_ring_maximum(rings[3])
    want = scipy.signal.detrend((c1 * 1 + c3 * 3) / 4)
    assert np.array_equal(res["pwr_mean"], want) and res["n_images"] == [1, 3]
    R = np.linspace(1 / 2.2365, 1 / 2.0235, 100)
    assert np.allclose(res["R"], R, rtol=1e-15) and res["res_peak"] == 1 / res["R"][np.argmax(want)]
    assert res["apix_new"] == round(1.0 * 2.13 / res["res_peak"], 3) and res["changed"] == (res["apix_new"] != 1.0)
    assert (res["res_low"], res["res_high"], res["theta_samples"]) == PS.calibration_band(1.0, 2.13)


def test_planted_ring_with_the_yardstick_alone():
    """Unit noise plus three cosines of amplitude 0.3 per image at the graphene spacing: the calibration's arithmetic, fed by
    the float64 direct sum, finds the planted pixel size to the 0.1 % grid step plus rounding."""
    stack = Y.planted((128, 128), 1.00, 2)
    res = PS.calibrate_pixel_size(stack, 1.0, standard="graphene", _ring_maximum=Y.ring_maximum)
    print(f"planted 1.00: apix_new = {res['apix_new']}, lead = {Y.lead(res['pwr_mean']):.2e}")
    assert abs(res["apix_new"] - 1.00) <= 0.002
    assert res["theta_samples"] == 3103 and len(res["R"]) == 100 and res["n_images"] == [2]


def test_entry_points_in_header_exports_and_library():
    hdr = (ROOT / "include" / "helicon_hip.h").read_text()
    declared = set(re.findall(r"^\s*int\s+(hh_nudft\w*)\s*\(", hdr, flags=re.M))
    assert declared == ENTRY_POINTS and ENTRY_POINTS <= set(_lib.EXPORTS)
    L = _lib.lib()
    for name in ENTRY_POINTS:
        assert hasattr(L, name)
    text = (ROOT / "helicon_amd" / "csrc" / "nudft.inc").read_text()
    assert set(re.findall(r'^extern "C" int (hh_\w+)\(', text, re.M)) == ENTRY_POINTS
    assert 'include "nudft.inc"' in (ROOT / "helicon_amd" / "csrc" / "helicon_hip.hip").read_text()
    assert L.hh_nudft_chunk() >= 64 and PS.nudft_chunk() == L.hh_nudft_chunk()
    assert "plugins/images2star/calibratepixelsize.py:88-156" in hdr


def test_package_exports_and_argument_checks():
    import helicon_amd as H

    assert H.calibrate_pixel_size is PS.calibrate_pixel_size and H.nudft2d2 is PS.nudft2d2
    assert H.fft_resolution_range is PS.fft_resolution_range and H.ring_power_curve is PS.ring_power_curve
    with pytest.raises(ValueError):
        PS.nudft2d2([0.0], [0.0], np.zeros((2, 2)), output="power")
    with pytest.raises(ValueError):
        PS.nudft2d2([0.0, 1.0], [0.0], np.zeros((2, 2)))
    with pytest.raises(ValueError):
        PS.nudft2d2([0.0], [0.0], np.zeros(4))
    # the library checks its arguments before it looks for a device: sides 1 ... 16384, the ring's group within the points
    with pytest.raises(ValueError, match="16384"):
        PS.nudft2d2([0.0], [0.0], np.zeros((16385, 1), np.float32))
    with pytest.raises(ValueError, match="group"):
        PS.ring_maximum([0.0, 1.0], [0.0, 1.0], np.zeros((4, 4), np.float32), 3)
    assert PS.nudft2d2([], [], np.zeros((3, 2, 2))).shape == (3, 0)
