"""The pixel-size calibration on the device (helicon_amd/pixel_size.py, csrc/nudft.inc) against the float64 direct sum of
tests/pixel_size_cases.py.  One bound, per image:  max |F_device - F_yardstick| <= B sum |f - mean(f)|, with B four times the
largest value tools/pixel_size_bench.py measured over these same cases (profiles/pixel_size.json; pixel_size_cases.MEASURED)."""
import functools
import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import pixel_size_cases as Y
from helicon_amd import pixel_size as PS
from helicon_amd.mrc import write_mrc

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent


def _held(label, f, x, y):
    """Complex and abs outputs of a stack against the yardstick, under the bound; returns the complex output."""
    want = Y.yardstick(x, y, f)
    lim = Y.B * Y.scale(f)[:, None]
    got = PS.nudft2d2(x, y, f)
    mag = PS.nudft2d2(x, y, f, output="abs")
    assert got.shape == want.shape and got.dtype == np.complex64 and mag.shape == want.shape and mag.dtype == np.float32
    e_c = np.abs(got.astype(np.complex128) - want)
    e_a = np.abs(mag.astype(np.float64) - np.abs(want))
    s = Y.scale(f)[:, None]
    worst = max(float((e / np.where(s > 0, s, np.inf)).max()) for e in (e_c, e_a))
    print(f"{label}: max error / sum|f - mean| = {worst:.3e} (B = {Y.B:g})")
    assert (e_c <= lim).all(), label
    assert (e_a <= lim).all(), label
    return got


@pytest.mark.parametrize("n_img", [1, 3])
@pytest.mark.parametrize("shape", Y.POINT_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_points(shape, n_img):
    f = Y.images(shape, n_img)
    lim = Y.B * Y.scale(f)
    for n in Y.POINT_COUNTS + [PS.nudft_chunk() + 1]:
        x, y = Y.points(n)
        got = _held(f"points {shape} stack {n_img} n {n}", f, x, y).astype(np.complex128)
        assert x[0] == 0 and y[0] == 0
        assert (np.abs(got[:, 0] - f.astype(np.float64).sum(axis=(1, 2))) <= lim).all()      # the origin: the plain sum
        if n >= 3:
            assert x[2] == x[1] - 2 * np.pi and y[2] == y[1] + 2 * np.pi
            assert (np.abs(got[:, 2] - got[:, 1]) <= lim).all()                              # a shift by 2 pi changes nothing
    one = PS.nudft2d2(x[:5], y[:5], f[0])                                                    # a single image: no stack axis
    assert one.shape == (5,) and np.array_equal(one, PS.nudft2d2(x[:5], y[:5], f[:1])[0])


@pytest.mark.parametrize("shape", Y.LONG_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_long_sides(shape):
    """Unit noise with indices up to +-4096 at up to 4.44 radians per pixel, where a float32 phase is off by 1e-3 radians.
    This holds the long-side paths (32 to 64 stages, 64 row tiles) to the bound on noise; it does not, alone, rule out float32
    phases: on noise their errors add with random sign, and a model with both phases as float32 products reaches 1.17, 0.87 and
    1.61 times the bound on the three shapes, so 4096 x 4 passes it (tests/test_nudft_probes_host.py).  The deltas at the ends
    of a 16384-long side in tests/test_gpu_nudft_probes.py miss by a factor of several hundred with such phases."""
    x, y = Y.points(65)
    assert max(np.abs(x).max(), np.abs(y).max()) > 4.0
    _held(f"long {shape}", Y.images(shape, 1), x, y)


def test_offset_is_carried_by_the_mean_term():
    """1000 + N(0, 1): the bound stays relative to sum |f - mean|, which an offset pushed through float32 accumulation
    (error about 1e-7 * 1000 * 4096) does not meet."""
    f = Y.images(Y.OFFSET_SHAPE, 1, offset=Y.OFFSET)
    assert abs(float(f.mean()) - Y.OFFSET) < 1 and Y.scale(f)[0] < 1.2 * f[0].size
    _held("offset", f, *Y.offset_points())


def test_bit_identity():
    shape = (65, 63)
    f = Y.images(shape, 3)
    x, y = Y.points(200)
    a = PS.nudft2d2(x, y, f)
    assert np.array_equal(a.view(np.float32), PS.nudft2d2(x, y, f).view(np.float32))                    # two runs
    assert np.array_equal(a.view(np.float32), PS.nudft2d2(x[::-1], y[::-1], f)[:, ::-1].copy().view(np.float32))   # reversed
    parts = np.concatenate([PS.nudft2d2(x[:77], y[:77], f), PS.nudft2d2(x[77:], y[77:], f)], axis=1)     # two calls
    assert np.array_equal(a.view(np.float32), parts.view(np.float32))
    for b in range(3):                                                                                  # alone and in a stack
        assert np.array_equal(a[b].view(np.float32), PS.nudft2d2(x, y, f[b]).view(np.float32))
    m = PS.nudft2d2(x, y, f, output="abs")
    assert np.array_equal(m, PS.nudft2d2(x, y, f, output="abs"))


def test_image_chunk_seam():
    chunk = PS.nudft_chunk()
    f = Y.images((8, 8), chunk + 1)
    x, y = Y.points(7)
    got = PS.nudft2d2(x, y, f)
    assert got.shape == (chunk + 1, 7)
    for b in (0, chunk - 1, chunk):
        assert np.array_equal(got[b].view(np.float32), PS.nudft2d2(x, y, f[b]).view(np.float32))
    pick = np.r_[0:3, chunk - 2:chunk + 1]
    want = Y.yardstick(x, y, f[pick])
    assert (np.abs(got[pick].astype(np.complex128) - want) <= Y.B * Y.scale(f[pick])[:, None]).all()
    ring = PS.ring_maximum(x, y, f, 7)
    assert np.array_equal(ring, PS.nudft2d2(x, y, f, output="abs").max(axis=0))


@functools.lru_cache(maxsize=None)
def _band_case():
    f = Y.images(Y.RING_SHAPE, Y.RING_STACK)
    X, Yp, R, theta = Y.band()
    want = Y.yardstick(X, Yp, f)
    for a in (f, X, Yp, R, want):
        a.setflags(write=False)
    return f, X, Yp, R, theta, want


def test_ring_maximum_is_the_abs_outputs_maximum():
    f, X, Yp, R, theta, _ = _band_case()
    assert (theta, len(R)) == (3103, 100)
    mag = PS.nudft2d2(X, Yp, f, output="abs").reshape(3, theta, 100)
    ring = PS.ring_maximum(X, Yp, f, 100)
    assert ring.dtype == np.float32 and np.array_equal(ring, mag.max(axis=(0, 1)))                      # bit for bit
    parts = np.maximum(PS.ring_maximum(X, Yp, f[:2], 100), PS.ring_maximum(X, Yp, f[2], 100))
    assert np.array_equal(ring, parts)
    curve, n = PS.ring_power_curve(f, 1.0, 2.2365, 2.0235, 100, 3103)
    assert n == 3 and np.array_equal(curve, PS.curve_from_ring_maximum(ring))


def test_fft_resolution_range_on_the_band():
    f, X, Yp, R, theta, want = _band_case()
    got = PS.fft_resolution_range(f, 1.0, 2.2365, 2.0235, 100, theta)
    assert got.shape == (3, 3103, 100) and got.dtype == np.complex64
    err = np.abs(got.reshape(3, -1).astype(np.complex128) - want) / Y.scale(f)[:, None]
    print(f"band: max error / sum|f - mean| = {err.max():.3e} (B = {Y.B:g})")
    assert err.max() <= Y.B
    assert PS.fft_resolution_range(f[0], 1.0, 2.2365, 2.0235, 100, 12).shape == (12, 100)
    assert PS.fft_resolution_range(f[:1], 1.0, 2.2365, 2.0235, 100, 12).shape == (1, 12, 100)           # a stack of one stays one


@pytest.mark.parametrize("shape, apix_true", [((128, 128), 1.03), ((160, 96), 0.97)], ids=["128x128-1.03", "160x96-0.97"])
def test_calibration_end_to_end(shape, apix_true):
    """Two "micrographs" of 2 and 1 images with a planted graphene ring: the device's calibration is the yardstick's."""
    stack = Y.planted(shape, apix_true, 3)
    stacks = [stack[:2], stack[2:]]
    want = PS.calibrate_pixel_size(stacks, 1.0, standard="graphene", _ring_maximum=Y.ring_maximum)
    got = PS.calibrate_pixel_size(stacks, 1.0, standard="graphene")
    lead = Y.lead(want["pwr_mean"])
    print(f"planted {apix_true}: device {got['apix_new']}, yardstick {want['apix_new']}, lead {lead:.2e}, "
          f"max curve difference {np.abs(got['pwr_mean'] - want['pwr_mean']).max():.2e}")
    assert lead >= 1e-3                    # the yardstick's top value leads by more than the device's error: arg-max is comparable
    assert got["n_images"] == [2, 1] and got["theta_samples"] == 3103 and got["changed"]
    assert int(np.argmax(got["pwr_mean"])) == int(np.argmax(want["pwr_mean"]))
    assert got["apix_new"] == want["apix_new"]
    assert abs(got["apix_new"] - apix_true) <= 0.002


def test_command_line(tmp_path):
    stack = Y.planted((64, 80), 1.02, 2)
    write_mrc(tmp_path / "a.mrc", stack, apix=1.0)
    write_mrc(tmp_path / "b.mrc", stack[1], apix=1.0)
    curve = tmp_path / "curve.txt"
    run = subprocess.run([sys.executable, "-m", "helicon_amd.pixel_size", str(tmp_path / "a.mrc"), str(tmp_path / "b.mrc"), "--standard",
                          "graphene", "--curve", str(curve)], cwd=str(ROOT), capture_output=True, text=True, timeout=240)
    assert run.returncode == 0, run.stderr
    report = json.loads(run.stdout.strip().splitlines()[-1])
    want = PS.calibrate_pixel_size([stack, stack[1]], 1.0, standard="graphene")
    assert report["apix_new"] == want["apix_new"] and report["n_images"] == [2, 1] and report["apix"] == 1.0
    assert report["res_peak"] == want["res_peak"] and report["theta_samples"] == 3103 and report["changed"] == want["changed"]
    table = np.loadtxt(curve)
    assert table.shape == (100, 2) and np.array_equal(table[:, 0], want["R"]) and np.array_equal(table[:, 1], want["pwr_mean"])


def test_limits_are_argument_errors():
    with pytest.raises(ValueError, match="16384"):
        PS.nudft2d2([0.0], [0.0], np.zeros((1, 16385), np.float32))
    with pytest.raises(ValueError):
        PS.ring_maximum([0.0, 1.0], [0.0, 1.0], np.zeros((4, 4), np.float32), 3)
    one = PS.nudft2d2([0.0], [0.0], np.full((1, 16384), 0.5, np.float32))
    assert one.shape == (1,) and one[0] == np.complex64(8192.0)
