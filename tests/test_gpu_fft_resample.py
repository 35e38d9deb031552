"""Fourier resampling on the device (hh_separable_transform_3d, csrc/fourier_resample.inc): fft_resample (abs and real),
fft_rescale and fft_crop against the float64 restatements of tests/fft_resample_oracle.py, on the smallest shapes that
reach every seam of the kernel (one tile / several, M > K, odd sides, a K slice holding 2, skipped passes, sides far
below a tile), the module's command line, and the symmetry search on a device-resampled map.

Tolerance: the project's rule for three MFMA passes, 2e-6 max|want|, raised to 4 x the float32 floor of the NumPy
restatement where that floor exceeds a quarter of it (fft_resample_oracle.tolerance).  Every test prints its figures first."""
import functools

import numpy as np
import pytest

import fft_resample_oracle as O
import helicon_amd as H
from oracle import path_b as PB
from test_gpu_symmetry_search import GRID_R, GRID_T, helix_map

pytestmark = pytest.mark.gpu

APIX = 1.3
IDS = [f"{a}-{b}".replace(" ", "") for a, b in O.CASES]


@functools.lru_cache(maxsize=None)
def case(shape, size):
    """Input and float64 references of one case, computed once; read-only."""
    x = O.blob_volume(shape, seed=sum(shape))
    scale = float(np.prod(size) / np.prod(shape))
    ops = O.resample_ops(shape, size)
    ops = [None if op.shape[0] == op.shape[1] and np.abs(op - np.eye(len(op))).max() < 1e-12 else op for op in ops]
    cut = O.rescale_cutoffs(shape, size, APIX)
    out = dict(x=x, cut=cut)
    for kind in ("abs", "real"):
        want, new_apix = O.fft_resample(x, APIX, size, output=kind)
        out[kind] = (want, float(np.abs(O.float32_passes(x, ops, kind, scale) - want).max()), new_apix)
    spec = O.fft_rescale_3d(x, APIX, cut, size)
    fr, fi = O.float32_passes(x, O.rescale_ops(shape, size, APIX, cut), "store")
    out["spec"] = (spec, float(max(np.abs(fr - spec.real).max(), np.abs(fi - spec.imag).max())))
    for v in out.values():
        for a in (v if isinstance(v, tuple) else (v,)):
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
    return out


def check(got, want, floor, label):
    atol = O.tolerance(want, floor, label)
    err = float(np.abs(got - want).max())
    peak = float(np.abs(want).max())
    print(f"{label}: max |got - want| = {err / peak:.2e} max|want| (float32 floor {floor / peak:.2e}, bound {atol / peak:.2e})")
    assert got.shape == want.shape
    assert err <= atol, f"{label}: {err / peak:.3e} max|want| exceeds {atol / peak:.3e}"
    return err / peak


@pytest.mark.parametrize("kind", ["abs", "real"])
@pytest.mark.parametrize("shape,size", O.CASES, ids=IDS)
def test_fft_resample_matches_the_oracle(shape, size, kind):
    c = case(shape, size)
    want, floor, new_apix = c[kind]
    got, got_apix = H.fft_resample(c["x"], APIX, size, output=kind)
    assert got.dtype == np.float32 and got_apix == new_apix
    check(got, want, floor, f"fft_resample {kind} {shape} -> {size}")


@pytest.mark.parametrize("shape,size", O.LONGEST)
def test_the_longest_side_on_each_axis(shape, size):
    """A side of 1024, in or out, on each axis in turn (32 K slices, 16 M tiles); the other axes have no pass."""
    c = case(shape, size)
    for kind in ("abs", "real"):
        want, floor, _ = c[kind]
        got, _ = H.fft_resample(c["x"], APIX, size, output=kind)
        check(got, want, floor, f"fft_resample {kind} {shape} -> {size}")


@pytest.mark.parametrize("shape,size", O.CASES, ids=IDS)
def test_fft_rescale_matches_the_oracle(shape, size):
    c = case(shape, size)
    want, floor = c["spec"]
    got = H.fft_rescale(c["x"], APIX, c["cut"], size)
    assert got.dtype == np.complex64 and got.shape == tuple(size)
    peak = float(np.abs(want).max())
    atol = O.tolerance(want, floor, f"fft_rescale {shape} -> {size}")
    err = max(float(np.abs(got.real - want.real).max()), float(np.abs(got.imag - want.imag).max()))
    print(f"fft_rescale {shape} -> {size}: max |re, im error| = {err / peak:.2e} max|F| (float32 floor {floor / peak:.2e})")
    assert err <= atol


def test_fft_rescale_2d_matches_the_path_b_oracle():
    shape, size, cut = (24, 20), (16, 30), (5.0, 3.1)
    x = O.blob_volume(shape, seed=24)
    want = PB.fft_rescale(x, APIX, cut, size)
    fr, fi = O.float32_passes(x, O.rescale_ops(shape, size, APIX, cut), "store")
    floor = float(max(np.abs(fr - want.real).max(), np.abs(fi - want.imag).max()))
    got = H.fft_rescale(x, APIX, cut, size)
    assert got.dtype == np.complex64
    check(got.real, want.real, floor, "fft_rescale 2-D re")
    atol = O.tolerance(want, floor, "fft_rescale 2-D")
    assert np.abs(got.imag - want.imag).max() <= atol
    # the defaults on an even image: np.fft.fft2
    want = np.fft.fft2(x.astype(np.float64))
    fr, fi = O.float32_passes(x, O.rescale_ops(shape, shape, 1.0, (2.0, 2.0)), "store")
    floor = float(max(np.abs(fr - want.real).max(), np.abs(fi - want.imag).max()))
    got = H.fft_rescale(x)
    atol = O.tolerance(want, floor, "fft_rescale 2-D, defaults")
    assert max(np.abs(got.real - want.real).max(), np.abs(got.imag - want.imag).max()) <= atol


def test_fft_crop_matches_the_2d_fixtures(golden_dir):
    g = np.load(golden_dir / "g23_fft_crop.npz")
    for k in range(3):
        x, size, want = g[f"case{k}_in"], tuple(int(v) for v in g[f"case{k}_size"]), g[f"case{k}_out"]
        floor = float(np.abs(O.float32_passes(x, O.crop_ops(x.shape, size), "real") - want).max())
        got = H.fft_crop(x, size)
        assert got.dtype == np.float32
        check(got, want, floor, f"fft_crop fixture {k} {x.shape} -> {size}")


@pytest.mark.parametrize("shape,size", O.CROP_CASES_3D)
def test_fft_crop_3d_is_irfftn(shape, size):
    x = O.blob_volume(shape, seed=sum(size))
    want = O.fft_crop(x.astype(np.float64), size)
    floor = float(np.abs(O.float32_passes(x, O.crop_ops(shape, size), "real") - want).max())
    got = H.fft_crop(x, size)
    assert got.shape == tuple(2 * (v // 2) for v in size)
    check(got, want, floor, f"fft_crop {shape} -> {size}")


def test_the_same_size_returns_the_input():
    x = O.blob_volume((24, 20, 28), seed=3)
    got, apix = H.fft_resample(x, APIX, x.shape, output="real")
    assert apix == APIX and got.dtype == np.float32
    check(got, x.astype(np.float64), 0.0, "fft_resample to the same size")
    got, _ = H.fft_resample(x, APIX, x.shape)          # the reference's abs
    check(got, np.abs(x.astype(np.float64)), 0.0, "fft_resample to the same size, abs")


def test_command_line_round_trip(tmp_path, capsys):
    import json

    from helicon_amd.fft_resample import main
    from helicon_amd.mrc import read_mrc, write_mrc

    x = O.blob_volume((24, 24, 24), seed=72)
    write_mrc(tmp_path / "in.mrc", x, 1.5)
    assert main([str(tmp_path / "in.mrc"), str(tmp_path / "out.mrc"), "--size", "16", "16", "16", "--output", "real"]) == 0
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert line["new_shape"] == [16, 16, 16] and line["new_apix"] == 2.25 and line["shape"] == [24, 24, 24] and line["kind"] == "real"
    vol, apix = read_mrc(tmp_path / "out.mrc")
    assert vol.shape == (16, 16, 16) and abs(apix - 2.25) < 1e-6
    want, _ = H.fft_resample(x, 1.5, (16, 16, 16), output="real")
    assert np.array_equal(np.asarray(vol), want)


def test_symmetry_search_on_a_device_resampled_map():
    """48^3 helix at 1 A -> 24^3 at 2 A on the device and by the oracle: the maps agree and the search peaks in the same cell."""
    vol = helix_map((48, 48, 48), 1.0, 29.0, 6.0)
    want, want_apix = O.fft_resample(vol, 1.0, (24, 24, 24), output="real")
    ops = O.resample_ops(vol.shape, (24, 24, 24))
    floor = float(np.abs(O.float32_passes(vol, ops, "real", 1 / 8) - want).max())
    got, apix = H.fft_resample(vol, 1.0, (24, 24, 24), output="real")
    assert apix == want_apix == 2.0
    check(got, want, floor, "helix 48^3 -> 24^3")
    res_dev = H.helical_symmetry_search(got, apix, GRID_T, GRID_R, (1,))
    res_ref = H.helical_symmetry_search(want.astype(np.float32), apix, GRID_T, GRID_R, (1,))
    print(f"best cell: device-resampled {res_dev.best[0]}, oracle-resampled {res_ref.best[0]}")
    assert int(res_dev.best_index[0]) == int(res_ref.best_index[0])
