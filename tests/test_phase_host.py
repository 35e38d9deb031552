"""Host side of the phase score across the meridian: the port of compute_phase_difference_across_meridian against the
reference's recorded outputs (G21), the oracle's definition against that function, the four-product identities the kernel
rests on, the weight's specification and the public surface.  No GPU."""
import ctypes as C
import inspect
import re
from pathlib import Path

import numpy as np
import pytest

import helicon_amd as H
from helicon_amd import _lib
from helicon_amd.grid import phase_spec
from oracle import path_b as O

from tests import phase_oracle as P

ROOT = Path(__file__).resolve().parents[1]
NEW = ("hh_set_spectrum_phase", "hh_sweep_parts", "hh_phase_map")


def test_port_equals_the_reference_outputs():
    g = np.load(ROOT / "tests" / "golden" / "g21_phase_difference.npz")
    n = int(g["n_cases"][0])
    assert n == 4
    shapes = set()
    for k in range(n):
        phase, want = g[f"phase_{k}"], g[f"diff_{k}"]
        got = H.compute_phase_difference_across_meridian(phase)
        assert got.dtype == want.dtype and got.shape == want.shape
        assert np.array_equal(got, want), k
        assert np.all(got[..., 0] == 0) and got.min() >= 0 and got.max() <= 180   # the index-0 column rule, degrees in [0, 180]
        shapes.add((phase.ndim, phase.shape[-1] % 2))
    assert {(2, 0), (2, 1), (3, 0)} <= shapes


def test_port_pairs_an_odd_length_too():
    phase = np.array([[0.3, 1.0, -2.0, 0.5, 2.5]])
    got = H.compute_phase_difference_across_meridian(phase)
    d = np.array([0.0, 1.0 - 2.5, -2.0 - 0.5, 0.5 + 2.0, 2.5 - 1.0])
    np.testing.assert_allclose(got[0], np.rad2deg(np.arccos(np.cos(d))), rtol=0, atol=1e-12)
    assert got[0, 0] == 0 and not np.shares_memory(got, phase)


@pytest.mark.parametrize("ny,nx", [(64, 64), (48, 80)])
def test_oracle_cosine_is_the_reference_function_at_the_default_sampling(ny, nx):
    """c on the fftshifted plane = cos(deg2rad(f(phase_of(img.T)))).T: the reference mirrors the last axis (a vertical
    helix), the sweep's helix lies along x."""
    apix = 2.0
    clean = O.simulate_helical_projection(1, 29.0, 10.0, 1, 0.4 * ny * apix, 2 * apix, 0, 0, ny, nx, apix, rot=40)
    img = clean + np.random.default_rng(0).normal(0, 0.5 * clean.std(), clean.shape)
    c = P.phase_map(img, apix)[1]
    phase_t = O.compute_power_spectra(img.T, apix)[1]
    ref = np.cos(np.deg2rad(H.compute_phase_difference_across_meridian(phase_t))).T
    err = np.abs(c - ref)
    print(f"{ny} x {nx}: max |c - reference| = {err.max():.2e}")
    assert err.max() <= 1e-12
    assert np.all(ref[0] == 1.0) and np.abs(c[0] - 1.0).max() <= 1e-12      # row 0: the unpaired frequency, 1 on both sides


def test_four_product_identities():
    rng = np.random.default_rng(3)
    a = rng.normal(size=(40, 17)) + 1j * rng.normal(size=(40, 17))       # Gy_c[u]
    b = rng.normal(size=(17, 56)) + 1j * rng.normal(size=(17, 56))       # Gx_c[v]
    p1, p2, p3, p4 = a.real @ b.real, a.imag @ b.imag, a.real @ b.imag, a.imag @ b.real
    f, ft = a @ b, np.conj(a) @ b
    scale = np.abs(f).max()
    assert np.abs(f - ((p1 - p2) + 1j * (p3 + p4))).max() <= 1e-13 * scale
    assert np.abs(ft - ((p1 + p2) + 1j * (p3 - p4))).max() <= 1e-13 * scale
    assert np.abs((f * np.conj(ft)).real - (p1 ** 2 - p2 ** 2 + p3 ** 2 - p4 ** 2)).max() <= 1e-13 * scale ** 2


def test_conjugate_factors_are_the_transform_across_the_meridian():
    """A real footprint's factor at -f_y is the conjugate of its factor at f_y, on a zoomed grid as well: F~ of the oracle
    (conj(Ey)) is the image's transform at (-f_y, f_x), also on the row u = ony/2 that has no partner on the grid."""
    img = np.random.default_rng(4).normal(size=(20, 24))
    f, ft = P.transforms(img, 2.0, (7.0, 9.0), (16, 18))
    fy = np.fft.fftshift(np.fft.fftfreq(16) * 4.0 / 7.0)
    fx = np.fft.fftshift(np.fft.fftfreq(18) * 4.0 / 9.0)
    y, x = np.arange(20) - 10, np.arange(24) - 12
    direct = np.exp(-2j * np.pi * np.outer(-fy, y)) @ img @ np.exp(-2j * np.pi * np.outer(fx, x)).T
    assert np.abs(ft - direct).max() <= 1e-12 * np.abs(f).max()


def test_phase_spec():
    for w in (0, 0.0, None, -0.0):
        assert phase_spec(w) is None
    assert phase_spec() is None
    assert phase_spec(0.25) == 0.25 and phase_spec(1) == 1.0 and phase_spec(np.float32(0.5)) == 0.5
    assert isinstance(phase_spec(1), float)
    for w in (float("nan"), -0.1, 1.0001, float("inf"), -float("inf")):
        with pytest.raises(ValueError):
            phase_spec(w)
    assert H.phase_spec is phase_spec


def test_public_surface():
    header = (ROOT / "include" / "helicon_hip.h").read_text()
    assert "int hh_set_spectrum_phase(hh_ctx* ctx, double weight);" in header
    assert "int hh_sweep_parts(hh_ctx* ctx, const double* params, int64_t g, float* scores, float* amplitude, float* phase);" in header
    assert "int hh_phase_map(hh_ctx* ctx, const float* image, int log_flag, float* map_out, float* cos_out);" in header
    L = _lib.lib()                                           # loads the library and binds every name of EXPORTS
    for name in NEW:
        assert name in _lib.EXPORTS and hasattr(L, name)
    assert L.hh_abi_version() == 1
    assert inspect.signature(H.sweep).parameters["phase_weight"].default == 0.0
    assert list(inspect.signature(H.SweepEngine.set_phase_score).parameters) == ["self", "weight"]
    assert list(inspect.signature(H.SweepEngine.sweep_parts).parameters) == ["self", "params"]
    assert inspect.signature(H.SweepEngine.phase_map).parameters["log"].default is True
    assert '"phase"' in (H.SweepEngine.last_first_pass.__doc__ or "")


def test_null_context_is_refused_without_a_device():
    L = _lib.lib()
    assert L.hh_set_spectrum_phase(None, 0.5) == -1
    out = np.zeros(1, np.float32)
    p = np.array([[29.0, 10.0, 1.0, 0.0]])
    assert L.hh_sweep_parts(None, p.ctypes.data_as(C.POINTER(C.c_double)), 1, out.ctypes.data_as(C.POINTER(C.c_float)), None, None) == -1
    assert L.hh_phase_map(None, out.ctypes.data_as(C.POINTER(C.c_float)), 1, out.ctypes.data_as(C.POINTER(C.c_float)), None) == -1


def test_entry_points_are_function_try_blocks():
    src = (ROOT / "helicon_amd" / "csrc" / "phase_sweep.inc").read_text()
    for name in NEW:
        assert re.search(r'extern "C" int ' + name + r"\([^)]*\) try \{", src), name
        assert f'HH_CATCH_CTX(c, "{name}")' in src, name
    main = (ROOT / "helicon_amd" / "csrc" / "helicon_hip.hip").read_text()
    assert main.index('#include "filtered_sweep.inc"') < main.index('#include "phase_sweep.inc"')


def test_driver_flag_and_sweep_argument(monkeypatch, tmp_path):
    import argparse

    from helicon_amd import denovo3DBatch as B
    from helicon_amd.grid import build_grid

    class Result:
        grid = build_grid(np.array([29.0]), np.array([10.0]), (1,), tube_length=128.0)
        scores = np.zeros((1, 1, 1, 1), np.float32)
        best = [(29.0, 10.0, 1, 0.0)]

    np.save(tmp_path / "img.npy", np.zeros((64, 64), np.float32))
    seen = []
    monkeypatch.setattr(B, "sweep", lambda images, *a, **k: seen.append(k) or Result())
    args = lambda argv: B.add_args(argparse.ArgumentParser()).parse_args(argv)   # noqa: E731
    base = [str(tmp_path / "img.npy"), "--twist", "29", "29", "1", "--rise", "10", "10", "1", "--apix", "2"]
    rep = B.run(args(base + ["--out", str(tmp_path / "a.npz")]))
    assert "phase_weight" not in seen[-1] and "phase_weight" not in rep                # off: everything is as before the flag
    assert "phase_weight" not in np.load(tmp_path / "a.npz").files
    rep = B.run(args(base + ["--phase-weight", "0", "--out", str(tmp_path / "a.npz")]))
    assert "phase_weight" not in seen[-1] and "phase_weight" not in rep
    rep = B.run(args(base + ["--phase-weight", "0.5", "--cutoff-res", "8", "8", "--out", str(tmp_path / "b.npz")]))
    assert seen[-1]["phase_weight"] == 0.5 and rep["phase_weight"] == 0.5
    assert float(np.load(tmp_path / "b.npz")["phase_weight"]) == 0.5
    n = len(seen)
    for bad in (["--phase-weight", "1.5"], ["--phase-weight", "nan"], ["--phase-weight", "0.5", "--spectrum-high-pass", "0.05"]):
        with pytest.raises(SystemExit, match="phase-weight"):
            B.run(args(base + bad))
    assert len(seen) == n
    img = np.zeros((64, 64), np.float32)
    with pytest.raises(ValueError, match="phase_weight"):                             # refused before any engine is asked
        H.sweep(img, np.array([29.0]), np.array([10.0]), (1,), apix=2.0, helical_diameter=50.0, ball_radius=4.0,
                phase_weight=0.5, high_pass_fraction=0.05, engine=object())
