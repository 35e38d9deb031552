"""Host side of the Fourier shell / ring correlation (no GPU): the float64 restatement against the reference's recorded
output, the shell rules, the resolution rule, the C ABI's new entry points and their refusals, and the two command lines
with stand-ins for the library calls."""
import argparse
import ctypes as C
import json
import re
from pathlib import Path

import numpy as np
import pytest

import fsc_oracle as O
import helicon_amd as H
from helicon_amd import _lib
from helicon_amd import denovo3DBatch as DB
from helicon_amd import fsc as F

ROOT = Path(__file__).resolve().parents[1]
ENTRY_POINTS = {"hh_fsc_3d", "hh_frc_2d"}


@pytest.fixture(scope="module")
def g19(golden_dir):
    return np.load(golden_dir / "g19_fsc.npz")


def test_restatement_equals_the_reference(g19):
    """The yardstick of the GPU tests is pinned to the reference's own output.  The reference transforms these float32 maps
    in single precision, so the restatement's shell rules and sums are fed the same single-precision spectra here and must
    then give the recorded float64 curves to 1e-12; run in float64 (as the GPU tests use it) it differs from them by
    single-precision rounding only."""
    from scipy.fft import fft2, fftn, rfftn

    for k in range(int(g19["n_cubes"][0])):
        a, b = g19[f"cube{k}_a"].astype(np.float32), g19[f"cube{k}_b"].astype(np.float32)
        n = a.shape[0]
        half = O.ratio(O.shell_sums(rfftn(a), rfftn(b), O.shell_3d_half(n), n // 2 + 1))
        full = O.ratio(O.shell_sums(fftn(a), fftn(b), O.shell_3d_full(n), n // 2 + 1))
        for j, apix in enumerate(g19["cube_apix"]):
            rows = g19[f"cube{k}_{j}_fsc"]
            mine = O.calc_fsc(a, b, float(apix))
            assert mine.shape == rows.shape
            assert np.array_equal(mine[:, 0], rows[:, 0])
            assert np.abs(half[: len(rows)] - rows[:, 1]).max() <= 1e-12
            assert np.abs(full - g19[f"cube{k}_{j}_per_shell"]).max() <= 1e-12
            # and the float64 restatement differs from it by single-precision rounding only
            assert np.abs(mine[:, 1] - rows[:, 1]).max() < 1e-6
            assert np.abs(O.calc_fsc_per_shell(a, b, float(apix)) - g19[f"cube{k}_{j}_per_shell"]).max() < 1e-6
        assert len(g19[f"cube{k}_1_fsc"]) < len(g19[f"cube{k}_0_fsc"]) == n // 2 + 1   # apix 0.4 cuts rows
    for k in range(int(g19["n_images"][0])):
        a, b = g19[f"img{k}_a"].astype(np.float32), g19[f"img{k}_b"].astype(np.float32)
        shell, n_shells = O.shell_2d(*a.shape)
        frc = O.ratio(O.shell_sums(fft2(a), fft2(b), shell, n_shells + 1))
        assert np.abs(frc - g19[f"img{k}_frc"]).max() <= 1e-12
        saxis, mine = O.calc_frc_2d(a, b, 2.0)
        assert np.array_equal(saxis, g19[f"img{k}_saxis"]) and np.abs(mine - g19[f"img{k}_frc"]).max() < 1e-6
        assert abs(O.frc_score(a, b, 2.0) - float(g19[f"img{k}_score"])) < 1e-6
        # the package's host half on the reference's curve: the score and the fit are the reference's
        assert F._score_of_curve(g19[f"img{k}_saxis"], g19[f"img{k}_frc"], False) == pytest.approx(float(g19[f"img{k}_score"]), abs=1e-15)
        assert F._score_of_curve(g19[f"img{k}_saxis"], g19[f"img{k}_frc"], True) == pytest.approx(float(g19[f"img{k}_score_fit"]), abs=1e-12)
        empty = np.bincount(shell.ravel(), minlength=n_shells + 1) == 0
        assert empty.any() and (g19[f"img{k}_frc"][empty] == 1.0).all()   # rings above ~0.707 n_shells hold no bin


def test_fixture_inputs_carry_a_noise_floor(g19):
    for k in range(int(g19["n_cubes"][0])):
        a, b = g19[f"cube{k}_a"].astype(np.float32), g19[f"cube{k}_b"].astype(np.float32)
        assert O.floor_ratio(O.sums_3d(a, b)) >= 1e-4 and O.floor_ratio(O.sums_3d(a, b, True)) >= 1e-4
    for k in range(int(g19["n_images"][0])):
        assert O.floor_ratio(O.sums_2d(g19[f"img{k}_a"].astype(np.float32), g19[f"img{k}_b"].astype(np.float32))) >= 1e-4


@pytest.mark.parametrize("shape", [(64, 64), (48, 96), (45, 63), (200, 300), (8, 8)])
def test_host_shell_table_is_the_numpy_expression(shape):
    h, w = shape
    n_shells = min(h, w) // 2
    kx = np.fft.fftfreq(w) ** 2
    ky = np.fft.fftfreq(h) ** 2
    want = np.clip(np.round(np.sqrt(ky[:, None] + kx[None, :]) * n_shells).astype(np.int32), 0, n_shells)
    got = F.frc_shell_table(h, w)
    assert got.dtype == np.int32 and got.flags.c_contiguous and not got.flags.writeable
    assert np.array_equal(got, want) and np.array_equal(got, O.shell_2d(h, w)[0])
    assert F.frc_shell_table(h, w) is got   # cached per shape


@pytest.mark.parametrize("n", [8, 33, 64, 127])
def test_integer_shell_rule_equals_the_float64_expression(n):
    f = np.rint(np.fft.fftfreq(n) * n).astype(np.int64)
    m = f[:, None, None] ** 2 + f[None, :, None] ** 2 + f[None, None, : n // 2 + 1] ** 2
    if n % 2 == 0:
        assert f[n // 2] == -(n // 2)
    assert np.array_equal(np.minimum(F.shell_index_3d(m), n // 2), O.shell_3d_half(n))
    mf = f[:, None, None] ** 2 + f[None, :, None] ** 2 + f[None, None, :] ** 2
    assert np.array_equal(np.minimum(F.shell_index_3d(mf), n // 2), O.shell_3d_full(n))


def test_integer_shell_rule_on_the_largest_shells_of_512():
    n = 512
    k2, kr2 = np.fft.fftfreq(n) ** 2, np.fft.rfftfreq(n) ** 2
    f = np.rint(np.fft.fftfreq(n) * n).astype(np.int64)
    for kz in (0, 255, 256):
        want = np.round(np.sqrt(k2[kz] + k2[:, None] + kr2[None, :]) * n).astype(np.int64)   # unclipped: up to 443
        m = f[kz] ** 2 + f[:, None] ** 2 + f[None, : n // 2 + 1] ** 2
        assert np.array_equal(F.shell_index_3d(m), want)
    assert F.shell_index_3d(np.array([0, 1, 2, 3, 6, 7, 12, 13])).tolist() == [0, 1, 1, 2, 2, 3, 3, 4]


def test_fsc_resolution_rule(g19):
    s = np.arange(6) / 48.0
    # crossing between shells 3 (0.3) and 4 (0.1) at 0.143, between 2 and 3 at 0.5
    c = np.array([1.0, 0.9, 0.6, 0.3, 0.1, 0.0])
    assert H.fsc_resolution(s, c, 0.143) == pytest.approx(1.0 / (s[3] + (0.143 - 0.3) * (s[4] - s[3]) / (0.1 - 0.3)))
    assert H.fsc_resolution(s, c, 0.5) == pytest.approx(1.0 / (s[2] + (0.5 - 0.6) * (s[3] - s[2]) / (0.3 - 0.6)))
    assert H.fsc_resolution(s, c) == H.fsc_resolution(s, c, 0.143)
    assert H.fsc_resolution(s, np.array([1.0, 0.9, 0.8, 0.7, 0.6, 0.55]), 0.5) == 999.0       # never below
    assert H.fsc_resolution(s, np.array([0.1, 0.9, 0.6, 0.3, 0.1, 0.0]), 0.5) == 999.0        # first shell below, at frequency 0
    assert H.fsc_resolution(s + 0.01, np.array([0.1, 0.9, 0.6, 0.3, 0.1, 0.0]), 0.5) == pytest.approx(100.0)
    assert H.fsc_resolution(s, np.array([1.0, 1.0, 0.4, 0.4, 0.05, 0.05]), 0.5) == pytest.approx(1.0 / (s[1] + 0.5 / 0.6 * (s[2] - s[1])))
    flat = np.array([0.4, 0.4, 0.4, 0.4, 0.4, 0.4])   # y0 == y1 never arises past index 0: the first index is the one below
    assert H.fsc_resolution(s + 0.01, flat, 0.5) == pytest.approx(100.0)
    # and the reference's own answers, hand-made curves and the fixture's
    for c, want, want_shifted in zip(g19["res_curves"], g19["res_expected"], g19["res_shifted_expected"]):
        for t, thr in enumerate(g19["res_thresholds"]):
            assert H.fsc_resolution(g19["res_saxis"], c, float(thr)) == want[t]
            assert H.fsc_resolution(g19["res_saxis"] + 0.01, c, float(thr)) == want_shifted[t]
    for k in range(int(g19["n_cubes"][0])):
        for j in range(2):
            rows = g19[f"cube{k}_{j}_fsc"]
            for t, thr in enumerate((0.143, 0.5)):
                assert H.fsc_resolution(rows[:, 0], rows[:, 1], thr) == float(g19[f"cube{k}_{j}_res{t}"])


def test_entry_points_in_header_exports_and_library():
    hdr = (ROOT / "include" / "helicon_hip.h").read_text()
    declared = set(re.findall(r"^\s*(?:int64_t|int|void|const char\*)\s+(hh_f[sr]c_\w+)\s*\(", hdr, flags=re.M))
    assert declared == ENTRY_POINTS and ENTRY_POINTS <= set(_lib.EXPORTS)
    L = _lib.lib()
    for name in ENTRY_POINTS:
        assert hasattr(L, name)
    text = (ROOT / "helicon_amd" / "csrc" / "fourier_correlation.inc").read_text()
    found = re.findall(r'^extern "C" int (hh_\w+)\([^;{]*\)\s*(try)?\s*\{', text, re.M)
    assert dict(found) == {name: "try" for name in ENTRY_POINTS}        # function-try-blocks: the exception barrier
    assert 'fourier_correlation.inc"' in (ROOT / "helicon_amd" / "csrc" / "helicon_hip.hip").read_text()
    for name in ("calc_fsc", "calc_fsc_per_shell", "calc_frc_2d", "frc_score", "calc_fsc_batch", "fsc_resolution", "half_map_fsc"):
        assert getattr(H, name) is getattr(F, name)


def test_argument_refusals_need_no_gpu():
    L = _lib.lib()
    f32p, f64p, i32p = C.POINTER(C.c_float), C.POINTER(C.c_double), C.POINTER(C.c_int32)
    a = np.zeros(16 ** 3, np.float32)
    sums = np.zeros(3 * 600, np.float64)
    pa, ps = a.ctypes.data_as(f32p), sums.ctypes.data_as(f64p)
    table = np.zeros(64, np.int32)
    pt = table.ctypes.data_as(i32p)
    cases = [
        (lambda: L.hh_fsc_3d(0, None, pa, 1, 16, 0, ps, None), b"hh_fsc_3d", b"NULL"),
        (lambda: L.hh_fsc_3d(0, pa, pa, 1, 16, 0, None, None), b"hh_fsc_3d", b"NULL"),
        (lambda: L.hh_fsc_3d(0, pa, pa, 0, 16, 0, ps, None), b"hh_fsc_3d", b"batch"),
        (lambda: L.hh_fsc_3d(0, pa, pa, 1, 7, 0, ps, None), b"hh_fsc_3d", b"[8, 512]"),
        (lambda: L.hh_fsc_3d(0, pa, pa, 1, 513, 0, ps, None), b"hh_fsc_3d", b"[8, 512]"),
        (lambda: L.hh_frc_2d(0, pa, pa, 1, 8, 8, None, 4, ps, None), b"hh_frc_2d", b"NULL"),
        (lambda: L.hh_frc_2d(0, pa, pa, 0, 8, 8, pt, 4, ps, None), b"hh_frc_2d", b"batch"),
        (lambda: L.hh_frc_2d(0, pa, pa, 1, 7, 8, pt, 3, ps, None), b"hh_frc_2d", b"[8, 1024]"),
        (lambda: L.hh_frc_2d(0, pa, pa, 1, 8, 1025, pt, 4, ps, None), b"hh_frc_2d", b"[8, 1024]"),
        (lambda: L.hh_frc_2d(0, pa, pa, 1, 8, 8, pt, 513, ps, None), b"hh_frc_2d", b"n_shells"),
        (lambda: L.hh_frc_2d(0, pa, pa, 1, 8, 8, pt, -1, ps, None), b"hh_frc_2d", b"n_shells"),
    ]
    for call, name, word in cases:
        assert call() == -1   # HH_ERR_ARG
        msg = L.hh_last_error(None)
        assert msg.startswith(name) and word in msg, msg
    table[5] = 9
    assert L.hh_frc_2d(0, pa, pa, 1, 8, 8, pt, 4, ps, None) == -1 and b"shell index" in L.hh_last_error(None)


def test_python_refusals_come_before_any_device_call():
    cube = np.zeros((16, 16, 16), np.float32)
    with pytest.raises(NotImplementedError):
        H.calc_fsc(cube, cube, 2.0, F1=np.zeros((16, 16, 9), np.complex64))
    with pytest.raises(NotImplementedError):
        H.calc_fsc(cube, cube, 2.0, None, None, np.zeros(16 * 16 * 9, np.int32))
    for bad1, bad2 in ((np.zeros((16, 16, 12), np.float32),) * 2, (cube, np.zeros((12, 12, 12), np.float32)),
                       (np.zeros((7, 7, 7), np.float32),) * 2, (np.zeros((16, 16), np.float32),) * 2):
        for fn in (H.calc_fsc, H.calc_fsc_per_shell):
            with pytest.raises(ValueError):
                fn(bad1, bad2, 2.0)
    big = np.broadcast_to(np.float32(0), (513, 513, 513))
    with pytest.raises(ValueError, match=r"\[8, 512\]"):
        F.fsc_sums_3d(big, big)
    with pytest.raises(ValueError, match="Image shapes must match: \\(16, 16\\) vs \\(16, 12\\)"):
        H.calc_frc_2d(np.zeros((16, 16), np.float32), np.zeros((16, 12), np.float32), 2.0)
    with pytest.raises(ValueError, match="Image shapes must match"):
        H.frc_score(np.zeros((16, 16), np.float32), np.zeros((12, 16), np.float32), 2.0)
    with pytest.raises(ValueError):
        H.calc_frc_2d(np.zeros((7, 16), np.float32), np.zeros((7, 16), np.float32), 2.0)
    with pytest.raises(ValueError):
        H.calc_frc_2d(np.zeros((16, 1025), np.float32), np.zeros((16, 1025), np.float32), 2.0)
    nan = cube.copy()
    nan[1, 2, 3] = np.nan
    with pytest.raises(ValueError, match="NaN or infinite"):
        H.calc_fsc(nan, cube, 2.0)
    with pytest.raises(ValueError):
        H.calc_fsc_batch(np.zeros((2, 16, 16, 16), np.float32), np.zeros((3, 16, 16, 16), np.float32), 2.0)


def test_no_gpu_means_loud_failure():
    import torch

    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    cube = np.ones((16, 16, 16), np.float32)
    with pytest.raises(H.HeliconHipError):
        H.calc_fsc(cube, cube, 2.0)
    with pytest.raises(H.HeliconHipError):
        H.calc_frc_2d(np.ones((16, 24), np.float32), np.ones((16, 24), np.float32), 2.0)


# ------------------------------------------------------------------------------------------
# half_map_fsc with stand-ins
# ------------------------------------------------------------------------------------------
def oracle_fsc_batch(maps1, maps2, apix, per_shell=False, *, device=0):
    fn = O.calc_fsc_per_shell if per_shell else O.calc_fsc
    return np.stack([fn(a, b, apix) for a, b in zip(maps1, maps2)])


def test_half_map_fsc_composition_with_stand_ins():
    seen = []

    def symmetrize(data, apix, twist, rise, csym, fraction, new_size, new_apix, *, device=0):
        seen.append((data.shape, apix, twist, rise, csym, fraction, tuple(new_size), new_apix))
        rng = np.random.default_rng(int(abs(data).sum() * 1000) % 2**31)
        return rng.standard_normal(new_size).astype(np.float32)

    h1, h2 = np.ones((10, 17, 17), np.float32), np.full((10, 17, 17), 2, np.float32)
    out = F.half_map_fsc_batch([h1, h1], [h2, h2], 3.0, [(29.0, 6.0, 1), (-40.0, 7.5, 2)], symmetrize=symmetrize, fsc_batch=oracle_fsc_batch)
    assert len(out) == 2 and len(seen) == 4
    assert seen[0] == ((10, 17, 17), 3.0, 29.0, 6.0, 1, 1.0, (16, 16, 16), 3.0)      # shape[1] rounded down to even, new_apix = apix3d
    assert seen[3] == ((10, 17, 17), 3.0, -40.0, 7.5, 2, 1.0, (16, 16, 16), 3.0)
    curve, res = out[0]
    assert curve.shape == (9, 2) and set(res) == {"0.5", "0.143"}
    assert res["0.143"] == H.fsc_resolution(curve[:, 0], curve[:, 1], 0.143) and res["0.5"] == H.fsc_resolution(curve[:, 0], curve[:, 1], 0.5)
    out = F.half_map_fsc_batch([h1], [h2], 3.0, [(29.0, 6.0, 1)], size=12, new_apix=4.0, fraction=0.5, per_shell=True, symmetrize=symmetrize,
                               fsc_batch=oracle_fsc_batch)
    assert seen[-1] == ((10, 17, 17), 3.0, 29.0, 6.0, 1, 0.5, (12, 12, 12), 4.0) and out[0][0].shape == (7,)
    with pytest.raises(ValueError, match="not the 12\\^3 cube"):
        F.half_map_fsc_batch([h1], [h2], 3.0, [(29.0, 6.0, 1)], size=12, symmetrize=lambda d, *a, **k: np.zeros((12, 12, 10), np.float32),
                             fsc_batch=oracle_fsc_batch)
    with pytest.raises(ValueError):
        F.half_map_fsc_batch([h1], [h2, h2], 3.0, [(29.0, 6.0, 1)], symmetrize=symmetrize, fsc_batch=oracle_fsc_batch)


# ------------------------------------------------------------------------------------------
# python -m helicon_amd.fsc
# ------------------------------------------------------------------------------------------
def _args(argv):
    return F.add_args(argparse.ArgumentParser()).parse_args(argv)


def oracle_fsc_fn(a, b, apix, per_shell, device=0):
    return O.calc_fsc_per_shell(a, b, apix) if per_shell else O.calc_fsc(a, b, apix)


def test_cli_arguments():
    a = _args(["h1.mrc", "h2.mrc"])
    assert (a.half1, a.half2, a.apix, a.per_shell, a.threshold, a.out, a.device) == ("h1.mrc", "h2.mrc", None, False, [0.143, 0.5], None, 0)
    a = _args(["h1.npy", "h2.npy", "--apix", "1.5", "--per-shell", "--threshold", "0.3", "--out", "c.txt", "--device", "1"])
    assert (a.apix, a.per_shell, a.threshold, a.out, a.device) == (1.5, True, [0.3], "c.txt", 1)
    with pytest.raises(SystemExit):
        _args(["h1.mrc"])


def test_cli_report_and_out_file_with_a_stand_in(tmp_path):
    from helicon_amd.mrc import write_mrc

    a, b = O.make_map_pair(24, 5)
    write_mrc(tmp_path / "h1.mrc", a, 2.0)
    write_mrc(tmp_path / "h2.mrc", b, 2.0)
    out = tmp_path / "curve.txt"
    rep = F.run(_args([str(tmp_path / "h1.mrc"), str(tmp_path / "h2.mrc"), "--out", str(out)]), fsc_fn=oracle_fsc_fn)
    json.dumps(rep)
    want = O.calc_fsc(a, b, 2.0)
    assert rep["maps"] == dict(half1=str(tmp_path / "h1.mrc"), half2=str(tmp_path / "h2.mrc"), shape=[24, 24, 24], apix=2.0)
    assert rep["per_shell"] is False and rep["saxis"] == want[:, 0].tolist() and rep["fsc"] == want[:, 1].tolist()
    assert rep["resolution"] == {"0.143": H.fsc_resolution(want[:, 0], want[:, 1], 0.143), "0.5": H.fsc_resolution(want[:, 0], want[:, 1], 0.5)}
    rows = np.loadtxt(out)
    assert rows.shape == want.shape and np.allclose(rows, want, rtol=1e-8)
    rep = F.run(_args([str(tmp_path / "h1.mrc"), str(tmp_path / "h2.mrc"), "--apix", "0.4", "--per-shell", "--threshold", "0.3"]), fsc_fn=oracle_fsc_fn)
    assert rep["per_shell"] is True and rep["maps"]["apix"] == 0.4 and len(rep["fsc"]) == 13 and list(rep["resolution"]) == ["0.3"]
    assert rep["saxis"] == (np.arange(13) / (24 * 0.4)).tolist() and rep["fsc"] == O.calc_fsc_per_shell(a, b, 0.4).tolist()


def test_cli_refusals(tmp_path):
    np.save(tmp_path / "a.npy", np.zeros((16, 16, 16), np.float32))
    np.save(tmp_path / "b.npy", np.zeros((16, 16, 12), np.float32))
    np.save(tmp_path / "c.npy", np.zeros((6, 6, 6), np.float32))
    with pytest.raises(SystemExit, match="--apix is required"):
        F.run(_args([str(tmp_path / "a.npy"), str(tmp_path / "a.npy")]), fsc_fn=oracle_fsc_fn)
    with pytest.raises(SystemExit, match="two cubic maps"):
        F.run(_args([str(tmp_path / "a.npy"), str(tmp_path / "b.npy"), "--apix", "2"]), fsc_fn=oracle_fsc_fn)
    with pytest.raises(SystemExit, match=r"\[8, 512\]"):
        F.run(_args([str(tmp_path / "c.npy"), str(tmp_path / "c.npy"), "--apix", "2"]), fsc_fn=oracle_fsc_fn)


# ------------------------------------------------------------------------------------------
# denovo3DBatch --rescore N --half-map-fsc K
# ------------------------------------------------------------------------------------------
def _batch_args(tmp_path, *extra):
    np.save(tmp_path / "img.npy", np.random.default_rng(0).random((32, 32)).astype(np.float32))
    argv = [str(tmp_path / "img.npy"), "--apix", "2", "--twist", "28", "30", "1", "--rise", "5", "6", "0.5", "--top", "4", *extra]
    return DB.add_args(argparse.ArgumentParser()).parse_args(argv)


@pytest.fixture
def stub_pipeline(monkeypatch):
    """The sweep, the group solver and the symmetriser replaced by closed forms; the correlation by the restatement."""
    from helicon_amd import denovo3D as D
    from helicon_amd import grid as G
    from helicon_amd import solver as S

    calls = dict(lsq=[], sym=0, fsc=[])

    def fake_sweep(images, twists, rises, csyms, **kw):
        grid = G.build_grid(twists, rises, csyms, tube_length=images.shape[-1] * kw["apix"])
        p = grid.params
        scores = np.exp(-((p[:, 0] - 29.0) ** 2) - ((p[:, 1] - 5.5) ** 2)).astype(np.float32)
        return D.finish_sweep(np.repeat(scores[None], len(images), axis=0), grid)

    def fake_lsq_batch(img, scale, cands, **kw):
        calls["lsq"].append(dict(n=len(cands), fsc_test=kw.get("fsc_test", 0), return_3d=kw["return_3d"]))
        out = []
        for i, (tw, rs, cs) in enumerate(cands):
            maps = (None, None, None)
            if kw["return_3d"]:
                rng = np.random.default_rng(i)
                shape = (kw["reconstruct_length_3d_pixel"], kw["reconstruct_diameter_3d_pixel"], kw["reconstruct_diameter_3d_pixel"])
                sig = rng.standard_normal(shape).astype(np.float32)
                maps = (sig, sig + 0.5 * rng.standard_normal(shape).astype(np.float32), sig + 0.5 * rng.standard_normal(shape).astype(np.float32))
            out.append((maps, 0.5 + 0.01 * tw - 0.02 * rs))
        return out

    def fake_symmetrize(data, apix, twist, rise, csym=1, fraction=1.0, new_size=None, new_apix=None, cpu=1, *, device=0):
        calls["sym"] += 1
        n = new_size[0]
        return np.resize(np.asarray(data, np.float32), (n, n, n))

    def fake_fsc_batch(maps1, maps2, apix, per_shell=False, *, device=0):
        calls["fsc"].append(len(maps1))
        return oracle_fsc_batch(maps1, maps2, apix, per_shell)

    monkeypatch.setattr(DB, "sweep", fake_sweep)
    monkeypatch.setattr(S, "lsq_reconstruct_batch", fake_lsq_batch)
    monkeypatch.setattr(D, "apply_helical_symmetry", fake_symmetrize)
    monkeypatch.setattr(D, "_prepare_task_image", lambda image, *a: image)
    monkeypatch.setattr(F, "calc_fsc_batch", fake_fsc_batch)
    return calls


def test_batch_driver_flag_parses_and_defaults_off(tmp_path):
    assert _batch_args(tmp_path).half_map_fsc == 0
    assert _batch_args(tmp_path, "--rescore", "3", "--half-map-fsc", "2").half_map_fsc == 2
    with pytest.raises(SystemExit):
        _batch_args(tmp_path, "--half-map-fsc", "3")


def test_batch_driver_without_the_flag_is_unchanged(tmp_path, stub_pipeline):
    out = tmp_path / "s.npz"
    args = _batch_args(tmp_path, "--rescore", "3", "--out", str(out))
    del args.half_map_fsc   # a caller that builds its Namespace by hand, from before the flag
    rep = DB.run(args)
    assert all(c == dict(n=c["n"], fsc_test=0, return_3d=False) for c in stub_pipeline["lsq"]) and stub_pipeline["sym"] == 0
    assert set(rep) == {"n_candidates", "n_skipped", "images", "cutoff_res", "spectrum_size", "spectrum_filter", "rescore_interpolation",
                        "rescore_model"}
    rec = rep["images"][0]["rescored"]
    assert len(rec) == 3 and all(set(r) == {"twist", "rise", "csym", "sweep_score", "lsq_score", "interpolation"} for r in rec)
    assert set(np.load(out).files) == {"scores", "twists", "rises", "csyms", "params", "valid", "cutoff_res", "spectrum_size",
                                       "spectrum_filter", "rescore_interpolation", "rescore_model", "rescore_l1_ratio", "rescore_alpha",
                                       "rescored"}


def test_batch_driver_with_the_flag_adds_the_curves(tmp_path, stub_pipeline):
    out = tmp_path / "s.npz"
    rep = DB.run(_batch_args(tmp_path, "--rescore", "3", "--half-map-fsc", "2", "--out", str(out)))
    json.dumps(rep)
    assert all(c["fsc_test"] == 2 and c["return_3d"] for c in stub_pipeline["lsq"])
    assert sum(stub_pipeline["fsc"]) == 3 and len(stub_pipeline["fsc"]) == len(stub_pipeline["lsq"])   # one batched call per box group
    assert stub_pipeline["sym"] == 6
    rec = rep["images"][0]["rescored"]
    assert [r["lsq_score"] for r in rec] == sorted((r["lsq_score"] for r in rec), reverse=True)
    for r in rec:
        assert set(r) == {"twist", "rise", "csym", "sweep_score", "lsq_score", "interpolation", "fsc", "fsc_resolution_0143",
                          "fsc_resolution_05"}
        curve = np.asarray(r["fsc"])
        assert curve.ndim == 2 and curve.shape[1] == 2 and (np.abs(curve[:, 1]) <= 1 + 1e-12).all()
        assert r["fsc_resolution_0143"] == H.fsc_resolution(curve[:, 0], curve[:, 1], 0.143)
        assert r["fsc_resolution_05"] == H.fsc_resolution(curve[:, 0], curve[:, 1], 0.5)
    z = np.load(out)
    assert {"rescored", "rescored_fsc", "rescored_fsc_resolution"} <= set(z.files)
    assert z["rescored_fsc"].shape[:2] == (1, 3) and z["rescored_fsc"].shape[3] == 2 and z["rescored_fsc_resolution"].shape == (1, 3, 2)
    assert np.array_equal(z["rescored_fsc"][0, 0], np.asarray(rec[0]["fsc"]))


def test_batch_driver_refuses_the_flag_with_a_tilt(tmp_path, stub_pipeline):
    for extra in (("--tilt", "5"), ("--psi", "2")):
        with pytest.raises(SystemExit, match="--half-map-fsc needs --tilt 0 --psi 0"):
            DB.run(_batch_args(tmp_path, "--rescore", "3", "--half-map-fsc", "1", *extra))
