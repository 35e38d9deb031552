"""Host side of the local resolution map (helicon_amd/local_resolution.py, csrc/local_resolution.inc): the C ABI's shape,
argument refusals through ctypes with no device, the LDS arithmetic of every window side, the three host rules against the
float64 yardstick (tests/local_fsc_cases.py), the yardstick's own sensitivity to five wrong variants on the GPU cases, and
the cap on the windows the GPU tests may leave out of the resolution comparison.  No GPU."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

import local_fsc_cases as Y
import helicon_amd as H
from helicon_amd import _lib
from helicon_amd.local_resolution import (LocalFSC, lds_bytes, resolution_from_curve, taper_profile, window_centres)

ROOT = Path(__file__).resolve().parent.parent
ENTRY_POINTS = {"hh_lres_create", "hh_lres_destroy", "hh_lres_run", "hh_lres_set_budget", "hh_lres_plan", "hh_lres_upsample"}
LDS_MAX = 163840


def test_entry_points_in_header_exports_and_library():
    hdr = (ROOT / "include" / "helicon_hip.h").read_text()
    declared = set(re.findall(r"^\s*(?:int64_t|int|void|const char\*)\s+(hh_lres_\w+)\s*\(", hdr, flags=re.M))
    assert declared == ENTRY_POINTS and ENTRY_POINTS <= set(_lib.EXPORTS)
    L = _lib.lib()
    for name in ENTRY_POINTS:
        assert hasattr(L, name)
    assert L.hh_abi_version() == 1
    text = (ROOT / "helicon_amd" / "csrc" / "local_resolution.inc").read_text()
    found = re.findall(r'^extern "C" int (hh_\w+)\([^;{]*\)\s*(try)?\s*\{', text, re.M)
    assert dict(found) == {name: "try" for name in ENTRY_POINTS}        # function-try-blocks: the exception barrier
    assert text.count("HH_CATCH_CTX(nullptr, ") == len(ENTRY_POINTS)
    for other in ("fourier_correlation.inc", "true_fsc.inc"):
        assert "hh_lres" not in (ROOT / "helicon_amd" / "csrc" / other).read_text()
    unit = (ROOT / "helicon_amd" / "csrc" / "helicon_hip.hip").read_text()
    assert unit.index('#include "fourier_correlation.inc"') < unit.index('#include "local_resolution.inc"')
    assert H.LocalFSC is LocalFSC and H.taper_profile is taper_profile and H.window_centres is window_centres
    assert H.resolution_from_curve is resolution_from_curve and callable(H.local_resolution)


def test_argument_refusals_need_no_gpu():
    L = _lib.lib()
    f32p, f64p, i32p = C.POINTER(C.c_float), C.POINTER(C.c_double), C.POINTER(C.c_int32)
    a = np.zeros(16 ** 3, np.float32)
    cen = np.full(3, 8, np.int32)
    out = np.zeros(64, np.float64)
    pa, pc, po = a.ctypes.data_as(f32p), cen.ctypes.data_as(i32p), out.ctypes.data_as(f64p)
    h = C.c_void_p()
    fake = C.c_void_p(1)      # never dereferenced: these checks come first
    nan = float("nan")
    cases = [
        (lambda: L.hh_lres_create(None, 0, pa, pa, 16, 16, 16), b"hh_lres_create", b"NULL"),
        (lambda: L.hh_lres_create(C.byref(h), 0, None, pa, 16, 16, 16), b"hh_lres_create", b"NULL"),
        (lambda: L.hh_lres_create(C.byref(h), 0, pa, None, 16, 16, 16), b"hh_lres_create", b"NULL"),
        (lambda: L.hh_lres_create(C.byref(h), 0, pa, pa, 7, 16, 16), b"hh_lres_create", b"[8, 512]"),
        (lambda: L.hh_lres_create(C.byref(h), 0, pa, pa, 16, 513, 16), b"hh_lres_create", b"[8, 512]"),
        (lambda: L.hh_lres_create(C.byref(h), 0, pa, pa, 16, 16, 0), b"hh_lres_create", b"[8, 512]"),
        (lambda: L.hh_lres_run(None, 8, pa, pc, 1, 1.0, 0.5, 0, po, None, None), b"hh_lres_run", b"NULL"),
        (lambda: L.hh_lres_run(fake, 8, None, pc, 1, 1.0, 0.5, 0, po, None, None), b"hh_lres_run", b"NULL"),
        (lambda: L.hh_lres_run(fake, 8, pa, None, 1, 1.0, 0.5, 0, po, None, None), b"hh_lres_run", b"NULL"),
        (lambda: L.hh_lres_run(fake, 8, pa, pc, 1, 1.0, 0.5, 0, None, None, None), b"hh_lres_run", b"NULL"),
        (lambda: L.hh_lres_run(fake, 9, pa, pc, 1, 1.0, 0.5, 0, po, None, None), b"hh_lres_run", b"even"),
        (lambda: L.hh_lres_run(fake, 6, pa, pc, 1, 1.0, 0.5, 0, po, None, None), b"hh_lres_run", b"[8, 64]"),
        (lambda: L.hh_lres_run(fake, 66, pa, pc, 1, 1.0, 0.5, 0, po, None, None), b"hh_lres_run", b"[8, 64]"),
        (lambda: L.hh_lres_run(fake, 26, pa, pc, 1, 1.0, 0.5, 1, po, None, None), b"hh_lres_run", b"LDS route"),
        (lambda: L.hh_lres_run(fake, 8, pa, pc, 1, 1.0, 0.5, 3, po, None, None), b"hh_lres_run", b"route"),
        (lambda: L.hh_lres_run(fake, 8, pa, pc, 0, 1.0, 0.5, 0, po, None, None), b"hh_lres_run", b"windows"),
        (lambda: L.hh_lres_run(fake, 8, pa, pc, 1, 0.0, 0.5, 0, po, None, None), b"hh_lres_run", b"apix"),
        (lambda: L.hh_lres_run(fake, 8, pa, pc, 1, 1.0, nan, 0, po, None, None), b"hh_lres_run", b"threshold"),
        (lambda: L.hh_lres_run(fake, 8, pa, pc, 1, 1.0, 1.0, 0, po, None, None), b"hh_lres_run", b"threshold"),
        (lambda: L.hh_lres_run(fake, 8, pa, pc, 1, 1.0, -1.0, 0, po, None, None), b"hh_lres_run", b"threshold"),
        (lambda: L.hh_lres_set_budget(None, 0, 0), b"hh_lres_set_budget", b"NULL"),
        (lambda: L.hh_lres_set_budget(fake, -1, 0), b"hh_lres_set_budget", b">= 0"),
        (lambda: L.hh_lres_set_budget(fake, 0, -1), b"hh_lres_set_budget", b">= 0"),
        (lambda: L.hh_lres_plan(9, 0, 0, 0, None, None, None), b"hh_lres_plan", b"even"),
        (lambda: L.hh_lres_plan(26, 1, 0, 0, None, None, None), b"hh_lres_plan", b"LDS route"),
        (lambda: L.hh_lres_plan(8, 0, -1, 0, None, None, None), b"hh_lres_plan", b">= 0"),
        (lambda: L.hh_lres_upsample(0, None, 1, 1, 1, 4, 8, 8, 8, pa), b"hh_lres_upsample", b"NULL"),
        (lambda: L.hh_lres_upsample(0, po, 1, 1, 1, 4, 8, 8, 8, None), b"hh_lres_upsample", b"NULL"),
        (lambda: L.hh_lres_upsample(0, po, 1, 1, 1, 0, 8, 8, 8, pa), b"hh_lres_upsample", b"step"),
        (lambda: L.hh_lres_upsample(0, po, 1, 1, 1, 4, 8, 513, 8, pa), b"hh_lres_upsample", b"[1, 512]"),
        (lambda: L.hh_lres_upsample(0, po, 1, 9, 1, 4, 8, 8, 8, pa), b"hh_lres_upsample", b"grid"),
    ]
    for call, name, word in cases:
        assert call() == -1   # HH_ERR_ARG
        msg = L.hh_last_error(None)
        assert msg.startswith(name) and word in msg, msg
        assert not h.value
    assert L.hh_lres_destroy(None) == 0


def test_python_refusals_come_before_any_device_call():
    cube = np.zeros((16, 16, 16), np.float32)
    for bad in (np.zeros((16, 16), np.float32), np.zeros((6, 16, 16), np.float32), np.broadcast_to(np.float32(0), (16, 16, 520))):
        with pytest.raises(ValueError):
            LocalFSC(bad, bad)
    with pytest.raises(ValueError, match="one shape"):
        LocalFSC(cube, np.zeros((16, 16, 18), np.float32))
    holed = cube.copy()
    holed[3, 4, 5] = np.nan
    with pytest.raises(ValueError, match="NaN or infinite"):
        LocalFSC(cube, holed)
    with pytest.raises(ValueError, match="real"):
        LocalFSC(cube.astype(np.complex64), cube)


def test_lds_plan_of_every_window_side():
    L = _lib.lib()
    for w in range(8, 65, 2):
        route, lds, per = C.c_int32(0), C.c_int64(-1), C.c_int64(0)
        assert L.hh_lres_plan(w, 0, 0, 0, C.byref(route), C.byref(lds), C.byref(per)) == 0
        h = w // 2 + 1
        if w <= 24:
            assert route.value == 1
            spectra = 2 * w * w * h * 8
            assert spectra <= lds.value <= LDS_MAX, (w, lds.value)
            assert lds.value == lds_bytes(w) == 8 * (4 * h + 3) + 4 * (2 * w * w * (w + 3) + 2 * w + 2)   # rows of w + 3 floats
            assert L.hh_lres_plan(w, 1, 0, 0, None, None, None) == 0
        else:
            assert route.value == 2 and lds.value == 0
            assert L.hh_lres_plan(w, 1, 0, 0, None, None, None) == -1
        assert L.hh_lres_plan(w, 2, 0, 0, C.byref(route), None, C.byref(per)) == 0 and route.value == 2
        assert per.value == min((8 << 30) // (10 * w ** 3 * 4), 65535 // (2 * w))          # fc_chunk's two caps
        assert L.hh_lres_plan(w, 2, 10 * w ** 3 * 4 * 3, 0, None, None, C.byref(per)) == 0 and per.value == 3
        assert L.hh_lres_plan(w, 2, 1, 0, None, None, C.byref(per)) == 0 and per.value == 1
        assert L.hh_lres_plan(w, 0, 0, 5, None, None, C.byref(per)) == 0 and per.value == 5
    assert 4 * lds_bytes(16) <= LDS_MAX       # four workgroups per compute unit at 16
    assert lds_bytes(24) == 125056


def test_host_rules_equal_the_yardstick():
    for w in range(8, 65, 2):
        for taper in ((0.5, 0.5), (0.8, 0.1), (0.0, 0.5), (1.0, 0.1), (0.3, 0.2)):
            got = taper_profile(w, *taper)
            assert got.dtype == np.float32 and np.array_equal(got, Y.taper_profile(w, *taper))
    assert (taper_profile(12, 1.2, 0.1) == 1).all() and taper_profile(16)[0] < 1e-6 and taper_profile(16)[8] == 1
    for n in (8, 9, 24, 31, 32, 70):
        for s in (1, 2, 3, 4, 7, 8, 32, 100):
            got = window_centres(n, s)
            assert np.array_equal(got, Y.window_centres(n, s))
            if s // 2 > n - 1:
                assert got.size == 0
                continue
            assert got[0] == s // 2 and got[-1] <= n - 1 < got[-1] + s and (np.diff(got) == s).all()
    rng = np.random.default_rng(3)
    for w in (8, 16, 26):
        for _ in range(50):
            f = np.clip(np.sort(rng.uniform(-0.2, 1.0, w // 2 + 1))[::-1] + rng.normal(0, 0.05, w // 2 + 1), -1, 1)
            for thr in (0.5, 0.143):
                want, _, _ = Y.resolution_from_curve(f, w, 1.5, thr)
                assert resolution_from_curve(f, w, 1.5, thr) == pytest.approx(want, rel=1e-13)


def test_crossing_rule_on_hand_made_curves():
    w, apix = 8, 2.0
    never = np.array([1.0, 0.9, 0.8, 0.7, 0.6])
    assert resolution_from_curve(never, w, apix, 0.5) == 2 * apix == Y.resolution_from_curve(never, w, apix, 0.5)[0]     # Nyquist, no 999
    first = np.array([1.0, 0.4, 0.9, 0.9, 0.9])
    assert resolution_from_curve(first, w, apix, 0.5) == w * apix and Y.resolution_from_curve(first, w, apix, 0.5)[1:] == ("first", 1)
    dc = np.array([-1.0, 0.9, 0.8, 0.7, 0.6])                                      # shell 0 is never searched
    assert resolution_from_curve(dc, w, apix, 0.5) == 2 * apix
    mid = np.array([1.0, 0.9, 0.7, 0.3, 0.9])                                      # crosses half way between shells 2 and 3
    assert resolution_from_curve(mid, w, apix, 0.5) == pytest.approx(1.0 / (2.5 / (w * apix)), rel=1e-15)
    assert Y.resolution_from_curve(mid, w, apix, 0.5)[1:] == ("interp", 3)
    last = np.array([1.0, 0.9, 0.8, 0.7, 0.1])
    assert resolution_from_curve(last, w, apix, 0.5) == pytest.approx(1.0 / ((3 + 0.2 / 0.6) / (w * apix)), rel=1e-15)
    with pytest.raises(ValueError):
        resolution_from_curve(never[:4], w, apix, 0.5)


WRONG = (("centre offset off by one", dict(corner_shift=1)), ("no taper", dict(taper=(0.0, 0.5))),
         ("half-spectrum weight", dict(full=False)), ("edge replication", dict(pad="edge")))


@pytest.mark.parametrize("shape,w,step", Y.ALL_CASES, ids=lambda v: str(v).replace(" ", ""))
def test_yardstick_tells_the_wrong_variants_apart(shape, w, step):
    h1, h2 = Y.make_halves(shape)
    base = Y.case(shape, w, step)
    bound = max(Y.TOL_CURVE.values())
    for name, kw in WRONG:
        v = Y.local_fsc(h1, h2, Y.APIX, w, step, 0.5, **kw)
        moved_curve = float(np.abs(v["curves"] - base["curves"]).max())
        moved_res = int((v["resolution"] != base["resolution"]).sum())
        print(f"LFSC_SENS {shape} w={w} {name}: curve {moved_curve:.2e} resolutions {moved_res}")
        assert moved_curve > 100 * bound or moved_res > 0, name


def test_yardstick_tells_dc_in_the_search_apart():
    """fsc[0] is +1 or -1 (the sign of the product of the two window sums), so including shell 0 only matters where the two
    sums differ in sign; the table as a whole must hold such windows."""
    moved = 0
    for shape, w, step in Y.ALL_CASES:
        h1, h2 = Y.make_halves(shape)
        base, v = Y.case(shape, w, step), Y.local_fsc(h1, h2, Y.APIX, w, step, 0.5, first_shell=0)
        assert np.array_equal(v["curves"], base["curves"])
        moved += int((v["resolution"] != base["resolution"]).sum())
    assert moved > 0


@pytest.mark.parametrize("shape,w,step", Y.ALL_CASES, ids=lambda v: str(v).replace(" ", ""))
def test_exclusion_cap_holds_from_the_yardstick_alone(shape, w, step):
    for thr in Y.THRESHOLDS:
        c = Y.case(shape, w, step, thr)
        near = Y.near_threshold(c["curves"], thr)
        print(f"LFSC_NEAR {shape} w={w} thr={thr}: {int(near.sum())} of {near.size}")
        assert near.sum() <= Y.MAX_EXCLUDED * near.size
        assert set(np.unique(c["branch"])) <= {"nyquist", "first", "interp"}


def test_yardstick_upsample_on_a_hand_made_grid():
    g = np.array([[[1.0, 3.0]]])                      # one centre along z and y, two along x at 2 and 6
    up = Y.upsample(g, 4, (3, 2, 9))
    assert up.shape == (3, 2, 9) and np.allclose(up[1, 1], [1, 1, 1, 1.5, 2, 2.5, 3, 3, 3])
    g = np.array([[[1.0, np.nan]]])
    assert np.array_equal(Y.upsample(g, 4, (1, 1, 9))[0, 0, :6], np.ones(6)) and np.isnan(Y.upsample(g, 4, (1, 1, 9))[0, 0, 6:]).all()
    assert np.isnan(Y.upsample(np.full((1, 1, 1), np.nan), 4, (2, 2, 2))).all()


def test_cli_report_and_files_with_a_stand_in(tmp_path):
    import argparse
    import json

    from helicon_amd import local_resolution as _fn      # the package attribute is the function, the module is reached by name
    import importlib

    LR = importlib.import_module("helicon_amd.local_resolution")
    assert _fn is LR.local_resolution
    from helicon_amd.mrc import read_mrc, write_mrc

    shape = (24, 24, 32)
    h1, h2 = Y.make_halves(shape)
    write_mrc(tmp_path / "h1.mrc", h1, 1.5)
    np.save(tmp_path / "h2.npy", h2)
    mask = np.zeros(shape, np.float32)
    mask[:, :, 16:] = 1
    write_mrc(tmp_path / "m.mrc", mask, 1.5)
    seen = {}

    class StandIn:
        route, kernel_ms = "lds", 0.25

        def __init__(self, want):
            self.resolution = want

        def resolution_map(self):
            return Y.upsample(self.resolution, 4, shape).astype(np.float32)

    def run_fn(a, b, apix, **kw):
        seen.update(kw, apix=apix, same=bool(np.array_equal(a, h1) and np.array_equal(b, h2)))
        want = Y.case(shape, 8, 4)["resolution"].copy()
        keep = kw["mask"][np.ix_(*Y.case(shape, 8, 4)["centres"])]
        want[~keep] = np.nan
        return StandIn(want)

    args = LR.add_args(argparse.ArgumentParser()).parse_args(
        [str(tmp_path / "h1.mrc"), str(tmp_path / "h2.npy"), "--window", "8", "--step", "4", "--mask", str(tmp_path / "m.mrc"),
         "--out", str(tmp_path / "locres.mrc"), "--grid-out", str(tmp_path / "grid.npy")])
    report = LR.run(args, run_fn=run_fn)
    json.dumps(report)
    assert seen["same"] and seen["apix"] == 1.5 and seen["window"] == 8 and seen["step"] == 4 and seen["threshold"] == 0.5
    assert seen["mask"].dtype == bool and seen["mask"].sum() == 24 * 24 * 16 and seen["route"] == "auto"
    grid = np.load(tmp_path / "grid.npy")
    assert report["grid"] == [6, 6, 8] and report["route"] == "lds" and report["kernel_ms"] == 0.25
    assert report["windows"] == 288 and report["evaluated"] == int(np.isfinite(grid).sum()) == 144
    vals = grid[np.isfinite(grid)]
    assert report["min"] == vals.min() and report["max"] == vals.max() and report["median"] == np.median(vals)
    assert len(report["histogram"]["counts"]) == 10 and sum(report["histogram"]["counts"]) == 144
    vol, apix = read_mrc(tmp_path / "locres.mrc")
    assert vol.shape == shape and apix == pytest.approx(1.5) and np.isnan(vol[:, :, :16]).any() and np.isfinite(vol[:, :, 20:]).all()
    with pytest.raises(SystemExit, match="apix"):
        LR.run(LR.add_args(argparse.ArgumentParser()).parse_args([str(tmp_path / "h2.npy"), str(tmp_path / "h2.npy"), "--window", "8", "--step", "4"]),
               run_fn=run_fn)
