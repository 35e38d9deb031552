"""Host side of the device adaptive mask (no GPU): the definition's pieces restated in NumPy against SciPy, np.histogram,
otsu_threshold_eman and the reference's recorded masks (tests/golden/g20_true_fsc.npz); the entry points and their refusals;
true_fsc(device_support=True) with a stand-in for the resident context."""
import argparse
import ctypes as C
import importlib
import re
from pathlib import Path

import numpy as np
import pytest

import adaptive_mask_cases as AC
import soft_mask_cases as SC
import helicon_amd as H
from helicon_amd import _lib

T = importlib.import_module("helicon_amd.true_fsc")

ROOT = Path(__file__).resolve().parents[1]
ENTRY_POINTS = {"hh_am_otsu", "hh_am_stage_ms", "hh_am_gaussian_3d", "hh_am_label_3d", "hh_am_mask_3d", "hh_am_context_support",
                "hh_am_context_get_support"}


def test_taps_equal_scipys_kernel_bit_for_bit():
    from scipy.ndimage import gaussian_filter1d

    for sigma in (0.1, 0.787, 1.3, 2.0997, 2.1, 3.0, 5.5, 10.5, 37.25):
        w = T.gaussian_taps(sigma)
        r = AC.radius(sigma)
        assert w.dtype == np.float64 and w.shape == (r + 1,)
        impulse = np.zeros(2 * r + 1)
        impulse[r] = 1.0                                                   # products with 1 and sums with 0 are exact
        kernel = gaussian_filter1d(impulse, sigma, mode="constant")
        assert np.array_equal(kernel[r:], w) and np.array_equal(kernel[: r + 1][::-1], w)
    assert H.gaussian_taps is T.gaussian_taps
    for bad in (0.0, -1.0, float("nan"), float("inf"), 1024.2):
        with pytest.raises(ValueError, match="gaussian_taps"):
            T.gaussian_taps(bad)
    assert len(T.gaussian_taps(1024.0)) == 4097


def test_loop_form_of_the_three_passes_equals_scipy_bit_for_bit():
    from scipy.ndimage import gaussian_filter

    for k, (shape, sigma) in enumerate(AC.GAUSS_CASES):
        V = AC.volume(shape, 20 + k)
        want = gaussian_filter(V, sigma)
        got = AC.gaussian_numpy(V, sigma)
        assert got.dtype == np.float64 and np.array_equal(got, want), (shape, sigma)
    assert AC.radius(5.5) == 22 and np.array_equal(AC.fold(np.array([-5, -1, 0, 3, 4, 8, 12]), 4), [3, 0, 0, 3, 3, 0, 3])


def test_edges_rule_equals_np_histogram():
    rng = np.random.RandomState(3)
    for hmin, hmax in ((-1.7, 4.9), (0.0, 1.0), (-3.25e-3, 7.5e-2), (1.0, 1.0 + 2.0**-40)):
        edges = np.linspace(hmin, hmax, 257)
        x = np.concatenate([rng.uniform(hmin, hmax, size=20000), edges, np.nextafter(edges[1:], -np.inf), np.nextafter(edges[:-1], np.inf), [hmin, hmax]])
        want, e = np.histogram(x, bins=256, range=(hmin, hmax))
        assert np.array_equal(e, edges)
        assert np.array_equal(AC.counts_by_edges(x, edges), want)
        # the library's host step builds the same edges
        got_edges, thr = np.empty(257), C.c_double(0.0)
        counts = np.ascontiguousarray(want, dtype=np.int64)
        assert _lib.lib().hh_am_otsu(counts.ctypes.data_as(C.POINTER(C.c_int64)), hmin, hmax, got_edges.ctypes.data_as(C.POINTER(C.c_double)), C.byref(thr)) == 0
        assert np.array_equal(got_edges, edges) and thr.value == T.otsu_from_counts(want, hmin, hmax)


def test_otsu_from_counts_equals_otsu_threshold_eman():
    rng = np.random.RandomState(4)
    volumes = [rng.normal(size=(12, 13, 14)), AC.blob_noise((24, 24, 24), 2), np.where(rng.uniform(size=(10, 10, 10)) < 0.5, 0.0, rng.normal(size=(10, 10, 10))),
               rng.uniform(size=(9, 9, 9)) ** 4]
    for c in AC.fixture_cases()[::4]:
        volumes.append(c[2])
    for V in volumes:
        flat = V.ravel()
        hmin, hmax = float(flat.min()), float(flat.max())
        counts = AC.counts_by_edges(flat[flat != 0], np.linspace(hmin, hmax, 257))
        want = T.otsu_threshold_eman(V)
        assert T.otsu_from_counts(counts, hmin, hmax) == want
        thr = C.c_double(0.0)
        c64 = np.ascontiguousarray(counts, dtype=np.int64)
        assert _lib.lib().hh_am_otsu(c64.ctypes.data_as(C.POINTER(C.c_int64)), hmin, hmax, None, C.byref(thr)) == 0 and thr.value == want
    assert T.otsu_from_counts(np.zeros(256), -1.0, 2.0) == -1.0 and H.otsu_from_counts is T.otsu_from_counts


def test_all_ties_composition_equals_the_recorded_masks():
    n_ge = {}
    for k, j, avg, apix, cutoff, mode, want in AC.fixture_cases():
        mask, LP, thresh, v_star, ge = AC.adaptive_mask_numpy(avg, apix, cutoff, **mode)
        assert mask.dtype == np.uint8 and np.array_equal(mask, want), (k, j)
        assert np.array_equal(T.adaptive_mask(avg, apix, cutoff, **mode), want)
        fig = AC.check_margins(avg, apix, cutoff, want, **mode)
        n_ge[k] = ge
        if fig["B"] > 0:                                                  # the filtered case: far from every tie
            for key in ("to_threshold", "to_edge", "rank_gap", "seed_gap"):
                assert fig.get(key) is None or fig[key] >= 1e7 * fig["B"], (k, j, key, fig)
    assert n_ge == {0: 1020, 1: 1000}                                     # case 0 (unfiltered) holds ties at v*
    assert not cutoff_filters(0) and cutoff_filters(1)


def cutoff_filters(k):
    c = [c for c in AC.fixture_cases() if c[0] == k][0]
    return c[4] > 2 * c[3]


def test_synthetic_cases_meet_their_margins_and_show_what_they_are_for():
    for name, V, apix, cutoff, mode in AC.synthetic_cases():
        host = T.adaptive_mask(V, apix, cutoff, **mode)
        fig = AC.check_margins(V, apix, cutoff, host, **mode)
        mine, LP, thresh, v_star, ge = AC.adaptive_mask_numpy(V, apix, cutoff, **mode)
        assert np.array_equal(mine, host != 0), name
        above = LP > thresh
        n_comp = AC.scipy_labels(above)[1]
        if name == "bright+dim-value":
            assert n_comp >= 2 and 0 < host.sum() < above.sum() and host[33, 33, 33] == 0 and above[33, 33, 33]
        if name == "two-blobs-fraction":
            assert n_comp == 2 and host.sum() == above.sum() and host[11, 12, 12] == 1 and host[29, 28, 29] == 1
        if name == "above-the-maximum":
            assert not above.any() and not host.any()
        assert fig["B"] > 0


def test_label_case_builders():
    cases = dict(AC.label_cases())
    assert AC.scipy_labels(cases["corner"])[1] == 1 and AC.scipy_labels(cases["edge"])[1] == 1
    from scipy.ndimage import label

    assert label(cases["corner"])[1] == 2 and label(cases["edge"])[1] == 2          # 6-connectivity: two
    assert AC.scipy_labels(cases["checkerboard"])[1] == 1 and label(cases["checkerboard"])[1] == int(cases["checkerboard"].sum())
    assert AC.scipy_labels(cases["serpentine"])[1] == 1 and cases["serpentine"].sum() > 24 * 6 * 64
    assert label(cases["serpentine"])[1] == 1                                       # a path even under 6-connectivity: one voxel wide
    assert AC.scipy_labels(cases["comb"])[1] == 1 and AC.scipy_labels(cases["comb"][:, :, :-1])[1] > 20
    assert AC.scipy_labels(cases["helix"])[1] == 1 and cases["helix"].any(axis=(1, 2)).all()
    assert AC.scipy_labels(cases["1x1x130"])[1] == 5
    lab = np.array([[[0, 5, 5, 0, 2, 0, 5]]])
    assert np.array_equal(AC.canonical(lab), [[[0, 1, 1, 0, 2, 0, 1]]])


def test_entry_points_in_header_exports_library_and_source():
    hdr = (ROOT / "include" / "helicon_hip.h").read_text()
    declared = set(re.findall(r"^\s*int\s+(hh_\w+)\s*\(", hdr, flags=re.M))
    assert ENTRY_POINTS <= declared and ENTRY_POINTS <= set(_lib.EXPORTS)
    assert {n for n in declared if n.startswith("hh_am_")} == ENTRY_POINTS == {n for n in _lib.EXPORTS if n.startswith("hh_am_")}
    L = _lib.lib()
    for name in ENTRY_POINTS:
        assert hasattr(L, name)
    text = (ROOT / "helicon_amd" / "csrc" / "adaptive_mask.inc").read_text()
    found = re.findall(r'^extern "C" int (hh_\w+)\([^;{]*\)\s*(try)?\s*\{', text, re.M)
    assert dict(found) == {name: "try" for name in ENTRY_POINTS}        # function-try-blocks: the exception barrier
    unit = (ROOT / "helicon_amd" / "csrc" / "helicon_hip.hip").read_text()
    assert unit.index('soft_mask.inc"') < unit.index('adaptive_mask.inc"')
    for name in ("gaussian_taps", "gaussian_filter_device", "label_components", "otsu_from_counts", "adaptive_mask_device"):
        assert getattr(H, name) is getattr(T, name) and name in T.__all__
    assert callable(H.TrueFSC.adaptive_support) and callable(H.TrueFSC.support)


def test_argument_refusals_of_the_library_need_no_gpu():
    L = _lib.lib()
    u8p, i32p, f64p, i64p = (C.POINTER(t) for t in (C.c_uint8, C.c_int32, C.c_double, C.c_int64))
    vol, out = np.zeros(10**3), np.zeros(10**3)
    sup, roots, taps, info = np.zeros(10**3, np.uint8), np.zeros(10**3, np.int32), T.gaussian_taps(1.0), np.zeros(16)
    count = C.c_int64(0)
    pv, po, ps, pr, pt, pi = vol.ctypes.data_as(f64p), out.ctypes.data_as(f64p), sup.ctypes.data_as(u8p), roots.ctypes.data_as(i32p), taps.ctypes.data_as(f64p), info.ctypes.data_as(f64p)
    vv = vol.ctypes.data_as(C.c_void_p)
    fake = C.c_void_p(1)      # never dereferenced: these checks come first
    nan, inf = float("nan"), float("inf")
    cases = [
        (lambda: L.hh_am_gaussian_3d(0, None, 10, 10, 10, 1.0, pt, po), b"hh_am_gaussian_3d", b"NULL"),
        (lambda: L.hh_am_gaussian_3d(0, pv, 10, 10, 10, 1.0, None, po), b"hh_am_gaussian_3d", b"NULL"),
        (lambda: L.hh_am_gaussian_3d(0, pv, 10, 10, 10, 1.0, pt, None), b"hh_am_gaussian_3d", b"NULL"),
        (lambda: L.hh_am_gaussian_3d(0, pv, 0, 10, 10, 1.0, pt, po), b"hh_am_gaussian_3d", b"[1, 1024]"),
        (lambda: L.hh_am_gaussian_3d(0, pv, 10, 1025, 10, 1.0, pt, po), b"hh_am_gaussian_3d", b"[1, 1024]"),
        (lambda: L.hh_am_gaussian_3d(0, pv, 1024, 1024, 1024, 1.0, pt, po), b"hh_am_gaussian_3d", b"2^28"),
        (lambda: L.hh_am_gaussian_3d(0, pv, 10, 10, 10, nan, pt, po), b"hh_am_gaussian_3d", b"sigma"),
        (lambda: L.hh_am_gaussian_3d(0, pv, 10, 10, 10, 0.0, pt, po), b"hh_am_gaussian_3d", b"sigma"),
        (lambda: L.hh_am_gaussian_3d(0, pv, 10, 10, 10, 1025.0, pt, po), b"hh_am_gaussian_3d", b"4096"),
        (lambda: L.hh_am_label_3d(0, None, 10, 10, 10, pr, C.byref(count)), b"hh_am_label_3d", b"NULL"),
        (lambda: L.hh_am_label_3d(0, ps, 10, 10, 10, None, C.byref(count)), b"hh_am_label_3d", b"NULL"),
        (lambda: L.hh_am_label_3d(0, ps, 10, 10, 10, pr, None), b"hh_am_label_3d", b"NULL"),
        (lambda: L.hh_am_label_3d(0, ps, 10, 10, 1025, pr, C.byref(count)), b"hh_am_label_3d", b"[1, 1024]"),
        (lambda: L.hh_am_label_3d(0, ps, 1024, 1024, 512, pr, C.byref(count)), b"hh_am_label_3d", b"2^28"),
        (lambda: L.hh_am_mask_3d(0, None, 1, 10, 10, 10, 1.0, pt, 0, 0.0, ps, pi), b"hh_am_mask_3d", b"NULL"),
        (lambda: L.hh_am_mask_3d(0, vv, 1, 10, 10, 10, 1.0, pt, 0, 0.0, None, pi), b"hh_am_mask_3d", b"NULL"),
        (lambda: L.hh_am_mask_3d(0, vv, 1, 10, 10, 10, 1.0, None, 0, 0.0, ps, pi), b"hh_am_mask_3d", b"NULL taps"),
        (lambda: L.hh_am_mask_3d(0, vv, 1, 10, 0, 10, 0.0, None, 0, 0.0, ps, pi), b"hh_am_mask_3d", b"[1, 1024]"),
        (lambda: L.hh_am_mask_3d(0, vv, 1, 1024, 1024, 257, 0.0, None, 0, 0.0, ps, pi), b"hh_am_mask_3d", b"2^28"),
        (lambda: L.hh_am_mask_3d(0, vv, 1, 9, 10, 11, 0.0, None, 0, 0.0, ps, pi), b"hh_am_mask_3d", b"fewer than 1000"),
        (lambda: L.hh_am_mask_3d(0, vv, 1, 10, 10, 10, nan, pt, 0, 0.0, ps, pi), b"hh_am_mask_3d", b"sigma"),
        (lambda: L.hh_am_mask_3d(0, vv, 1, 10, 10, 10, -1.0, pt, 0, 0.0, ps, pi), b"hh_am_mask_3d", b"sigma"),
        (lambda: L.hh_am_mask_3d(0, vv, 1, 10, 10, 10, 1.0, pt, 4, 0.0, ps, pi), b"hh_am_mask_3d", b"unknown mode"),
        (lambda: L.hh_am_mask_3d(0, vv, 1, 10, 10, 10, 1.0, pt, -1, 0.0, ps, pi), b"hh_am_mask_3d", b"unknown mode"),
        (lambda: L.hh_am_mask_3d(0, vv, 1, 10, 10, 10, 1.0, pt, 2, nan, ps, pi), b"hh_am_mask_3d", b"NaN or infinite"),
        (lambda: L.hh_am_mask_3d(0, vv, 1, 10, 10, 10, 1.0, pt, 3, 1000.0, ps, pi), b"hh_am_mask_3d", b"rank"),
        (lambda: L.hh_am_mask_3d(0, vv, 1, 10, 10, 10, 1.0, pt, 3, 2.5, ps, pi), b"hh_am_mask_3d", b"rank"),
        (lambda: L.hh_am_context_support(None, 1, 1.0, pt, 0, 0.0, pi), b"hh_am_context_support", b"NULL"),
        (lambda: L.hh_am_context_support(fake, 1, nan, pt, 0, 0.0, pi), b"hh_am_context_support", b"sigma"),
        (lambda: L.hh_am_context_support(fake, 1, 1.0, None, 0, 0.0, pi), b"hh_am_context_support", b"NULL taps"),
        (lambda: L.hh_am_context_support(fake, 1, 1.0, pt, 7, 0.0, pi), b"hh_am_context_support", b"unknown mode"),
        (lambda: L.hh_am_context_support(fake, 1, 1.0, pt, 1, inf, pi), b"hh_am_context_support", b"NaN or infinite"),
        (lambda: L.hh_am_context_get_support(None, 0, ps), b"hh_am_context_get_support", b"NULL"),
        (lambda: L.hh_am_context_get_support(fake, 0, None), b"hh_am_context_get_support", b"NULL"),
        (lambda: L.hh_am_context_get_support(fake, 2, ps), b"hh_am_context_get_support", b"which"),
        (lambda: L.hh_am_otsu(None, 0.0, 1.0, None, po), b"hh_am_otsu", b"NULL"),
        (lambda: L.hh_am_otsu(np.zeros(256, np.int64).ctypes.data_as(i64p), 1.0, 0.0, None, po), b"hh_am_otsu", b"range"),
    ]
    for call, name, word in cases:
        assert call() == -1   # HH_ERR_ARG
        msg = L.hh_last_error(None)
        assert msg.startswith(name) and word in msg, msg
    ms = np.ones(8)
    assert L.hh_am_stage_ms(ms.ctypes.data_as(f64p), 1) == 0 and (ms >= 0).all()


class _NoDevice:
    def __getattr__(self, name):
        raise AssertionError(f"the device was reached: {name}")


def test_python_refusals_come_before_any_device_call(monkeypatch):
    monkeypatch.setattr(_lib, "lib", lambda: _NoDevice())
    V = AC.volume((10, 10, 10), 1)
    for fn in (lambda v: T.gaussian_filter_device(v, 1.0), lambda v: T.adaptive_mask_device(v, 1.0, 8.0)):
        for bad in (np.zeros((8, 8)), np.zeros((0, 8, 8)), np.broadcast_to(0.0, (8, 8, 1025))):
            with pytest.raises(ValueError, match="3-D volume"):
                fn(bad)
        for poison in (np.nan, np.inf):
            W = V.copy()
            W[3, 4, 5] = poison
            with pytest.raises(ValueError, match="NaN or infinite"):
                fn(W)
    with pytest.raises(ValueError, match="gaussian_taps"):
        T.gaussian_filter_device(V, float("nan"))
    with pytest.raises(ValueError, match="at least 1000"):
        T.adaptive_mask_device(V[:9], 1.0, 8.0)
    with pytest.raises(ValueError, match="constant volume"):
        T.adaptive_mask_device(np.full((10, 10, 10), 2.5), 1.0, 0.0)
    with pytest.raises(ValueError, match="apix"):
        T.adaptive_mask_device(V, 0.0, 8.0)
    with pytest.raises(ValueError, match="3-D support"):
        T.label_components(np.zeros((4, 4)))
    ctx = object.__new__(T.TrueFSC)
    ctx.n, ctx.apix, ctx.cutoff_res, ctx._ctx = 8, 2.0, 8.0, _NoDevice()
    with pytest.raises(ValueError, match="at least 1000"):
        ctx.adaptive_support()
    with pytest.raises(ValueError, match="no support"):
        ctx.support()
    with pytest.raises(ValueError, match="which"):
        ctx.support(2)
    # the mode and its argument, in adaptive_mask's precedence
    assert T._mask_mode(4096, 2.0, 8.0, 0.3, 0.5, 40.0, "t")[2:] == (1, 0.3)
    assert T._mask_mode(4096, 2.0, 8.0, 0, 0.5, 40.0, "t")[2:] == (2, 0.5)
    assert T._mask_mode(4096, 2.0, 8.0, 0, 0, 1.0, "t")[2:] == (3, float(int(1e3 / (0.81 * 8.0))))
    assert T._mask_mode(4096, 2.0, 8.0, 0, 0, 1e6, "t")[2:] == (3, 4095.0)
    sigma, taps, mode, value = T._mask_mode(4096, 2.0, 8.0, 0, 0, 0, "t")
    assert sigma == 8.0 / (3.81 * 2.0) and np.array_equal(taps, T.gaussian_taps(sigma)) and (mode, value) == (0, 0.0)
    assert T._mask_mode(4096, 2.0, 4.0, 0, 0, 0, "t")[:2] == (0.0, None)                # cutoff <= 2 apix: no filter


class SupportOracle(SC.HostSoftOracle):
    """The stand-in with adaptive_support: the supports come from the NumPy composition (all ties), never from adaptive_mask."""

    def adaptive_support(self, one_mask=False, **kw):
        type(self).log.append(("adaptive_support", bool(one_mask), tuple(sorted(kw.items()))))
        vols = [(self.a + self.b) / 2] if one_mask else [self.a, self.b]
        self._sup = [AC.adaptive_mask_numpy(v, self.apix, self.cutoff_res, **kw)[0] != 0 for v in vols]


def test_true_fsc_device_support_with_a_stand_in_context(monkeypatch):
    import fsc_oracle as O

    n = 24
    a, b = O.make_map_pair(n, 77, dc="auto")
    g = np.arange(n) - n // 2
    blob = 6.0 * np.exp(-(g[:, None, None] ** 2 + g[None, :, None] ** 2 + g[None, None, :] ** 2) / 30.0)
    a, b = (a + blob).astype(np.float32), (b + blob).astype(np.float32)
    rng = np.random.RandomState(3)
    u = tuple(rng.uniform(0, 2 * np.pi, size=(n, n, n // 2 + 1)) for _ in range(2))
    kw = dict(cutoff_res=8.0, phases=u, context=SupportOracle, mask_soft=6.0, device_masks=True)
    SupportOracle.log = []
    host = T.true_fsc(a, b, 2.0, one_mask=True, **kw)
    assert [e[0] for e in SupportOracle.log] == ["set_support", "soft_masked", "soft_mask"] and host["host_mask_s"] > 0

    def boom(*p, **k):
        raise AssertionError("adaptive_mask ran on the host")

    monkeypatch.setattr(T, "adaptive_mask", boom)
    SupportOracle.log = []
    out = T.true_fsc(a, b, 2.0, one_mask=True, device_support=True, **kw)
    assert [e[0] for e in SupportOracle.log] == ["adaptive_support", "soft_masked", "soft_mask"]
    assert SupportOracle.log[0] == ("adaptive_support", True, (("mask_fraction_thresh", 0), ("mask_mass", 0), ("mask_thresh", 0)))
    assert out["host_mask_s"] == 0.0 and out["mask1"] is out["mask2"]
    assert np.array_equal(out["mask1"], host["mask1"])
    for key in ("masked", "randomized_masked", "true"):
        assert np.array_equal(out[key], host[key])
    SupportOracle.log = []
    two = T.true_fsc(a, b, 2.0, device_support=True, mask_fraction_thresh=0.3, **kw)
    assert [e[0] for e in SupportOracle.log] == ["adaptive_support", "soft_masked", "soft_mask", "soft_mask"]
    assert SupportOracle.log[0][1] is False and dict(SupportOracle.log[0][2])["mask_fraction_thresh"] == 0.3
    assert two["host_mask_s"] == 0.0 and two["mask1"] is not two["mask2"]


def test_the_two_value_errors_of_device_support():
    a = np.zeros((16, 16, 16), np.float32)
    with pytest.raises(ValueError, match="device_support needs device_masks"):
        T.true_fsc(a, a, 2.0, cutoff_res=8.0, device_support=True, context=_NoDevice())
    inexact = np.full((16, 16, 16), 0.1)                                  # float64 0.1 is not a float32
    with pytest.raises(ValueError, match="float32 represents exactly"):
        T.true_fsc(inexact, inexact, 2.0, cutoff_res=8.0, device_masks=True, device_support=True, context=_NoDevice())
    args = T.add_args(argparse.ArgumentParser()).parse_args(["h1.mrc", "h2.mrc", "--device-masks", "--device-support"])
    assert args.device_support and args.device_masks
    alone = T.add_args(argparse.ArgumentParser()).parse_args(["h1.mrc", "h2.mrc", "--device-support"])
    with pytest.raises(SystemExit, match="--device-masks"):
        T.run(alone, context=_NoDevice())
    assert not T.add_args(argparse.ArgumentParser()).parse_args(["h1.mrc", "h2.mrc"]).device_support
