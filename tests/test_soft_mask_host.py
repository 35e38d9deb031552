"""Host side of the device soft masks (no GPU): the tap tables the mask kernel reads against scipy.ndimage.zoom(order=1), the
definition composed in NumPy against helicon_amd.true_fsc.soft_mask and the reference's recorded masks
(tests/golden/g20_true_fsc.npz), the new entry points and their refusals, and true_fsc(device_masks=True) with a stand-in for
the resident context."""
import ctypes as C
import importlib
import re
from pathlib import Path

import numpy as np
import pytest

import fsc_oracle as O
import soft_mask_cases as SC
import helicon_amd as H
from helicon_amd import _lib

T = importlib.import_module("helicon_amd.true_fsc")

ROOT = Path(__file__).resolve().parents[1]
ENTRY_POINTS = {"hh_edt_3d", "hh_soft_mask_3d", "hh_soft_mask_taps", "hh_tfsm_set_support", "hh_tfsm_soft_mask", "hh_tfsm_soft_masked"}


def _interp(data, taps, outside_rule=True):
    i0, i1, w0, w1, outside = taps
    out = w0 * data[i0] + w1 * data[i1]
    if outside_rule:
        out[outside] = 0.0
    return out


def test_tap_tables_equal_zoom_for_every_side_and_step():
    """The census: every side 2 ... 1024, every step 1 ... max(1, side // 12), random data in (0, 50]."""
    from scipy.ndimage import zoom

    rng = np.random.RandomState(7)
    cases = worst = 0
    quirk_sides = set()
    for n in range(2, 1025):
        for step in range(1, max(1, n // 12) + 1):
            m = -(-n // step)
            data = 50.0 - rng.uniform(0, 50, size=m)            # never 0: a zero in the output is zoom's "outside"
            want = zoom(data, n / m, order=1)
            assert want.shape == (n,)
            taps = T.zoom_taps(n, m)
            got = _interp(data, taps)
            assert np.array_equal(got == 0, want == 0), (n, step)
            worst = max(worst, float(np.abs(got - want).max()))
            if taps[4].any():
                assert list(np.flatnonzero(taps[4])) == [n - 1], (n, step)      # always the last index, and only it
                plain = _interp(data, taps, outside_rule=False)
                assert abs(plain[n - 1] - data[m - 1]) <= 1e-12 and want[n - 1] == 0        # without the rule: wrong by a whole tap value
                quirk_sides.add(n)
            cases += 1
    print(f"SOFT_MASK_FIGURE census cases={cases} max_err={worst:.3e} sides_with_an_outside_last_index={len(quirk_sides)}")
    assert cases == 43275 and worst <= 1e-12
    assert {44, 80, 102, 140, 142, 150} <= quirk_sides
    assert T.zoom_taps(44, 15)[4][43] and not T.zoom_taps(44, 15)[4][:43].any()
    for n, m in ((1, 1), (5, 5), (7, 1)):
        i0, i1, w0, w1, outside = T.zoom_taps(n, m)
        assert not outside.any() and np.array_equal(w0 * np.arange(m)[i0] + w1 * np.arange(m)[i1], np.arange(n) * ((m - 1) / max(n - 1, 1)))


def test_integer_transform_equals_scipys():
    from scipy.ndimage import distance_transform_edt

    for shape, centre, r2 in SC.BOXES:
        S = SC.ellipsoid(shape, centre, r2)
        for s in (1, 2, 3):
            ds = S[::s, ::s, ::s] != 0
            assert np.array_equal(SC.edt_sq(ds), np.rint(distance_transform_edt(~ds) ** 2).astype(np.int64))


def test_numpy_composition_equals_soft_mask_and_the_reference(golden_dir):
    margins = []
    for shape, centre, r2 in SC.BOXES:
        S = SC.ellipsoid(shape, centre, r2)
        for w in SC.WIDTHS:
            soft, dist = SC.soft_mask_numpy(S, w)
            margin = float(np.abs(dist[S == 0] - w).min())
            margins.append(margin)
            assert margin >= SC.TIE                                   # no tie: every voxel is compared
            want = T.soft_mask(S, w)
            assert np.abs(soft - want).max() <= 1e-12, (shape, w)
            assert np.array_equal(soft == 0, want == 0) and np.array_equal(soft == 1, want == 1)
    print(f"SOFT_MASK_FIGURE tie margins min={min(margins):.3e} max={max(margins):.3e}")
    assert 4.2e-4 <= min(margins) and max(margins) <= 5.1e-2
    # the last-plane quirk and the interpolated zeros the GPU tests rely on
    S = SC.cube_support(44)
    soft = T.soft_mask(S, 13.7)
    for plane, sup in ((soft[-1], S[-1]), (soft[:, -1], S[:, -1]), (soft[:, :, -1], S[:, :, -1])):
        assert int(((plane == 1) & (sup == 0)).sum()) == 1936
    for shape in ((24, 24, 24), (20, 27, 33)):
        b = [c for c in SC.BOXES if c[0] == shape][0]
        S = SC.ellipsoid(*b)
        assert ((SC.distance(S, 13.7) == 0) & (S == 0)).any()
    # the reference's recorded masks
    g = np.load(golden_dir / "g20_true_fsc.npz")
    base = np.unpackbits(g["c0_adaptive0"])[: 16**3].reshape(16, 16, 16)
    for k, width in enumerate(g["soft_widths"]):
        if float(width) <= 0:
            continue
        soft, dist = SC.soft_mask_numpy(base, float(width))
        keep = ~((base == 0) & (np.abs(dist - float(width)) < SC.TIE))
        assert keep.mean() > 0.99 and np.abs(soft - g[f"c0_soft{k}"])[keep].max() <= 1e-12


def test_entry_points_in_header_exports_and_library():
    hdr = (ROOT / "include" / "helicon_hip.h").read_text()
    declared = set(re.findall(r"^\s*int\s+(hh_\w+)\s*\(", hdr, flags=re.M))
    assert ENTRY_POINTS <= declared and ENTRY_POINTS <= set(_lib.EXPORTS)
    L = _lib.lib()
    for name in ENTRY_POINTS:
        assert hasattr(L, name)
    text = (ROOT / "helicon_amd" / "csrc" / "soft_mask.inc").read_text()
    found = re.findall(r'^extern "C" int (hh_\w+)\([^;{]*\)\s*(try)?\s*\{', text, re.M)
    assert dict(found) == {name: "try" for name in ENTRY_POINTS}        # function-try-blocks: the exception barrier
    unit = (ROOT / "helicon_amd" / "csrc" / "helicon_hip.hip").read_text()
    assert unit.index('true_fsc.inc"') < unit.index('soft_mask.inc"')
    assert "atomic" not in re.sub(r"//[^\n]*", "", text)
    assert H.distance_transform_edt_sq is T.distance_transform_edt_sq and H.soft_mask_device is T.soft_mask_device
    for name in ("set_support", "soft_mask", "soft_masked", "soft_masked_batch"):
        assert callable(getattr(H.TrueFSC, name))


def test_argument_refusals_of_the_library_need_no_gpu():
    L = _lib.lib()
    u8p, i32p, f32p, f64p = (C.POINTER(t) for t in (C.c_uint8, C.c_int32, C.c_float, C.c_double))
    sup = np.ones(8**3, np.uint8)
    d2, mask, w, sums = np.zeros(8**3, np.int32), np.zeros(8**3, np.float32), np.array([2.0, np.nan]), np.zeros(2 * 2 * 5 * 3)
    ps, pd, pm, pw, pq = sup.ctypes.data_as(u8p), d2.ctypes.data_as(i32p), mask.ctypes.data_as(f32p), w.ctypes.data_as(f64p), sums.ctypes.data_as(f64p)
    fake = C.c_void_p(1)      # never dereferenced: the argument check comes first
    nan, inf = float("nan"), float("inf")
    cases = [
        (lambda: L.hh_edt_3d(0, None, 8, 8, 8, 1, pd, None), b"hh_edt_3d", b"NULL"),
        (lambda: L.hh_edt_3d(0, ps, 8, 8, 8, 1, None, None), b"hh_edt_3d", b"NULL"),
        (lambda: L.hh_edt_3d(0, ps, 0, 8, 8, 1, pd, None), b"hh_edt_3d", b"[1, 1024]"),
        (lambda: L.hh_edt_3d(0, ps, 8, 8, 1025, 1, pd, None), b"hh_edt_3d", b"[1, 1024]"),
        (lambda: L.hh_edt_3d(0, ps, 8, 8, 8, 0, pd, None), b"hh_edt_3d", b"stride"),
        (lambda: L.hh_soft_mask_3d(0, None, 8, 8, 8, 2.0, pm, None), b"hh_soft_mask_3d", b"NULL"),
        (lambda: L.hh_soft_mask_3d(0, ps, 8, 8, 8, 2.0, None, None), b"hh_soft_mask_3d", b"NULL"),
        (lambda: L.hh_soft_mask_3d(0, ps, 8, 1025, 8, 2.0, pm, None), b"hh_soft_mask_3d", b"[1, 1024]"),
        (lambda: L.hh_soft_mask_3d(0, ps, 8, 8, 8, nan, pm, None), b"hh_soft_mask_3d", b"NaN or infinite"),
        (lambda: L.hh_soft_mask_3d(0, ps, 8, 8, 8, inf, pm, None), b"hh_soft_mask_3d", b"NaN or infinite"),
        (lambda: L.hh_soft_mask_taps(8, 9, pd, pd, pq, pq, pd), b"hh_soft_mask_taps", b"m <= n"),
        (lambda: L.hh_soft_mask_taps(8, 4, None, pd, pq, pq, pd), b"hh_soft_mask_taps", b"NULL"),
        (lambda: L.hh_tfsm_set_support(None, ps, None), b"hh_tfsm_set_support", b"NULL"),
        (lambda: L.hh_tfsm_set_support(fake, None, ps), b"hh_tfsm_set_support", b"NULL"),
        (lambda: L.hh_tfsm_soft_mask(None, 0, 2.0, pm), b"hh_tfsm_soft_mask", b"NULL"),
        (lambda: L.hh_tfsm_soft_mask(fake, 0, 2.0, None), b"hh_tfsm_soft_mask", b"NULL"),
        (lambda: L.hh_tfsm_soft_mask(fake, 2, 2.0, pm), b"hh_tfsm_soft_mask", b"which"),
        (lambda: L.hh_tfsm_soft_mask(fake, 0, nan, pm), b"hh_tfsm_soft_mask", b"NaN or infinite"),
        (lambda: L.hh_tfsm_soft_masked(None, pw, 1, 0, pq, None), b"hh_tfsm_soft_masked", b"NULL"),
        (lambda: L.hh_tfsm_soft_masked(fake, None, 1, 0, pq, None), b"hh_tfsm_soft_masked", b"NULL"),
        (lambda: L.hh_tfsm_soft_masked(fake, pw, 1, 0, None, None), b"hh_tfsm_soft_masked", b"NULL"),
        (lambda: L.hh_tfsm_soft_masked(fake, pw, 0, 0, pq, None), b"hh_tfsm_soft_masked", b"batch"),
        (lambda: L.hh_tfsm_soft_masked(fake, pw, 2, 0, pq, None), b"hh_tfsm_soft_masked", b"NaN or infinite"),
    ]
    for call, name, word in cases:
        assert call() == -1   # HH_ERR_ARG
        msg = L.hh_last_error(None)
        assert msg.startswith(name) and word in msg, msg
    # a width <= 0 is the support as 0 / 1 and touches no device
    sup[:100] = 0
    assert L.hh_soft_mask_3d(0, ps, 8, 8, 8, 0.0, pm, None) == 0 and np.array_equal(mask, sup.astype(np.float32))


class _NoDevice:
    def __getattr__(self, name):
        raise AssertionError(f"the device was reached: {name}")


def test_python_refusals_come_before_any_device_call(monkeypatch):
    S = SC.cube_support(24)
    lonely = np.zeros((24, 24, 24), np.uint8)
    lonely[5, 7, 9] = 1                                               # odd indices: nothing is left at step 2
    monkeypatch.setattr(_lib, "lib", lambda: _NoDevice())
    for bad in (np.zeros((8, 8), np.uint8), np.zeros((0, 8, 8), np.uint8), np.broadcast_to(np.uint8(1), (8, 8, 1025))):
        with pytest.raises(ValueError, match="3-D support"):
            T.soft_mask_device(bad, 2.0)
        with pytest.raises(ValueError, match="3-D support"):
            T.distance_transform_edt_sq(bad)
    for w in (float("nan"), float("inf")):
        with pytest.raises(ValueError, match="NaN or infinite"):
            T.soft_mask_device(S, w)
    with pytest.raises(ValueError, match="step 2"):
        T.soft_mask_device(lonely, 9.3)
    with pytest.raises(ValueError, match="step 2"):
        T.distance_transform_edt_sq(lonely, 2)
    with pytest.raises(ValueError, match="step 1"):
        T.distance_transform_edt_sq(np.zeros((4, 4, 4)))
    with pytest.raises(ValueError, match="stride"):
        T.distance_transform_edt_sq(S, 0)
    with pytest.raises(ValueError, match="NaN or infinite"):
        T.soft_mask_device(np.full((4, 4, 4), np.nan), 2.0)
    assert np.array_equal(T.soft_mask_device(S, 0), S.astype(np.float32)) and T.soft_mask_device(S, -1.0).dtype == np.float32
    ctx = object.__new__(T.TrueFSC)
    ctx.n, ctx._ctx = 24, _NoDevice()
    with pytest.raises(ValueError, match="no support"):
        ctx.soft_masked(2.5)
    with pytest.raises(ValueError, match="shape"):
        ctx.set_support(np.ones((24, 24, 20), np.uint8))
    with pytest.raises(ValueError, match="shape"):
        ctx.set_support(S, np.ones((16, 16, 16), np.uint8))
    ctx._supports = [S, lonely]
    with pytest.raises(ValueError, match="step 2"):
        ctx.soft_masked_batch([2.5, 9.3])
    with pytest.raises(ValueError, match="NaN or infinite"):
        ctx.soft_masked(float("nan"))
    with pytest.raises(ValueError, match="NaN or infinite"):
        ctx.soft_mask(float("inf"))
    with pytest.raises(ValueError, match="which"):
        ctx.soft_mask(2.5, which=2)
    with pytest.raises(ValueError, match="list of widths"):
        ctx.soft_masked_batch([])
    a = np.zeros((16, 16, 16), np.float32)
    with pytest.raises(ValueError, match="device_masks"):
        T.true_fsc(a, a, 2.0, mask=np.ones((16, 16, 16)), cutoff_res=8.0, device_masks=True, context=_NoDevice())


def _blob_pair(n, seed):
    a, b = O.make_map_pair(n, seed, dc="auto")
    g = np.arange(n) - n // 2
    blob = 6.0 * np.exp(-(g[:, None, None] ** 2 + g[None, :, None] ** 2 + g[None, None, :] ** 2) / 30.0)
    return (a + blob).astype(np.float32), (b + blob).astype(np.float32)


def test_true_fsc_device_masks_with_a_stand_in_context():
    n = 24
    a, b = _blob_pair(n, 77)
    rng = np.random.RandomState(3)
    u = tuple(rng.uniform(0, 2 * np.pi, size=(n, n, n // 2 + 1)) for _ in range(2))
    kw = dict(cutoff_res=8.0, phases=u, context=SC.HostSoftOracle)
    support = T.adaptive_mask((a.astype(np.float64) + b) / 2, 2.0, 8.0)

    def run(**more):
        SC.HostSoftOracle.log = []
        out = T.true_fsc(a, b, 2.0, **kw, **more)
        return out, list(SC.HostSoftOracle.log)

    # a given width: one upload, one soft_masked, the masks downloaded, never .masked(array)
    out, log = run(one_mask=True, mask_soft=6.0, device_masks=True)
    assert [e[0] for e in log] == ["set_support", "soft_masked", "soft_mask"] and log[0] == ("set_support", False)
    assert log[1] == ("soft_masked", 3.0, False) and out["mask_soft_px"] == 3.0 and out["mask1"] is out["mask2"]
    assert out["mask1"].dtype == np.float32 and np.array_equal(out["mask1"], T.soft_mask(support, 3.0).astype(np.float32))
    host, hlog = run(one_mask=True, mask_soft=6.0)
    assert [e[0] for e in hlog] == ["masked"]                         # the default path is what it was
    for key in ("masked", "randomized_masked", "true"):
        assert np.abs(out[key][:, 1] - host[key][:, 1]).max() <= 1e-6  # float32 masks against float64 ones
    # two supports
    out, log = run(mask_soft=6.0, device_masks=True)
    assert log[0] == ("set_support", True) and [e[0] for e in log] == ["set_support", "soft_masked", "soft_mask", "soft_mask"]
    assert out["mask1"] is not out["mask2"] and np.array_equal(out["mask2"], T.soft_mask(T.adaptive_mask(b.astype(np.float64), 2.0, 8.0), 3.0).astype(np.float32))
    # the refinement: every trial is one soft_masked(per_shell=True), then the final one
    out, log = run(one_mask=True, refine_mask=True, device_masks=True)
    names = [e[0] for e in log]
    trials = [e for e in log if e[0] == "soft_masked" and e[2]]
    assert names.count("set_support") == 1 and names[0] == "set_support" and "masked" not in names
    assert len(trials) >= 4 and names == ["set_support"] + ["soft_masked"] * (len(trials) + 1) + ["soft_mask"]
    assert log[-2] == ("soft_masked", out["mask_soft_px"], False) and 0 < out["mask_soft_px"] < n / 3
    host, hlog = run(one_mask=True, refine_mask=True)
    assert len(hlog) == len(trials) + 1 and host["host_mask_s"] > out["host_mask_s"] > 0
    # the command line passes the flag through
    import argparse

    args = T.add_args(argparse.ArgumentParser()).parse_args(["h1.mrc", "h2.mrc", "--device-masks"])
    assert args.device_masks and not T.add_args(argparse.ArgumentParser()).parse_args(["h1.mrc", "h2.mrc"]).device_masks
