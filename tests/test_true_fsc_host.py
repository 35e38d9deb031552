"""Host side of the phase-randomised true FSC (no GPU): the float64 restatement and the package's host helpers against the
reference's recorded output (tests/golden/g20_true_fsc.npz), the cutoff rules, the C ABI's new entry points and their
refusals, and the command line with a stand-in for the resident context."""
import argparse
import ctypes as C
import importlib
import json
import re
from pathlib import Path

import numpy as np
import pytest

import fsc_oracle as O
import true_fsc_oracle as TO
import helicon_amd as H
from helicon_amd import _lib

T = importlib.import_module("helicon_amd.true_fsc")

ROOT = Path(__file__).resolve().parents[1]
ENTRY_POINTS = {"hh_tfsc_create", "hh_tfsc_curves", "hh_tfsc_download", "hh_tfsc_masked", "hh_tfsc_destroy"}


@pytest.fixture(scope="module")
def g20(golden_dir):
    return np.load(golden_dir / "g20_true_fsc.npz")


def _case(g20, k):
    n, seed, cutoff, apix, rseed = g20[f"c{k}_par"]
    a, b = g20[f"c{k}_a"].astype(np.float32), g20[f"c{k}_b"].astype(np.float32)
    n = int(n)
    np.random.seed(int(rseed))
    shape = (n, n, n // 2 + 1)
    u1, u2 = np.random.uniform(0, 2 * np.pi, size=shape), np.random.uniform(0, 2 * np.pi, size=shape)
    return n, float(cutoff), float(apix), int(rseed), a, b, u1, u2


def test_the_draws_are_numpys_frozen_stream(g20):
    n, cutoff, apix, rseed, a, b, u1, u2 = _case(g20, 0)
    assert np.array_equal(u1, g20["c0_u1"]) and np.array_equal(u2, g20["c0_u2"])
    n, cutoff, apix, rseed, a, b, u1, u2 = _case(g20, 1)
    assert np.array_equal(u1.ravel()[:64], g20["c1_u1_head"]) and np.array_equal(u2.ravel()[:64], g20["c1_u2_head"])


def test_restatement_of_randomize_phases_lowpass_equals_the_reference(g20):
    """In the input's own precision the restatement is the reference's output bit for bit; in float64 with the integer rule (the
    GPU tests' form) it differs from it by single-precision rounding only."""
    for k in range(int(g20["n_cases"][0])):
        n, cutoff, apix, rseed, a, b, u1, u2 = _case(g20, k)
        mine = TO.randomize_phases_lowpass(a, apix, cutoff, True, u1)
        assert mine.dtype == np.complex64
        want = g20[f"c{k}_rpl_fft"]
        assert np.array_equal(mine if k == 0 else mine[:, :, :: n // 4], want)
        m_cut = T.cutoff_m(n, apix, cutoff)
        assert np.array_equal(TO.m_half(n) >= m_cut, TO.reference_cutoff_mask(n, apix, cutoff))       # no tie at these cutoffs
        F64 = TO.randomized_spectrum(a, m_cut, u1)
        got = F64 if k == 0 else F64[:, :, :: n // 4]
        assert np.abs(got - want).max() <= 2e-6 * np.abs(want).max()
        if k == 0:
            assert np.array_equal(TO.randomize_phases_lowpass(a, apix, cutoff, False, u1), g20["c0_rpl_map"])
            assert np.abs(TO.irfftn(F64) - g20["c0_rpl_map"]).max() <= 2e-6 * np.abs(g20["c0_rpl_map"]).max()


def test_oracle_composition_equals_the_reference_curves(g20):
    for k in range(int(g20["n_cases"][0])):
        n, cutoff, apix, rseed, a, b, u1, u2 = _case(g20, k)
        ctx = TO.OracleTrueFSC(a, b, apix, cutoff, phases=(u1, u2))
        assert ctx.m_cut == T.cutoff_m(n, apix, cutoff)
        mask = g20[f"c{k}_mask"].astype(np.float64)
        t, nz = ctx.masked(mask)
        for mine, key in ((ctx.unmasked, "unmasked"), (ctx.randomized_unmasked, "rand_unmasked"), (t, "masked"), (nz, "rand_masked")):
            want = g20[f"c{k}_{key}"]
            assert mine.shape == want.shape and np.array_equal(mine[:, 0], want[:, 0])
            assert np.abs(mine[:, 1] - want[:, 1]).max() <= 1e-12, key
        assert np.abs(ctx.true_fsc(mask)[:, 1] - g20[f"c{k}_true"]).max() <= 1e-12
        pt, pn = ctx.masked(mask, per_shell=True)
        assert np.abs(pt - g20[f"c{k}_per_shell_t"]).max() <= 1e-12 and np.abs(pn - g20[f"c{k}_per_shell_n"]).max() <= 1e-12
        assert ctx.cutoff_index == int(n * apix / cutoff)
        # the package's host pieces on the reference's curves
        assert np.array_equal(T.corrected(g20[f"c{k}_masked"][:, 1], g20[f"c{k}_rand_masked"][:, 1], ctx.cutoff_index), g20[f"c{k}_true"])


def test_host_helpers_equal_the_reference(g20):
    for k in range(int(g20["n_cases"][0])):
        n, cutoff, apix, rseed, a, b, u1, u2 = _case(g20, k)
        avg = (a.astype(np.float64) + b.astype(np.float64)) / 2
        assert T.otsu_threshold_eman(avg) == float(g20[f"c{k}_otsu"])
        modes = [dict(), dict(mask_fraction_thresh=0.3), dict(mask_thresh=0.5), dict(mask_mass=40.0)]
        for j, mode in enumerate(modes):
            want = np.unpackbits(g20[f"c{k}_adaptive{j}"])[: n**3].reshape(n, n, n).astype(np.float64)
            got = T.adaptive_mask(avg, apix, cutoff, **mode)
            assert got.dtype == np.float64 and np.array_equal(got, want), (k, j)
            assert 0 < want.sum() < n**3
        s_fit, f_fit, r_fit = T.fit_fsc_curve(g20[f"c{k}_masked"][:, 0], g20[f"c{k}_true"])
        assert np.array_equal(s_fit, g20[f"c{k}_fit_s"]) and np.abs(f_fit - g20[f"c{k}_fit_f"]).max() <= 1e-12
        assert r_fit == pytest.approx(float(g20[f"c{k}_fit_res"]), rel=1e-12)
        un = g20[f"c{k}_unmasked"]
        assert T.choose_cutoff(un[:, 0], un[:, 1]) == float(g20[f"c{k}_cutoff_rule"])
    base = np.unpackbits(g20["c0_adaptive0"])[: 16**3].reshape(16, 16, 16).astype(np.float64)
    for w, width in enumerate(g20["soft_widths"]):
        got = T.soft_mask(base, float(width))
        assert got.dtype == np.float64 and np.abs(got - g20[f"c0_soft{w}"]).max() <= 1e-12
    assert np.array_equal(T.soft_mask(base, 0), base) and ((g20["c0_soft2"] > 0) & (g20["c0_soft2"] < 1)).any()


def test_cutoff_rule_on_hand_made_curves(g20):
    s = g20["rule_saxis"]
    for c, want in zip(g20["rule_curves"], g20["rule_expected"]):
        assert T.choose_cutoff(s, c) == want
    assert len(set(g20["rule_expected"])) >= 4
    c = g20["rule_curves"][0]
    assert T.choose_cutoff(s, c, 7.3) == 7.3 and T.choose_cutoff(s, c, 2.0) == T.choose_cutoff(s, c) == T.choose_cutoff(s, c, 0)
    # each branch of the rounding by hand: 0.8 is crossed between shells whose frequencies are known
    s = np.arange(5) / 100.0
    assert T.choose_cutoff(s, np.array([1, 0.9, 0.7, 0.1, 0])) == round(1.0 / 0.015)                  # 66.7 -> 67
    s = np.arange(5) / 11.0
    assert T.choose_cutoff(s, np.array([1, 0.9, 0.7, 0.1, 0])) == 7.5                                 # 11 / 1.5 = 7.33 -> 7.5
    s = np.arange(5) / 5.0
    assert T.choose_cutoff(s, np.array([1, 0.9, 0.7, 0.1, 0])) == 3.25                                # 5 / 1.5 = 3.33 -> 3.25


def test_integer_cutoff_rule_and_ties():
    # quarter-integer thresholds: no tie, and the reference expression selects the same bins
    for n in (16, 24, 32, 64):
        cutoff = 2.0 * n / (n / 4 + 0.5)
        m_cut = T.cutoff_m(n, 2.0, cutoff)
        assert m_cut == int(np.ceil((n / 4 + 0.5) ** 2)) and np.array_equal(TO.m_half(n) >= m_cut, TO.reference_cutoff_mask(n, 2.0, cutoff))
    # a tie: (apix / cutoff)^2 n^2 is the integer 36 up to rounding, whichever side the float64 product falls on
    assert T.cutoff_m(24, 2.0, 8.0) == 36 and T.cutoff_m(24, 1.1, 4.4) == 36 and T.cutoff_m(24, 0.3, 1.2) == 36
    assert T.cutoff_m(24, 2.0, 8.0001) == 36 and T.cutoff_m(24, 2.0, 7.9999) == 37
    assert T.cutoff_m(24, 2.0, 1e-9) == 2**62           # nothing is randomised
    with pytest.raises(ValueError):
        T.cutoff_m(24, 2.0, 0.0)


def test_entry_points_in_header_exports_and_library():
    hdr = (ROOT / "include" / "helicon_hip.h").read_text()
    declared = set(re.findall(r"^\s*(?:int64_t|int|void|const char\*)\s+(hh_tfsc_\w+)\s*\(", hdr, flags=re.M))
    assert declared == ENTRY_POINTS and ENTRY_POINTS <= set(_lib.EXPORTS)
    L = _lib.lib()
    for name in ENTRY_POINTS:
        assert hasattr(L, name)
    text = (ROOT / "helicon_amd" / "csrc" / "true_fsc.inc").read_text()
    found = re.findall(r'^extern "C" int (hh_\w+)\([^;{]*\)\s*(try)?\s*\{', text, re.M)
    assert dict(found) == {name: "try" for name in ENTRY_POINTS}        # function-try-blocks: the exception barrier
    other = (ROOT / "helicon_amd" / "csrc" / "fourier_correlation.inc").read_text()
    assert "hh_tfsc" not in other
    unit = (ROOT / "helicon_amd" / "csrc" / "helicon_hip.hip").read_text()
    assert unit.index('fourier_correlation.inc"') < unit.index('true_fsc.inc"')
    assert H.TrueFSC is T.TrueFSC and H.randomize_phases_lowpass is T.randomize_phases_lowpass
    assert H.true_fsc is T and callable(T.true_fsc)       # the module keeps its name in the package


def test_argument_refusals_need_no_gpu():
    L = _lib.lib()
    f32p, f64p = C.POINTER(C.c_float), C.POINTER(C.c_double)
    a = np.zeros(16 ** 3, np.float32)
    ph = np.zeros(16 * 16 * 9, np.float64)
    sums = np.zeros(2 * 3 * 300, np.float64)
    pa, pp, ps = a.ctypes.data_as(f32p), ph.ctypes.data_as(f64p), sums.ctypes.data_as(f64p)
    h = C.c_void_p()
    fake = C.c_void_p(1)      # never dereferenced: the argument check comes first
    cases = [
        (lambda: L.hh_tfsc_create(None, 0, pa, pa, 16, 4, None, None, 0), b"hh_tfsc_create", b"NULL"),
        (lambda: L.hh_tfsc_create(C.byref(h), 0, None, pa, 16, 4, None, None, 0), b"hh_tfsc_create", b"NULL"),
        (lambda: L.hh_tfsc_create(C.byref(h), 0, pa, None, 16, 4, None, None, 0), b"hh_tfsc_create", b"NULL"),
        (lambda: L.hh_tfsc_create(C.byref(h), 0, pa, pa, 16, 4, pp, None, 0), b"hh_tfsc_create", b"phases"),
        (lambda: L.hh_tfsc_create(C.byref(h), 0, pa, pa, 15, 4, None, None, 0), b"hh_tfsc_create", b"even"),
        (lambda: L.hh_tfsc_create(C.byref(h), 0, pa, pa, 6, 4, None, None, 0), b"hh_tfsc_create", b"[8, 512]"),
        (lambda: L.hh_tfsc_create(C.byref(h), 0, pa, pa, 514, 4, None, None, 0), b"hh_tfsc_create", b"[8, 512]"),
        (lambda: L.hh_tfsc_create(C.byref(h), 0, pa, pa, 16, -1, None, None, 0), b"hh_tfsc_create", b"m_cut"),
        (lambda: L.hh_tfsc_curves(None, ps), b"hh_tfsc_curves", b"NULL"),
        (lambda: L.hh_tfsc_curves(fake, None), b"hh_tfsc_curves", b"NULL"),
        (lambda: L.hh_tfsc_download(None, 0, pa, None), b"hh_tfsc_download", b"NULL"),
        (lambda: L.hh_tfsc_download(fake, 0, None, None), b"hh_tfsc_download", b"NULL"),
        (lambda: L.hh_tfsc_download(fake, 2, pa, None), b"hh_tfsc_download", b"which"),
        (lambda: L.hh_tfsc_masked(None, pa, None, 1, 0, ps, None), b"hh_tfsc_masked", b"NULL"),
        (lambda: L.hh_tfsc_masked(fake, None, None, 1, 0, ps, None), b"hh_tfsc_masked", b"NULL"),
        (lambda: L.hh_tfsc_masked(fake, pa, None, 1, 0, None, None), b"hh_tfsc_masked", b"NULL"),
        (lambda: L.hh_tfsc_masked(fake, pa, None, 0, 0, ps, None), b"hh_tfsc_masked", b"batch"),
    ]
    for call, name, word in cases:
        assert call() == -1   # HH_ERR_ARG
        msg = L.hh_last_error(None)
        assert msg.startswith(name) and word in msg, msg
        assert not h.value
    assert L.hh_tfsc_destroy(None) == 0


def test_python_refusals_come_before_any_device_call():
    cube = np.zeros((16, 16, 16), np.float32)
    for bad in (np.zeros((15, 15, 15), np.float32), np.broadcast_to(np.float32(0), (520, 520, 520)), np.zeros((6, 6, 6), np.float32),
                np.zeros((16, 16, 12), np.float32), np.zeros((16, 16), np.float32)):
        with pytest.raises(ValueError):
            H.randomize_phases_lowpass(bad, 2.0, 8.0)
        with pytest.raises(ValueError):
            H.TrueFSC(bad, bad, 2.0, 8.0)
    with pytest.raises(ValueError, match="even"):
        H.randomize_phases_lowpass(np.zeros((33, 33, 33), np.float32), 2.0, 8.0)
    with pytest.raises(ValueError, match="one shape"):
        H.TrueFSC(cube, np.zeros((24, 24, 24), np.float32), 2.0, 8.0)
    nan = cube.copy()
    nan[1, 2, 3] = np.nan
    with pytest.raises(ValueError, match="NaN or infinite"):
        H.TrueFSC(nan, cube, 2.0, 8.0)
    with pytest.raises(ValueError, match="NaN or infinite"):
        H.randomize_phases_lowpass(nan, 2.0, 8.0, seed=1)
    with pytest.raises(ValueError, match="not both"):
        H.randomize_phases_lowpass(cube, 2.0, 8.0, phases=np.zeros((16, 16, 9)), seed=1)
    with pytest.raises(ValueError, match="half spectrum"):
        H.randomize_phases_lowpass(cube, 2.0, 8.0, phases=np.zeros((16, 16, 16)))
    with pytest.raises(ValueError, match="positive"):
        H.randomize_phases_lowpass(cube, 2.0, 0.0, seed=1)
    # fsc.py is unchanged: precomputed spectra are still refused
    with pytest.raises(NotImplementedError):
        H.calc_fsc(cube, cube, 2.0, F1=np.zeros((16, 16, 9), np.complex64))


def test_no_gpu_means_loud_failure():
    import torch

    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    cube = np.ones((16, 16, 16), np.float32)
    with pytest.raises(H.HeliconHipError):
        H.randomize_phases_lowpass(cube, 2.0, 8.0, seed=3)
    with pytest.raises(H.HeliconHipError):
        H.TrueFSC(cube, cube, 2.0, 8.0, seed=3)


# ------------------------------------------------------------------------------------------
# true_fsc() and python -m helicon_amd.true_fsc with the oracle standing in for the resident context
# ------------------------------------------------------------------------------------------
class DrawingOracle(TO.OracleTrueFSC):
    """The oracle context with TrueFSC's defaults: the cutoff rule on its own unmasked curve, host draws when no angles come."""

    calls = 0

    def __init__(self, map1, map2, apix, cutoff_res=0, *, phases=None, seed=None, device=0):
        n = np.asarray(map1).shape[0]
        if not cutoff_res > 2:
            rows = O.calc_fsc(map1, map2, apix)
            cutoff_res = T.choose_cutoff(rows[:, 0], rows[:, 1], cutoff_res)
        if phases is None:
            rng = np.random.RandomState(5 if seed is None else seed)
            phases = tuple(rng.uniform(0, 2 * np.pi, size=(n, n, n // 2 + 1)) for _ in range(2))
        super().__init__(map1, map2, apix, cutoff_res, phases=phases)

    def masked(self, *a, **k):
        type(self).calls += 1
        return super().masked(*a, **k)


def test_true_fsc_reproduces_the_reference_curves_from_the_fixture_maps(g20):
    for k in range(int(g20["n_cases"][0])):
        n, cutoff, apix, rseed, a, b, u1, u2 = _case(g20, k)
        out = T.true_fsc(a, b, apix, mask=g20[f"c{k}_mask"].astype(np.float64), cutoff_res=cutoff, phases=(u1, u2), context=DrawingOracle)
        for key, name in (("unmasked", "unmasked"), ("randomized_unmasked", "rand_unmasked"), ("masked", "masked"),
                          ("randomized_masked", "rand_masked")):
            assert np.abs(out[key][:, 1] - g20[f"c{k}_{name}"][:, 1]).max() <= 1e-12
        assert np.abs(out["true"][:, 1] - g20[f"c{k}_true"]).max() <= 1e-12
        assert np.abs(out["true_fit"][:, 1] - g20[f"c{k}_fit_f"]).max() <= 1e-9
        assert out["mask_soft_px"] is None and out["mask2"] is out["mask1"] and out["cutoff_res"] == cutoff
        assert set(out["resolution"]) == {"unmasked", "masked", "true", "true_fit"}
        assert out["resolution"]["true"] == TO.find_resolution(out["true"][:, 0], g20[f"c{k}_true"], 0.143)


def test_true_fsc_mask_modes_with_the_stand_in():
    a, b = O.make_map_pair(24, 77, dc="auto")
    g = np.arange(24) - 12
    blob = 6.0 * np.exp(-(g[:, None, None] ** 2 + g[None, :, None] ** 2 + g[None, None, :] ** 2) / 30.0)
    a, b = (a + blob).astype(np.float32), (b + blob).astype(np.float32)
    out = T.true_fsc(a, b, 2.0, cutoff_res=8.0, mask_soft=6.0, context=DrawingOracle)
    assert out["mask_soft_px"] == 3.0 and out["mask1"] is not out["mask2"] and out["mask1"].shape == (24, 24, 24)
    one = T.true_fsc(a, b, 2.0, cutoff_res=8.0, mask_soft=6.0, one_mask=True, context=DrawingOracle)
    assert one["mask1"] is one["mask2"]
    assert np.array_equal(one["mask1"], T.soft_mask(T.adaptive_mask((a.astype(np.float64) + b) / 2, 2.0, 8.0), 3.0))
    default = T.true_fsc(a, b, 2.0, cutoff_res=8.0, one_mask=True, context=DrawingOracle)
    assert default["mask_soft_px"] == 3 * default["resolution"]["unmasked"] / 2.0
    auto = T.true_fsc(a, b, 2.0, one_mask=True, mask_soft=6.0, context=DrawingOracle)
    assert auto["cutoff_res"] == T.choose_cutoff(auto["unmasked"][:, 0], auto["unmasked"][:, 1])
    DrawingOracle.calls = 0
    ref = T.true_fsc(a, b, 2.0, cutoff_res=8.0, one_mask=True, refine_mask=True, context=DrawingOracle)
    assert 0 < ref["mask_soft_px"] < 8 and DrawingOracle.calls >= 4          # every evaluation is one .masked() call, then the final one
    two = T.true_fsc(a, b, 2.0, cutoff_res=8.0, mask=[one["mask1"], default["mask1"]], one_mask=True, context=DrawingOracle)
    assert np.array_equal(two["mask1"], (one["mask1"] + default["mask1"]) / 2) and two["mask1"] is two["mask2"]
    with pytest.raises(ValueError):
        T.true_fsc(a, b, 2.0, cutoff_res=8.0, mask=[one["mask1"]] * 3, context=DrawingOracle)


def _args(argv):
    return T.add_args(argparse.ArgumentParser()).parse_args(argv)


def test_cli_arguments():
    a = _args(["h1.mrc", "h2.mrc"])
    assert (a.apix, a.mask, a.one_mask, a.cutoff_res, a.mask_soft, a.refine_mask, a.mask_fraction_thresh, a.mask_thresh, a.mask_mass, a.seed,
            a.out_prefix, a.device) == (None, None, False, 0.0, 0.0, False, 0.0, 0.0, 0.0, None, None, 0)
    a = _args(["h1.mrc", "h2.mrc", "--apix", "1.5", "--mask", "m1.mrc", "m2.mrc", "--one-mask", "--cutoff-res", "9", "--mask-soft", "6",
               "--refine-mask", "--mask-mass", "40", "--seed", "3", "--out-prefix", "p", "--device", "1"])
    assert (a.apix, a.mask, a.one_mask, a.cutoff_res, a.mask_soft, a.refine_mask, a.mask_mass, a.seed, a.out_prefix, a.device) == \
        (1.5, ["m1.mrc", "m2.mrc"], True, 9.0, 6.0, True, 40.0, 3, "p", 1)
    with pytest.raises(SystemExit):
        _args(["h1.mrc", "h2.mrc", "--mask-thresh", "1", "--mask-mass", "40"])
    with pytest.raises(SystemExit):
        _args(["h1.mrc"])


def test_cli_report_and_the_six_files_with_a_stand_in(tmp_path, g20):
    from helicon_amd.mrc import read_mrc, write_mrc

    n, cutoff, apix, rseed, a, b, u1, u2 = _case(g20, 1)
    write_mrc(tmp_path / "h1.mrc", a, apix)
    write_mrc(tmp_path / "h2.mrc", b, apix)
    write_mrc(tmp_path / "mask.mrc", g20["c1_mask"].astype(np.float32), apix)
    prefix = tmp_path / "run"
    rep = T.run(_args([str(tmp_path / "h1.mrc"), str(tmp_path / "h2.mrc"), "--mask", str(tmp_path / "mask.mrc"), "--cutoff-res", str(cutoff),
                       "--out-prefix", str(prefix)]), context=DrawingOracle)
    json.dumps(rep)
    assert set(rep) == {"maps", "cutoff_res", "cutoff_index", "mask_soft_px", "saxis", "unmasked", "randomized_unmasked", "masked",
                        "randomized_masked", "true", "resolution"}
    assert rep["maps"]["shape"] == [24, 24, 24] and rep["maps"]["apix"] == apix and rep["cutoff_res"] == cutoff
    # curves that do not see the random draws are the reference's
    assert np.abs(np.asarray(rep["unmasked"]) - g20["c1_unmasked"][:, 1]).max() <= 1e-12
    assert np.abs(np.asarray(rep["masked"]) - g20["c1_masked"][:, 1]).max() <= 1e-12
    for name, key in (("unmasked", "unmasked"), ("randomized-unmasked", "randomized_unmasked"), ("masked", "masked"),
                      ("randomized-masked", "randomized_masked"), ("true", "true")):
        rows = np.loadtxt(f"{prefix}.{name}.txt")
        assert rows.shape == (12, 2) and np.allclose(rows[:, 1], rep[key][1:], rtol=1e-15) and np.allclose(rows[:, 0], rep["saxis"][1:])
    assert np.loadtxt(f"{prefix}.true.fit.txt").shape == (500, 2)
    written, _ = read_mrc(f"{prefix}.common_mask.mrc")
    assert np.array_equal(written, g20["c1_mask"].astype(np.float32))
    # adaptive masks, one per map
    rep = T.run(_args([str(tmp_path / "h1.mrc"), str(tmp_path / "h2.mrc"), "--cutoff-res", "8", "--mask-soft", "4", "--out-prefix", str(prefix)]),
                context=DrawingOracle)
    assert rep["mask_soft_px"] == 2.0 and Path(f"{prefix}.mask1.mrc").exists() and Path(f"{prefix}.mask2.mrc").exists()


def test_cli_refusals(tmp_path):
    np.save(tmp_path / "a.npy", np.zeros((16, 16, 16), np.float32))
    np.save(tmp_path / "b.npy", np.zeros((16, 16, 12), np.float32))
    np.save(tmp_path / "c.npy", np.zeros((15, 15, 15), np.float32))
    np.save(tmp_path / "m.npy", np.zeros((12, 12, 12), np.float32))
    A = str(tmp_path / "a.npy")
    with pytest.raises(SystemExit, match="--apix is required"):
        T.run(_args([A, A]), context=DrawingOracle)
    with pytest.raises(SystemExit, match="two cubic maps"):
        T.run(_args([A, str(tmp_path / "b.npy"), "--apix", "2"]), context=DrawingOracle)
    with pytest.raises(SystemExit, match="even"):
        T.run(_args([str(tmp_path / "c.npy"), str(tmp_path / "c.npy"), "--apix", "2"]), context=DrawingOracle)
    with pytest.raises(SystemExit, match="a mask must have"):
        T.run(_args([A, A, "--apix", "2", "--mask", str(tmp_path / "m.npy")]), context=DrawingOracle)
