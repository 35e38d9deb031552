"""The phase-randomised true FSC on the device (hh_tfsc_*; helicon_amd/true_fsc.py) against the float64 restatement of the
reference (tests/true_fsc_oracle.py, pinned to the reference by tests/golden/g20_true_fsc.npz) and against the reference's
recorded curves.

Inputs: ``make_map_pair(n, seed, dc="auto")``; the cutoff makes ``(apix / cutoff)^2 n^2 = (n / 4 + 1/2)^2``, a quarter-integer
for n divisible by 4 (every side here; for n = 4 j + 2 it is the integer (j + 1)^2: tests/true_fsc_sides.py has the rule for those),
so no bin is a tie (asserted: the reference's float64 expression selects the integer rule's bins).  Every pair whose curve is
compared keeps each shell's den1, den2 at least 1e-4 of the strongest shell's (asserted: the unmasked pair, the randomised
pair and both masked pairs), the condition of tests/test_gpu_fsc.py.

Bounds, none of them measured:
* curves that see forward passes only (unmasked, masked, and the randomised-unmasked one, whose bins are the forward passes'
  with one more float32 rounding each): the project's TOL_FSC_3D = 3e-7;
* curves that see forward, inverse and forward passes (randomised-masked, and fsc_t - fsc_n, the numerator of fsc_true, and
  fsc_true against the reference's recorded values): 3 x 3e-7 = 9e-7, the linear sum of that bound over three times the passes;
* the randomised map against float64 irfftn, max |d| / max |map|: 8 x the distance of SciPy's own float32 irfftn from
  float64 on the same spectrum, computed here (8 covers sqrt(n / log2 n), the growth of an n-term product's rounding over an
  FFT's, for n <= 256);
* |F'| against |F|: two float32 roundings, 2^-22.
Every test prints its figures (TFSC_FIGURE) before it asserts.  Measured maxima on an MI355X (profiles/true_fsc.json,
"accuracy"): 3.7e-8 against the 3e-7, 5.8e-8 against the 9e-7 (1.4e-7 in the end-to-end run), 7.4e-7 against the map's 1.3e-6 ...
1.8e-6, 5.9e-8 against 2^-22."""
import importlib

import numpy as np
import pytest

import fsc_oracle as O
import true_fsc_oracle as TO
import helicon_amd as H

T = importlib.import_module("helicon_amd.true_fsc")

pytestmark = pytest.mark.gpu

TOL_FSC_3D = 3e-7
TOL_ROUND_TRIP = 9e-7
FLOOR = 1e-4
APIX = 2.0
SIDES = (24, 32, 64, 128)


def _cutoff(n):
    return APIX * n / (n / 4 + 0.5)


def _inputs(n, seed=None):
    a, b = O.make_map_pair(n, 3000 + n if seed is None else seed, dc="auto")
    rng = np.random.RandomState(n)
    shape = (n, n, n // 2 + 1)
    return a, b, (rng.uniform(0, 2 * np.pi, size=shape), rng.uniform(0, 2 * np.pi, size=shape))


def _plain_spectrum(a, b, which):
    """The device's own half spectrum with nothing substituted (m_cut above every bin)."""
    ctx = T._Context(np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32), 2**62, None, None, 0, 0)
    try:
        return ctx.download(which, want_map=False, want_spec=True)[1]
    finally:
        ctx.close()


def _err(got, want):
    return float(np.abs(np.asarray(got) - np.asarray(want)).max())


@pytest.mark.parametrize("n", SIDES)
def test_host_phases_against_float64(n):
    a, b, u = _inputs(n)
    cutoff = _cutoff(n)
    ora = TO.OracleTrueFSC(a, b, APIX, cutoff, phases=u)
    sel = TO.m_half(n) >= ora.m_cut
    assert ora.m_cut == int(np.ceil((n / 4 + 0.5) ** 2)) and np.array_equal(sel, TO.reference_cutoff_mask(n, APIX, cutoff))
    mask = TO.sphere_mask(n, 0.3 * n, 4.0)
    with H.TrueFSC(a, b, APIX, cutoff, phases=u) as dev:
        assert dev.m_cut == ora.m_cut and dev.cutoff_index == ora.cutoff_index == n // 4 and dev.cutoff_res == cutoff
        assert O.floor_ratio(ora.sums[0]) >= FLOOR and O.floor_ratio(ora.sums[1]) >= FLOOR
        # the stored spectrum
        for which, (F, src) in enumerate(((ora.F1r, a), (ora.F2r, b))):
            spec, plain = dev.randomized_map(which, return_fft=True), _plain_spectrum(a, b, which)
            assert spec.dtype == np.complex64 and spec.shape == (n, n, n // 2 + 1)
            assert np.array_equal(spec[~sel].view(np.float32), plain[~sel].view(np.float32))       # untouched below the cutoff
            amp, amp0 = np.abs(spec.astype(np.complex128)), np.abs(plain.astype(np.complex128))
            e_amp = float((np.abs(amp - amp0)[sel] / amp0[sel].clip(1e-30)).max())
            e_spec = float(np.abs(spec - F).max() / np.abs(F).max())
            print(f"TFSC_FIGURE spectrum n={n} map={which} amp_rel={e_amp:.3e} spec_vs_f64={e_spec:.3e} randomised={int(sel.sum())}")
            assert e_amp <= 2.0**-22
            # the inverse transform
            got = dev.randomized_map(which)
            want = ora.ar if which == 0 else ora.br
            from scipy.fft import irfftn

            F32 = F.astype(np.complex64)
            dist = float(np.abs(irfftn(F32) - TO.irfftn(F32)).max() / np.abs(want).max())
            e_map = float(np.abs(got - want).max() / np.abs(want).max())
            print(f"TFSC_FIGURE map_r n={n} map={which} err={e_map:.3e} scipy_f32_dist={dist:.3e} bound={8 * dist:.3e}")
            assert got.dtype == np.float32 and e_map <= 8 * dist
        # curves
        e_un, e_run = _err(dev.unmasked[:, 1], ora.unmasked[:, 1]), _err(dev.randomized_unmasked[:, 1], ora.randomized_unmasked[:, 1])
        assert np.array_equal(dev.unmasked[:, 0], ora.unmasked[:, 0])
        print(f"TFSC_FIGURE unmasked n={n} fsc={e_un:.3e} randomised={e_run:.3e}")
        assert e_un <= TOL_FSC_3D and e_run <= TOL_FSC_3D
        for per_shell in (False, True):
            sums = ora.masked_sums(mask[None], None, per_shell)[0]
            assert O.floor_ratio(sums[0]) >= FLOOR and O.floor_ratio(sums[1]) >= FLOOR
            t, nz = dev.masked(mask, per_shell=per_shell)
            wt, wn = ora.masked(mask, per_shell=per_shell)
            if not per_shell:
                assert np.array_equal(t[:, 0], wt[:, 0])
                t, nz, wt, wn = t[:, 1], nz[:, 1], wt[:, 1], wn[:, 1]
            i = dev.cutoff_index + 1
            e_t, e_n, e_num = _err(t, wt), _err(nz, wn), _err(t - nz, wt - wn)
            e_true = _err(TO.corrected(t, nz, dev.cutoff_index), TO.corrected(wt, wn, dev.cutoff_index))
            print(f"TFSC_FIGURE masked n={n} per_shell={int(per_shell)} fsc_t={e_t:.3e} fsc_n={e_n:.3e} numerator={e_num:.3e} "
                  f"fsc_true={e_true:.3e} max_fsc_n_past_cutoff={float(np.abs(wn[i:]).max()):.3f}")
            assert e_t <= TOL_FSC_3D and e_n <= TOL_ROUND_TRIP and e_num <= TOL_ROUND_TRIP
        t, nz = dev.masked(mask)
        assert np.array_equal(dev.true_fsc(mask)[:, 1], TO.corrected(t[:, 1], nz[:, 1], dev.cutoff_index))
        # two masks
        mask2 = TO.sphere_mask(n, 0.35 * n, 3.0)
        t, nz = dev.masked(mask, mask2)
        wt, wn = ora.masked(mask, mask2)
        e_t, e_n = _err(t[:, 1], wt[:, 1]), _err(nz[:, 1], wn[:, 1])
        print(f"TFSC_FIGURE two_masks n={n} fsc_t={e_t:.3e} fsc_n={e_n:.3e}")
        assert e_t <= TOL_FSC_3D and e_n <= TOL_ROUND_TRIP


def test_fixture_curves_against_the_reference(golden_dir):
    g = np.load(golden_dir / "g20_true_fsc.npz")
    for k in range(int(g["n_cases"][0])):
        n, _, cutoff, apix, rseed = g[f"c{k}_par"]
        n = int(n)
        a, b = g[f"c{k}_a"].astype(np.float32), g[f"c{k}_b"].astype(np.float32)
        mask = g[f"c{k}_mask"].astype(np.float64)
        np.random.seed(int(rseed))
        with H.TrueFSC(a, b, float(apix), float(cutoff)) as dev:        # the host draws, from the reference's stream
            t, nz = dev.masked(mask)
            true = dev.true_fsc(mask)
            e = {"unmasked": _err(dev.unmasked[:, 1], g[f"c{k}_unmasked"][:, 1]),
                 "rand_unmasked": _err(dev.randomized_unmasked[:, 1], g[f"c{k}_rand_unmasked"][:, 1]),
                 "masked": _err(t[:, 1], g[f"c{k}_masked"][:, 1]), "rand_masked": _err(nz[:, 1], g[f"c{k}_rand_masked"][:, 1]),
                 "true": _err(true[:, 1], g[f"c{k}_true"])}
            pt, pn = dev.masked(mask, per_shell=True)
            e["per_shell_t"], e["per_shell_n"] = _err(pt, g[f"c{k}_per_shell_t"]), _err(pn, g[f"c{k}_per_shell_n"])
            print(f"TFSC_FIGURE fixture n={n} " + " ".join(f"{key}={v:.3e}" for key, v in e.items()))
            assert np.array_equal(true[:, 0], g[f"c{k}_masked"][:, 0])
            for key in ("unmasked", "rand_unmasked", "masked", "per_shell_t"):
                assert e[key] <= TOL_FSC_3D, key
            for key in ("rand_masked", "true", "per_shell_n"):
                assert e[key] <= TOL_ROUND_TRIP, key
        # the function alone, after the same seed, against the reference's own single-precision output
        from scipy.fft import irfftn

        np.random.seed(int(rseed))
        spec = H.randomize_phases_lowpass(a, float(apix), float(cutoff), return_fft=True)
        want = g[f"c{k}_rpl_fft"]
        got = spec if k == 0 else spec[:, :, :: n // 4]
        e_spec = float(np.abs(got - want).max() / np.abs(want).max())
        print(f"TFSC_FIGURE fixture n={n} randomize_phases_lowpass spec_vs_reference_c64={e_spec:.3e}")
        assert spec.dtype == np.complex64 and e_spec <= 2e-6          # two single-precision transforms of one map
        if k == 0:
            np.random.seed(int(rseed))
            vol = H.randomize_phases_lowpass(a, float(apix), float(cutoff))
            ref = g["c0_rpl_map"]
            F32 = want.astype(np.complex64)
            dist = float(np.abs(irfftn(F32) - TO.irfftn(F32)).max() / np.abs(ref).max())
            e_map = float(np.abs(vol - ref).max() / np.abs(ref).max())
            print(f"TFSC_FIGURE fixture n={n} randomize_phases_lowpass map_vs_reference_f32={e_map:.3e} scipy_f32_dist={dist:.3e}")
            assert vol.dtype == np.float32 and vol.shape == ref.shape and e_map <= 9 * dist + 2e-6     # + the spectra's difference


def _blob_pair(n, seed):
    a, b = O.make_map_pair(n, seed, dc="auto")
    g = np.arange(n) - n // 2
    blob = 6.0 * np.exp(-(g[:, None, None] ** 2 + g[None, :, None] ** 2 + g[None, None, :] ** 2) / (2.0 * (n / 6.0) ** 2))
    return (a + blob).astype(np.float32), (b + blob).astype(np.float32)


def _slope_at(curve, threshold=0.143):
    f = curve[:, 1]
    i = int(np.flatnonzero(f < threshold)[0])
    return abs(f[i] - f[i - 1])


def test_true_fsc_end_to_end_against_the_oracle_composition():
    n = 32
    a, b = _blob_pair(n, 4100)
    rng = np.random.RandomState(41)
    u = tuple(rng.uniform(0, 2 * np.pi, size=(n, n, n // 2 + 1)) for _ in range(2))
    cutoff = _cutoff(n)
    user = TO.sphere_mask(n, 0.3 * n, 4.0)
    for name, kw in (("user_mask", dict(mask=user)), ("two_user_masks", dict(mask=[user, TO.sphere_mask(n, 0.35 * n, 3.0)])),
                     ("mask_soft", dict(mask_soft=6.0, one_mask=True)), ("mask_soft_two", dict(mask_soft=5.0))):
        got = T.true_fsc(a, b, APIX, cutoff_res=cutoff, phases=u, **kw)
        want = T.true_fsc(a, b, APIX, cutoff_res=cutoff, phases=u, context=TO.OracleTrueFSC, **kw)
        assert np.array_equal(got["mask1"], want["mask1"]) and np.array_equal(got["mask2"], want["mask2"])     # the host's work: the same
        e = {k: _err(got[k][:, 1], want[k][:, 1]) for k in ("unmasked", "randomized_unmasked", "masked", "randomized_masked", "true")}
        print(f"TFSC_FIGURE end_to_end {name} " + " ".join(f"{k}={v:.3e}" for k, v in e.items()) +
              f" res={got['resolution']} slope={_slope_at(want['true']):.3f}")
        assert e["unmasked"] <= TOL_FSC_3D and e["masked"] <= TOL_FSC_3D and e["randomized_unmasked"] <= TOL_FSC_3D
        assert e["randomized_masked"] <= TOL_ROUND_TRIP
        assert got["mask_soft_px"] == want["mask_soft_px"] and got["cutoff_res"] == cutoff
        for key in ("unmasked", "masked", "true"):
            assert _slope_at(want[key]) >= 0.01
            assert got["resolution"][key] == pytest.approx(want["resolution"][key], rel=1e-4)
    got = T.true_fsc(a, b, APIX, cutoff_res=cutoff, phases=u, one_mask=True, refine_mask=True)
    want = T.true_fsc(a, b, APIX, cutoff_res=cutoff, phases=u, one_mask=True, refine_mask=True, context=TO.OracleTrueFSC)
    print(f"TFSC_FIGURE end_to_end refine width_dev={got['mask_soft_px']:.4f} width_oracle={want['mask_soft_px']:.4f} "
          f"res_dev={got['resolution']['true']:.4f} res_oracle={want['resolution']['true']:.4f}")
    assert 0 < got["mask_soft_px"] < n / 3 and abs(got["mask_soft_px"] - want["mask_soft_px"]) <= 2


def test_device_generator():
    n = 64
    a, b, _ = _inputs(n)
    cutoff = _cutoff(n)
    sel = TO.m_half(n) >= int(np.ceil((n / 4 + 0.5) ** 2))
    mask = TO.sphere_mask(n, 0.3 * n, 4.0)
    runs = []
    for seed in (11, 11, 12):
        with H.TrueFSC(a, b, APIX, cutoff, seed=seed) as dev:
            runs.append(dict(spec=[dev.randomized_map(w, return_fft=True) for w in (0, 1)], maps=[dev.randomized_map(w) for w in (0, 1)],
                             sums=dev.sums.copy(), masked=dev.masked_sums(mask[None]), curve=dev.randomized_unmasked.copy(),
                             index=dev.cutoff_index))
    r0, r1, r2 = runs
    for w in (0, 1):
        assert np.array_equal(r0["spec"][w].view(np.float32), r1["spec"][w].view(np.float32)) and np.array_equal(r0["maps"][w], r1["maps"][w])
        assert not np.array_equal(r0["spec"][w][sel], r2["spec"][w][sel]) and not np.array_equal(r0["maps"][w], r2["maps"][w])
    assert np.array_equal(r0["sums"], r1["sums"]) and np.array_equal(r0["masked"], r1["masked"])
    assert np.array_equal(r0["sums"][0], r2["sums"][0]) and not np.array_equal(r0["sums"][1], r2["sums"][1])
    assert not np.array_equal(r0["masked"][:, 1], r2["masked"][:, 1]) and np.array_equal(r0["masked"][:, 0], r2["masked"][:, 0])
    theta = []
    for w in (0, 1):
        spec, plain = r0["spec"][w], _plain_spectrum(a, b, w)
        assert np.array_equal(spec[~sel].view(np.float32), plain[~sel].view(np.float32))
        amp, amp0 = np.abs(spec.astype(np.complex128)), np.abs(plain.astype(np.complex128))
        e_amp = float((np.abs(amp - amp0)[sel] / amp0[sel].clip(1e-30)).max())
        assert e_amp <= 2.0**-22
        theta.append(np.angle(spec.astype(np.complex128)[sel]))
    N = int(sel.sum())
    assert N >= 10**5
    r_1, r_2 = abs(np.exp(1j * theta[0]).mean()), abs(np.exp(1j * theta[1]).mean())
    r_d = abs(np.exp(1j * (theta[0] - theta[1])).mean())
    r_n = abs(np.exp(1j * (theta[0][1:] - theta[0][:-1])).mean())        # neighbouring counters
    print(f"TFSC_FIGURE generator N={N} resultant map1={r_1:.3e} map2={r_2:.3e} difference={r_d:.3e} neighbours={r_n:.3e} bound={5 / np.sqrt(N):.3e}")
    assert max(r_1, r_2, r_d, r_n) < 5 / np.sqrt(N)
    bins = np.bincount(O.shell_3d_half(n).ravel(), minlength=n // 2 + 1)
    curve, first = r0["curve"], r0["index"] + 2
    worst = float((np.abs(curve[first:, 1]) * np.sqrt(bins[first: len(curve)])).max())
    print(f"TFSC_FIGURE generator randomised_unmasked max |fsc| sqrt(bins) past shell {first - 1} = {worst:.3f} (bound 5)")
    assert worst < 5


def test_batch_equals_single_calls_bit_for_bit():
    n = 40
    a, b, u = _inputs(n)
    masks = np.stack([TO.sphere_mask(n, (0.2 + 0.02 * j) * n, 2.0 + j) for j in range(8)]).astype(np.float32)
    with H.TrueFSC(a, b, APIX, _cutoff(n), phases=u) as dev:
        assert np.array_equal(dev.unmasked, H.calc_fsc(a, b, APIX))                 # the new x pass gives calc_fsc's bits
        for per_shell in (False, True):
            batch = dev.masked_sums(masks, None, per_shell)
            assert batch.shape == (8, 2, n // 2 + 1, 3)
            if not per_shell:
                first_two, curves = batch[:2].copy(), dev.sums.copy()
            assert np.array_equal(batch, np.stack([dev.masked_sums(masks[j: j + 1], None, per_shell)[0] for j in range(8)]))
            assert np.array_equal(batch, dev.masked_sums(masks, None, per_shell))                    # a repeated call
            assert np.array_equal(dev.masked_sums(masks[::-1], None, per_shell), batch[::-1])        # the place in the batch
            assert np.array_equal(dev.masked_sums(masks, masks, per_shell), batch)                    # the same mask given twice
            # the true pair's sums are hh_fsc_3d's of the masked maps
            want = H.fsc.fsc_sums_3d(a * masks[3], b * masks[3], per_shell)
            assert np.array_equal(batch[3, 0], want)
        t, nz = dev.masked_batch(masks)
        assert t.shape == nz.shape == (8, n // 2 + 1, 2)
        for j in (0, 5):
            st, sn = dev.masked(masks[j])
            assert np.array_equal(st, t[j]) and np.array_equal(sn, nz[j])
        pt, pn = dev.masked_batch(masks, per_shell=True)
        assert pt.shape == (8, n // 2 + 1) and np.array_equal(pt[2], dev.masked(masks[2], per_shell=True)[0])
    with H.TrueFSC(a, b, APIX, _cutoff(n), phases=u) as again:                        # a second context: the same bits
        assert np.array_equal(again.masked_sums(masks[:2]), first_two) and np.array_equal(again.sums, curves)


def test_refusals():
    cube = np.ones((16, 16, 16), np.float32)
    with pytest.raises(ValueError, match="even"):
        H.TrueFSC(np.ones((17, 17, 17), np.float32), np.ones((17, 17, 17), np.float32), APIX, 8.0, seed=1)
    big = np.broadcast_to(np.float32(1), (520, 520, 520))
    with pytest.raises(ValueError, match=r"\[8, 512\]"):
        H.TrueFSC(big, big, APIX, 8.0, seed=1)
    nan = cube.copy()
    nan[1, 2, 3] = np.nan
    with pytest.raises(ValueError, match="NaN or infinite"):
        H.TrueFSC(cube, nan, APIX, 8.0, seed=1)
    a, b, _ = _inputs(16, 5)
    with H.TrueFSC(a, b, APIX, 8.0, seed=1) as dev:
        with pytest.raises(ValueError, match="shape"):
            dev.masked(np.ones((16, 16, 12), np.float32))
        with pytest.raises(ValueError, match="shape"):
            dev.masked(cube, np.ones((12, 12, 12), np.float32))
        with pytest.raises(ValueError, match="shape"):
            dev.masked_batch(cube)
        with pytest.raises(ValueError, match="NaN or infinite"):
            dev.masked(nan)
        assert dev.masked(cube)[0].shape == (9, 2)          # and the context still works
    # the library itself, on a machine with a device: the argument check still comes first, a missing device is an error
    import ctypes as C
    from helicon_amd import _lib

    L = _lib.lib()
    f32p = C.POINTER(C.c_float)
    h = C.c_void_p()
    assert L.hh_tfsc_create(C.byref(h), 0, cube.ctypes.data_as(f32p), cube.ctypes.data_as(f32p), 17, 4, None, None, 0) == -1
    assert L.hh_last_error(None).startswith(b"hh_tfsc_create")
    assert L.hh_tfsc_create(C.byref(h), 99, cube.ctypes.data_as(f32p), cube.ctypes.data_as(f32p), 16, 4, None, None, 0) == -2 and not h.value
