"""The true-FSC context (hh_tfsc_*; helicon_amd/csrc/true_fsc.inc) on every even side 8 ... 72, 126 and 130 against the float64
oracle (tests/true_fsc_sides.py): all four values of n^2 mod 64 at the row edge of the 64-row tile of k_tfsc_xpass, k_tfsc_c2r
and the inverse passes of k_circ_gemm, every ncol = n / 2 + 1 from 5 to 37 and 64 / 66 across the 32-column sub-tile and the
c2r sum's 32-wide slice, both classes of n mod 4.  One context per side, host angles.

Held at every side, with tests/test_gpu_true_fsc.py's bounds unchanged (none measured): the unmasked, randomised-unmasked
and masked curves (half and full spectrum) and the two-mask curves at 3e-7, the randomised-masked curves and fsc_t - fsc_n
at 9e-7, the frequency column bit for bit; the randomised maps against float64 irfftn at 8 x SciPy's float32 distance; the
bins below the cutoff bit for bit and |F'| against |F| at 2^-22; and the STORED SPECTRUM of both maps against float64,
max |spec - F| / max |F| over every bin, at 8 x the distance of SciPy's float32 rfftn from float64 on the same map.
tests/test_true_fsc_sides_host.py shows that each of eleven faults of the pipeline exceeds one of these bounds a thousandfold.

The device generator (seed 0x1234567887654321, sides 10, 14, 30, 66, 130): every substituted bin of both stored spectra lies
within 2^-23 |F| per component of |F| e^{i theta}, theta the host's Philox4x32-10 of the bin's counter (known-answer vectors:
the host file); the oracle given those angles then holds the seeded context to every bound above.

Every test prints its figures (TFSC_FIGURE sides) before it asserts.  Measured on an MI355X, the largest over the 35 sides
(profiles/true_fsc.json, "sides"; DESIGN.md, "True-FSC side census"): 3.3e-8 against the 3e-7 (n = 10), 8.0e-8 against the 9e-7
(two masks, n = 130), 6.0e-8 against 2^-22, the randomised map 7.6e-7 = 3.4 x SciPy's distance (n = 126), the stored spectrum at
most 5.8 x SciPy's distance (n = 126, map 2: 2.038e-7 against 2.827e-7; median 1.6 x), the generator 5.9e-8 against 2^-23.

What the census found: with ONE multiply-add chain over all nx terms in the x pass that spectrum was 3.896e-7, 11.0 x, over the
bound, at the DC bin (which is max |F|: the maps carry an offset); three sequential float32 sums on the host gave the same
3.896e-7.  fc_pair_product now sums each staged slice of 32 on its own and adds the slices; the host chain in that order
(true_fsc_sides.sequential_dc) gives the device's 2.038e-7.  Each side prints the worst bin, SciPy's distance and both host chains
(TFSC_FIGURE sides host_angles_spectrum)."""
import importlib

import numpy as np
import pytest

import true_fsc_oracle as TO
import true_fsc_sides as S
import helicon_amd as H

T = importlib.import_module("helicon_amd.true_fsc")

pytestmark = pytest.mark.gpu


def _plain_spectra(a, b):
    """The device's own half spectra with nothing substituted (m_cut above every bin)."""
    ctx = T._Context(np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32), 2**62, None, None, 0, 0)
    try:
        return [ctx.download(which, want_map=False, want_spec=True)[1] for which in (0, 1)]
    finally:
        ctx.close()


def _report(tag, n, figs, pre=None, notes=None):
    print(f"TFSC_FIGURE sides {tag} n={n} rows_mod_64={n * n % 64} ncol={n // 2 + 1} " + S.figure_line(figs))
    if pre is not None:
        print(f"TFSC_FIGURE sides {tag}_preconditions n={n} " + " ".join(f"{k}={v:.3e}" if isinstance(v, float) else f"{k}={v}" for k, v in pre.items()))
    if notes:
        print(f"TFSC_FIGURE sides {tag}_spectrum n={n} " + " ".join(f"{k}={v:.3e}" if isinstance(v, float) else f"{k}={v}" for k, v in notes.items()))
    zero = [k for k, (v, b) in figs.items() if b == 0 and v != 0]
    print(f"TFSC_FIGURE sides {tag}_exact n={n} failed={','.join(zero) or 'none'}")


@pytest.mark.parametrize("n", S.SIDES)
def test_every_side_against_float64(n):
    a, b, u = S.inputs(n)
    ora = S.oracle(n)
    pre = S.preconditions(ora, n)
    with H.TrueFSC(a, b, S.APIX, S.cutoff(n), phases=u) as dev:
        notes = {}
        figs = S.compare(dev, ora, n, plain=_plain_spectra(a, b), notes=notes)
    _report("host_angles", n, figs, pre, notes)
    assert ora.m_cut == int(np.ceil(S.q_of(n) ** 2)) and pre["same_bins"] and S.preconditions_hold(pre), pre
    assert len(figs) == 28
    assert S.exceeded(figs) == [], {k: figs[k] for k in S.exceeded(figs)}


@pytest.mark.parametrize("n", S.GENERATOR_SIDES)
def test_device_generator_is_philox_of_the_bin(n):
    a, b, _ = S.inputs(n)
    seed = S.GENERATOR_SEED
    theta = S.philox_angles(n, seed)
    ora = S.oracle(n, phases=theta)
    sel = TO.m_half(n) >= ora.m_cut
    plain = _plain_spectra(a, b)
    with H.TrueFSC(a, b, S.APIX, S.cutoff(n), seed=seed) as dev:
        worst = []
        for which in (0, 1):
            e_re, e_im = S.generator_figures(dev.randomized_map(which, return_fft=True), plain[which], theta[which], sel)
            worst += [e_re, e_im]
            print(f"TFSC_FIGURE sides generator n={n} map={which} re={e_re:.3e} im={e_im:.3e} bound={S.TOL_ANGLE:.3e} substituted={int(sel.sum())}")
        figs = S.compare(dev, ora, n, plain=plain)
    _report("seeded", n, figs)
    assert sel.any() and max(worst) <= S.TOL_ANGLE
    assert S.exceeded(figs) == [], {k: figs[k] for k in S.exceeded(figs)}


def test_bit_for_bit_at_a_side_of_4_rows_in_the_last_tile():
    n = 30                                                  # n^2 mod 64 = 4, n mod 4 = 2
    assert n * n % 64 == 4 and n % 4 == 2
    a, b, u = S.inputs(n)
    masks = np.stack([TO.sphere_mask(n, (0.2 + 0.04 * j) * n, 2.0 + j) for j in range(4)]).astype(np.float32)
    with H.TrueFSC(a, b, S.APIX, S.cutoff(n), phases=u) as dev:
        assert np.array_equal(dev.unmasked, H.calc_fsc(a, b, S.APIX))
        first = {}
        for per_shell in (False, True):
            batch = dev.masked_sums(masks, None, per_shell)
            assert batch.shape == (4, 2, n // 2 + 1, 3)
            assert np.array_equal(batch, np.stack([dev.masked_sums(masks[j: j + 1], None, per_shell)[0] for j in range(4)]))
            assert np.array_equal(dev.masked_sums(masks[::-1], None, per_shell), batch[::-1])
            first[per_shell] = batch.copy()
        sums = dev.sums.copy()
        spec = [dev.randomized_map(w, return_fft=True) for w in (0, 1)]
        maps = [dev.randomized_map(w) for w in (0, 1)]
    with H.TrueFSC(a, b, S.APIX, S.cutoff(n), phases=u) as again:
        assert np.array_equal(again.sums, sums)
        for per_shell in (False, True):
            assert np.array_equal(again.masked_sums(masks, None, per_shell), first[per_shell])
        for w in (0, 1):
            assert np.array_equal(again.randomized_map(w, return_fft=True).view(np.float32), spec[w].view(np.float32))
            assert np.array_equal(again.randomized_map(w), maps[w])


def test_sides_outside_the_range_are_refused():
    for n in (6, 514):
        cube = np.broadcast_to(np.float32(1), (n, n, n))
        with pytest.raises(ValueError, match=r"\[8, 512\]"):
            H.TrueFSC(cube, cube, S.APIX, 8.0, seed=1)
        with pytest.raises(ValueError, match=r"\[8, 512\]"):
            H.randomize_phases_lowpass(cube, S.APIX, 8.0, seed=1)
    import ctypes as C
    from helicon_amd import _lib

    L = _lib.lib()
    one = np.ones(8, np.float32).ctypes.data_as(C.POINTER(C.c_float))     # never read: the side is checked first
    for n in (6, 514):
        h = C.c_void_p()
        assert L.hh_tfsc_create(C.byref(h), 0, one, one, n, 4, None, None, 0) == -1 and not h.value
        assert b"[8, 512]" in L.hh_last_error(None)
