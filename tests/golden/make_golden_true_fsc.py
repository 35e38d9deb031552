#!/usr/bin/env python3
"""Generate tests/golden/g20_true_fsc.npz — the phase-randomised true FSC — by importing the REFERENCE itself.

Run in the build container only (the reference never travels to the GPU box):

    MPLBACKEND=Agg PYTHONDONTWRITEBYTECODE=1 PYTHONPATH=<helicon checkout>/src:. python3 tests/golden/make_golden_true_fsc.py

Every array written is an INPUT or an OUTPUT of a reference function; no reference source text is stored:

* ``helicon.lib.filters.randomize_phases_lowpass`` (filters.py:469-520) after ``np.random.seed(seed)``, on the float32 map
  (complex64 / float32 out, both ``return_fft`` values) — and the uniform draws it consumed, regenerated from the same seed;
* the composition of ``helicon.commands.trueFSC.main`` (:113-157, :299-348) on the float64 maps, as ``main`` casts them:
  ``calc_fsc`` of the maps, of the two randomised spectra, of the masked maps and of the masked randomised maps, and
  ``fsc_true``, under a soft spherical mask;
* ``_soft_mask`` (widths 0, 2.5, 9), ``_otsu_threshold_eman``, ``_generate_adaptive_mask`` (Otsu, fraction, value, mass),
  the cutoff rule (:122-135, through the functions it calls) and ``_fit_fsc_curve``.

Cases: 16^3 and 24^3 pairs of tests/fsc_oracle.py's recipe (quantum 1/8, stored as float16, exactly).  To stay below the
sibling fixtures' size the 24^3 case stores the seed and the first 64 draws instead of all draws (NumPy's legacy
``np.random.seed`` stream is frozen, the host test checks the 64), three columns of the randomised spectrum and no soft masks.
"""
import argparse
import os
import sys
from pathlib import Path

import numpy as np
import scipy

import helicon  # the reference
from helicon.commands import trueFSC
from helicon.lib.filters import randomize_phases_lowpass

OUT = Path(__file__).resolve().parent
sys.path.insert(0, str(OUT.parent))
from fsc_oracle import make_map_pair  # noqa: E402
from true_fsc_oracle import sphere_mask  # noqa: E402

CASES = [(16, 200, 4.0, 2.0, 7), (24, 201, 6.0, 2.0, 8)]   # n, map seed, cutoff_res, apix, np.random seed


def cutoff_rule(saxis, fsc):
    """trueFSC.py:126-135 through the reference's own functions."""
    c = trueFSC._find_resolution(saxis, fsc, 0.8)
    if c > 100:
        s_fit, f_fit, _ = trueFSC._fit_fsc_curve(saxis, fsc)
        c = trueFSC._find_resolution(s_fit, f_fit, 0.8)
    if c > 10:
        return round(c)
    if c > 5:
        return round(c * 2) / 2
    return round(c * 4) / 4


def g20():
    from scipy.fft import irfftn

    out = {"versions": np.asarray([np.__version__, scipy.__version__]), "n_cases": np.asarray([len(CASES)])}
    for k, (n, seed, cutoff, apix, rseed) in enumerate(CASES):
        a, b = make_map_pair(n, seed, quantum=0.125)
        out[f"c{k}_a"], out[f"c{k}_b"] = a.astype(np.float16), b.astype(np.float16)
        assert np.array_equal(out[f"c{k}_a"].astype(np.float32), a)
        out[f"c{k}_par"] = np.asarray([n, seed, cutoff, apix, rseed], dtype=np.float64)
        shape = (n, n, n // 2 + 1)
        np.random.seed(rseed)
        u1, u2 = np.random.uniform(0, 2 * np.pi, size=shape), np.random.uniform(0, 2 * np.pi, size=shape)
        if k == 0:
            out[f"c{k}_u1"], out[f"c{k}_u2"] = u1, u2
        else:
            out[f"c{k}_u1_head"], out[f"c{k}_u2_head"] = u1.ravel()[:64], u2.ravel()[:64]
        # the function alone, on the float32 map as a user passes it
        np.random.seed(rseed)
        fft = randomize_phases_lowpass(a, apix, cutoff, return_fft=True)
        assert fft.dtype == np.complex64
        out[f"c{k}_rpl_fft"] = fft if k == 0 else fft[:, :, :: n // 4]       # 24^3: the columns kx = 0, 6, 12 only
        if k == 0:
            np.random.seed(rseed)
            out[f"c{k}_rpl_map"] = randomize_phases_lowpass(a, apix, cutoff)
        # main's composition on float64 maps
        m1, m2 = a.astype(np.float64), b.astype(np.float64)
        np.random.seed(rseed)
        F1r = randomize_phases_lowpass(m1, apix, cutoff, return_fft=True)
        F2r = randomize_phases_lowpass(m2, apix, cutoff, return_fft=True)
        un = helicon.calc_fsc(m1, m2, apix)
        run = helicon.calc_fsc(None, None, apix, F1=F1r, F2=F2r, n=n)
        mask = sphere_mask(n, 0.3 * n, 4.0)
        out[f"c{k}_mask"] = mask.astype(np.float16)          # rounded to float16: stored exactly, at half the size
        mask = out[f"c{k}_mask"].astype(np.float64)
        m1r, m2r = irfftn(F1r, workers=-1), irfftn(F2r, workers=-1)
        t = helicon.calc_fsc(m1 * mask, m2 * mask, apix)
        nz = helicon.calc_fsc(m1r * mask, m2r * mask, apix)
        ci = int(n * apix / cutoff)
        true = np.copy(t[:, 1])
        true[ci + 1:] = (t[ci + 1:, 1] - nz[ci + 1:, 1]) / (1 - nz[ci + 1:, 1])
        true[np.isnan(true)] = 1.0
        out[f"c{k}_unmasked"], out[f"c{k}_rand_unmasked"], out[f"c{k}_masked"], out[f"c{k}_rand_masked"] = un, run, t, nz
        out[f"c{k}_true"] = true
        out[f"c{k}_per_shell_t"] = helicon.calc_fsc_per_shell(m1 * mask, m2 * mask, apix)
        out[f"c{k}_per_shell_n"] = helicon.calc_fsc_per_shell(m1r * mask, m2r * mask, apix)
        out[f"c{k}_cutoff_rule"] = np.asarray(cutoff_rule(un[:, 0], un[:, 1]), dtype=np.float64)
        s_fit, f_fit, r_fit = trueFSC._fit_fsc_curve(t[:, 0], true)
        out[f"c{k}_fit_s"], out[f"c{k}_fit_f"], out[f"c{k}_fit_res"] = s_fit, f_fit, np.asarray(r_fit)
        # masks
        avg = (m1 + m2) / 2
        out[f"c{k}_otsu"] = np.asarray(trueFSC._otsu_threshold_eman(avg))
        modes = [dict(maskFractionThresh=-1, maskThresh=[], maskMass=0), dict(maskFractionThresh=0.3, maskThresh=[], maskMass=0),
                 dict(maskFractionThresh=-1, maskThresh=[0.5, 0.5], maskMass=0), dict(maskFractionThresh=-1, maskThresh=[], maskMass=40.0)]
        for j, mode in enumerate(modes):
            am = trueFSC._generate_adaptive_mask(avg, apix, cutoff, argparse.Namespace(**mode))
            out[f"c{k}_adaptive{j}"] = np.packbits(am.astype(bool))
            if j == 0 and k == 0:
                for w, width in enumerate((0.0, 2.5, 9.0)):
                    out[f"c{k}_soft{w}"] = trueFSC._soft_mask(am, width)
        print("g20 case", n, "cutoff rule", float(out[f"c{k}_cutoff_rule"]), "true", np.round(true, 3))
    out["soft_widths"] = np.asarray([0.0, 2.5, 9.0])
    # the cutoff rule on hand-made curves: each branch of the rounding, and the fitted branch
    s = np.arange(33) / (64 * 1.5)
    curves = [np.clip(1.2 - s / s[k], -0.05, 1.0) for k in (6, 12, 20, 30)] + [np.r_[0.7, np.clip(1.1 - s[1:] / s[14], 0, 1)]]
    out["rule_saxis"], out["rule_curves"] = s, np.asarray(curves)
    out["rule_expected"] = np.asarray([cutoff_rule(s, c) for c in curves], dtype=np.float64)
    np.savez_compressed(OUT / "g20_true_fsc.npz", **out)


if __name__ == "__main__":
    assert "reference" in os.path.abspath(helicon.__file__), helicon.__file__
    g20()
    f = OUT / "g20_true_fsc.npz"
    print(f.name, f.stat().st_size)
