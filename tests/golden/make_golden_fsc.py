#!/usr/bin/env python3
"""Generate tests/golden/g19_fsc.npz — Fourier shell / ring correlation — by importing the REFERENCE itself.

Run in the build container only (the reference never travels to the GPU box):

    MPLBACKEND=Agg PYTHONDONTWRITEBYTECODE=1 PYTHONPATH=<helicon checkout>/src:. python3 tests/golden/make_golden_fsc.py

Every array written is an INPUT or an OUTPUT of a reference function; no reference source text is stored:

* ``helicon.calc_fsc`` and ``helicon.calc_fsc_per_shell`` (lib/analysis.py:116-290) on cubes 24^3 and 33^3 at apix 2.0 and
  0.4 (the second cuts rows: the reference compares 1/Angstrom with cycles per pixel);
* ``helicon.calc_frc_2d`` and ``helicon.frc_score`` with and without the fit (analysis.py:293-484) on 64 x 64, 48 x 96,
  45 x 63 images;
* ``_find_resolution`` of ``helicon.commands.trueFSC`` (:427-462) on the curves above and on hand-made ones.

The inputs follow tests/fsc_oracle.py's recipe (smooth signal + unit white noise, rounded to multiples of 1/8 and to float16:
stored exactly, and few enough distinct values for the file to stay below the other fixtures' size; the reference ran on
their float32 values).
"""
import os
import sys
from pathlib import Path

import numpy as np

import helicon  # the reference
from helicon.commands import trueFSC

OUT = Path(__file__).resolve().parent
sys.path.insert(0, str(OUT.parent))
from fsc_oracle import make_map_pair  # noqa: E402


def g19_fsc():
    out = {}
    cubes = [(24, 190), (33, 191)]
    apixes = [2.0, 0.4]
    for k, (n, seed) in enumerate(cubes):
        a, b = make_map_pair(n, seed, quantum=0.125)
        out[f"cube{k}_a"], out[f"cube{k}_b"] = a.astype(np.float16), b.astype(np.float16)
        assert np.array_equal(out[f"cube{k}_a"].astype(np.float32), a)
        for j, apix in enumerate(apixes):
            rows = helicon.calc_fsc(a, b, apix)
            out[f"cube{k}_{j}_fsc"] = rows
            out[f"cube{k}_{j}_per_shell"] = helicon.calc_fsc_per_shell(a, b, apix)
            for t, thr in enumerate((0.143, 0.5)):
                out[f"cube{k}_{j}_res{t}"] = np.asarray(trueFSC._find_resolution(rows[:, 0], rows[:, 1], thr))
            print("g19 cube", n, apix, rows.shape)
    out["cube_apix"] = np.asarray(apixes)
    out["n_cubes"] = np.asarray([len(cubes)])
    images = [((64, 64), 192), ((48, 96), 193), ((45, 63), 194)]
    for k, (shape, seed) in enumerate(images):
        a, b = make_map_pair(0, seed, shape=shape, quantum=0.125)
        out[f"img{k}_a"], out[f"img{k}_b"] = a.astype(np.float16), b.astype(np.float16)
        saxis, fsc = helicon.calc_frc_2d(a, b, 2.0)
        out[f"img{k}_saxis"], out[f"img{k}_frc"] = saxis, fsc
        out[f"img{k}_score"] = np.asarray(helicon.frc_score(a, b, 2.0))
        out[f"img{k}_score_fit"] = np.asarray(helicon.frc_score(a, b, 2.0, use_fit=True))
        print("g19 image", shape, float(out[f"img{k}_score"]), float(out[f"img{k}_score_fit"]))
    out["img_apix"] = np.asarray([2.0])
    out["n_images"] = np.asarray([len(images)])
    # _find_resolution on hand-made curves: crossing, never crossing, the first shell below, a flat segment, a rising start
    s = np.arange(6) / 48.0
    curves = [np.array([1.0, 0.9, 0.6, 0.3, 0.1, 0.0]), np.array([1.0, 0.9, 0.8, 0.7, 0.6, 0.55]),
              np.array([0.1, 0.9, 0.6, 0.3, 0.1, 0.0]), np.array([1.0, 0.1, 0.1, 0.1, 0.1, 0.1]),
              np.array([1.0, 1.0, 0.4, 0.4, 0.05, 0.05])]
    out["res_saxis"] = s
    out["res_curves"] = np.asarray(curves)
    out["res_thresholds"] = np.asarray([0.143, 0.5])
    out["res_expected"] = np.asarray([[trueFSC._find_resolution(s, c, t) for t in (0.143, 0.5)] for c in curves])
    out["res_shifted_expected"] = np.asarray([[trueFSC._find_resolution(s + 0.01, c, t) for t in (0.143, 0.5)] for c in curves])
    np.savez_compressed(OUT / "g19_fsc.npz", **out)


if __name__ == "__main__":
    assert "reference" in os.path.abspath(helicon.__file__), helicon.__file__
    g19_fsc()
    f = OUT / "g19_fsc.npz"
    print(f.name, f.stat().st_size)
