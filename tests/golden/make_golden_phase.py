#!/usr/bin/env python3
"""Generate tests/golden/g21_phase_difference.npz — compute_phase_difference_across_meridian — by importing the REFERENCE.

Run in the build container only (the reference never travels to the GPU box):

    MPLBACKEND=Agg PYTHONDONTWRITEBYTECODE=1 PYTHONPATH=<helicon checkout>/src:. python3 tests/golden/make_golden_phase.py

Every array written is an INPUT or an OUTPUT of ``helicon.lib.transforms.compute_phase_difference_across_meridian``
(transforms.py:823-842); no reference source text is stored.  Inputs: seeded uniform phases in (-pi, pi] — a 2-D array with
an even last axis, one with an odd last axis and one 3-D array (float64), and the even one again as float32.
"""
from pathlib import Path

import numpy as np

from helicon.lib.transforms import compute_phase_difference_across_meridian  # the reference

OUT = Path(__file__).resolve().parent
SHAPES = [(12, 16), (9, 15), (3, 6, 10)]


def main():
    rng = np.random.default_rng(21)
    out = {"versions": np.asarray([np.__version__]), "n_cases": np.asarray([len(SHAPES) + 1])}
    cases = [rng.uniform(-np.pi, np.pi, s) for s in SHAPES]
    cases.append(cases[0].astype(np.float32))
    for k, phase in enumerate(cases):
        out[f"phase_{k}"] = phase
        out[f"diff_{k}"] = compute_phase_difference_across_meridian(phase.copy())
    np.savez_compressed(OUT / "g21_phase_difference.npz", **out)
    print({k: (v.shape, str(v.dtype)) for k, v in out.items()})


if __name__ == "__main__":
    main()
