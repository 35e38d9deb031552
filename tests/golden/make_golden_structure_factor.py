#!/usr/bin/env python3
"""Generate tests/golden/g24_structure_factor.npz — structure factors — by importing the REFERENCE itself.

Run in the build container only (the reference never travels to the GPU box):

    MPLBACKEND=Agg PYTHONDONTWRITEBYTECODE=1 PYTHONPATH=<helicon checkout>/src:. python3 tests/golden/make_golden_structure_factor.py

Every array written is an INPUT or an OUTPUT of a reference function; no reference source text is stored:

* ``helicon.calculate_structural_factor`` (lib/filters.py:22-95), ``helicon.set_structural_factors`` (:98-166) and
  ``helicon.match_structural_factors`` (:169-208) on the shapes and voxel sizes of
  tests/structure_factor_oracle.py's FIXTURE_CASES (cubes that tie with the last bin edge at, below and above it, unequal
  and odd boxes, two images), each plain, with a mask, with ``thresh`` and with both (with a mask the reference scales the
  RAW spectrum), the target at another voxel size.

The inputs follow tests/structure_factor_oracle.py's recipe and are stored as float16 (exactly); the reference ran on their
float64 values, so that its transforms are float64 (NumPy's transform of float32 input is float32).
"""
import os
import sys
from pathlib import Path

import numpy as np
import scipy

import helicon  # the reference

OUT = Path(__file__).resolve().parent
sys.path.insert(0, str(OUT.parent))
import structure_factor_oracle as O  # noqa: E402


def g24_structure_factor():
    out = {"versions": np.asarray([f"numpy {np.__version__}", f"scipy {scipy.__version__}", f"python {sys.version.split()[0]}"])}
    out["shapes"] = np.asarray([list(s) + [0] * (3 - len(s)) for s, _ in O.FIXTURE_CASES])
    out["apix"] = np.asarray([a for _, a in O.FIXTURE_CASES])
    out["apix_target_factor"] = np.asarray([O.TARGET_APIX_FACTOR])
    out["thresh"] = np.asarray([O.THRESH, O.THRESH_TARGET])
    for k, (shape, apix) in enumerate(O.FIXTURE_CASES):
        data, target, mask = O.make_inputs(shape, 240 + k)
        for name, a in (("data", data), ("target", target), ("mask", mask)):
            out[f"c{k}_{name}"] = a.astype(np.float16)
            assert np.array_equal(out[f"c{k}_{name}"].astype(np.float32), a)
        d64, t64, m64 = data.astype(np.float64), target.astype(np.float64), mask.astype(np.float64)
        apix_t = apix * O.TARGET_APIX_FACTOR
        for variant in O.VARIANTS:
            thresh, thresh_t, m = O.variant_args(variant, m64)
            key = O.case_key(k, variant)
            qbins, sf = helicon.calculate_structural_factor(d64, apix, thresh=thresh, mask=m)
            tbins, tsf = helicon.calculate_structural_factor(t64, apix_t, thresh=thresh_t, mask=m)
            out[f"{key}_qbins"], out[f"{key}_sf"] = qbins, sf
            out[f"{key}_tbins"], out[f"{key}_tsf"] = tbins, tsf
            out[f"{key}_match"] = helicon.match_structural_factors(d64, apix, t64, apix_t, thresh=thresh, thresh_target=thresh_t, mask=m)
            # (match is set on the target's profile: one array serves both, and the file stays within the size limit)
            assert np.array_equal(out[f"{key}_match"], helicon.set_structural_factors(d64, apix, tbins, tsf, thresh=thresh, mask=m))
        print("g24", shape, apix, len(qbins))
    np.savez_compressed(OUT / "g24_structure_factor.npz", **out)


if __name__ == "__main__":
    assert "reference" in os.path.abspath(helicon.__file__), helicon.__file__
    g24_structure_factor()
    f = OUT / "g24_structure_factor.npz"
    print(f.name, f.stat().st_size)
