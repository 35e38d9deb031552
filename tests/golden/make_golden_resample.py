#!/usr/bin/env python3
"""Generate tests/golden/g23_fft_crop.npz — inputs and outputs of the reference's ``fft_crop`` — by importing the REFERENCE.

Run in the build container only (the reference never travels to the GPU box):

    PYTHONDONTWRITEBYTECODE=1 PYTHONPATH=<helicon checkout>/src python3 tests/golden/make_golden_resample.py

Every array written is an INPUT or an OUTPUT of ``helicon.fft_crop`` (lib/transforms.py:610-660); no reference source text
is stored.  2-D: (24, 20) -> (16, 12), (24, 20) -> (15, 11) (an odd request gives 14 x 10) and (21, 17) -> (10, 8).
3-D: (12, 12, 12) -> (8, 8, 8), where the reference calls ``irfft2`` on the 3-D spectrum: its output is still in Fourier
space along z (and the imaginary part is dropped).  It is stored as it comes; tests/test_fft_resample_host.py pins that it
is NOT ``irfftn``, which is what helicon_amd.fft_crop computes.  The inputs are float32 values stored as float64.
``fft_rescale`` needs finufft, which is not installed: it has no fixture.
"""
import json
import os
import sys
from pathlib import Path

import numpy as np

import helicon  # the reference

OUT = Path(__file__).resolve().parent
CASES = [((24, 20), (16, 12)), ((24, 20), (15, 11)), ((21, 17), (10, 8)), ((12, 12, 12), (8, 8, 8))]


def g23_fft_crop(versions):
    out = {"n_cases": np.asarray([len(CASES)]), "versions": np.asarray(json.dumps(versions))}
    for k, (shape, size) in enumerate(CASES):
        # float32 values held as float64: NumPy 2 would transform a float32 array in single precision
        x = np.random.default_rng(230 + k).standard_normal(shape).astype(np.float32).astype(np.float64)
        got = np.asarray(helicon.fft_crop(x, size))
        out[f"case{k}_in"] = x
        out[f"case{k}_size"] = np.asarray(size)
        out[f"case{k}_out"] = got
        print("g23 case", k, shape, "->", size, got.dtype, got.shape)
    np.savez_compressed(OUT / "g23_fft_crop.npz", **out)


if __name__ == "__main__":
    assert "reference" in os.path.abspath(helicon.__file__), helicon.__file__
    import scipy

    versions = dict(helicon=helicon.__version__, numpy=np.__version__, scipy=scipy.__version__, python=sys.version.split()[0])
    assert versions == json.loads((OUT / "VERSIONS.json").read_text()), versions   # the other fixtures' versions
    g23_fft_crop(versions)
    f = OUT / "g23_fft_crop.npz"
    print(f.name, f.stat().st_size)
