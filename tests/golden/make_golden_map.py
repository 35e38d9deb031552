#!/usr/bin/env python3
"""Generate tests/golden/g17_map_input.npz — the app's 3-D map input — by importing the REFERENCE itself.

Run in the build container only (the reference never travels to the GPU box), with a fresh cache directory so that the
reference's cached ``symmetrize_transform_map`` really runs:

    HELION_CACHE_DIR=$(mktemp -d) PYTHONDONTWRITEBYTECODE=1 \\
        PYTHONPATH=<helicon checkout>/src python3 tests/golden/make_golden_map.py

Every array written is an INPUT or an OUTPUT of a reference function; no reference source text is stored:

* the 3-D branch of ``helicon.low_high_pass_filter`` (lib/filters.py:349-372) on even, odd and mixed shapes;
* ``symmetrize_transform_map`` (webApps/denovo3D/utils.py:346-383) with new_apix above and at apix, with axial rotation
  and tilt;
* ``generate_xyz_projections`` (utils.py:336-345), plain and amyloid (including a slab wider than the map).

The input maps are stored as float16 (the reference ran on their exact float32 values) to keep the file small.
"""
import json
import os
import sys
from pathlib import Path

import numpy as np

import helicon  # the reference
from helicon.webApps.denovo3D import utils

OUT = Path(__file__).resolve().parent


def _blob_map(shape, seed):
    """Smooth positive map (a dozen Gaussian blobs), rounded to float16 so it can be stored exactly in half the bytes."""
    rng = np.random.default_rng(seed)
    nz, ny, nx = shape
    Z, Y, X = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    vol = np.zeros(shape)
    for _ in range(12):
        cz, cy, cx = rng.uniform(0.2, 0.8, 3) * np.asarray(shape)
        vol += rng.uniform(0.5, 1.5) * np.exp(-((Z - cz) ** 2 + (Y - cy) ** 2 + (X - cx) ** 2) / rng.uniform(3, 9))
    return vol.astype(np.float16)


def g17_map_input():
    out = {}
    # low_high_pass_filter, 3-D branch: (shape, [(low, high), ...])
    fractions = [(0.3, 0.0), (0.0, 0.2), (0.5, 0.1)]
    filter_shapes = [(12, 12, 12), (11, 9, 13), (12, 11, 10)]
    for k, shape in enumerate(filter_shapes):
        vol = _blob_map(shape, 170 + k)
        out[f"filter{k}_in"] = vol
        for j, (lp, hp) in enumerate(fractions):
            got = helicon.low_high_pass_filter(vol.astype(np.float32), low_pass_fraction=lp, high_pass_fraction=hp)
            assert got.dtype == np.float32, got.dtype
            out[f"filter{k}_{j}_out"] = got
    out["filter_fractions"] = np.asarray(fractions, dtype=np.float64)
    out["n_filter"] = np.asarray([len(filter_shapes)])
    # symmetrize_transform_map: (map, apix, twist, rise, csym, fraction, new_size, new_apix, axial_rotation, tilt)
    maps = [_blob_map((32, 28, 28), 180), _blob_map((25, 23, 21), 181)]
    for m, vol in enumerate(maps):
        out[f"map{m}"] = vol
    sym_cases = [
        (0, 1.0, 30.0, 4.75, 1, 1.0, (24, 16, 16), 2.0, 0.0, 0.0),     # new_apix > apix: the filter runs (even sides)
        (0, 1.0, -41.5, 6.5, 2, 1.0, (20, 20, 20), 1.0, 20.0, 5.0),    # new_apix == apix: no filter; rotation and tilt
        (1, 1.2, 12.0, 4.75, 3, 1.0, (15, 13, 13), 1.6, 15.0, -3.0),   # odd sides, the filter, rotation and tilt
    ]
    for k, (m, apix, tw, rs, cs, fr, ns, na, rot, tilt) in enumerate(sym_cases):
        got = utils.symmetrize_transform_map(maps[m].astype(np.float32), apix, tw, rs, cs, fr, ns, na, rot, tilt)
        out[f"sym{k}_args"] = np.asarray([m, apix, tw, rs, cs, fr, *ns, na, rot, tilt], dtype=np.float64)
        out[f"sym{k}_out"] = np.asarray(got)
        print("g17 sym", k, np.asarray(got).dtype, np.asarray(got).shape)
    out["n_sym"] = np.asarray([len(sym_cases)])
    # generate_xyz_projections: (map, is_amyloid, apix)
    proj_cases = [(0, False, None), (0, True, 1.0), (1, True, 0.15)]   # the last slab (32 slices) is wider than the map (25)
    for k, (m, amy, apix) in enumerate(proj_cases):
        got = utils.generate_xyz_projections(maps[m].astype(np.float32), is_amyloid=amy, apix=apix)
        out[f"proj{k}_args"] = np.asarray([m, float(amy), -1.0 if apix is None else apix], dtype=np.float64)
        for a, p in enumerate(got):
            out[f"proj{k}_{a}"] = np.asarray(p)
    out["n_proj"] = np.asarray([len(proj_cases)])
    np.savez_compressed(OUT / "g17_map_input.npz", **out)


if __name__ == "__main__":
    assert "reference" in os.path.abspath(helicon.__file__), helicon.__file__
    g17_map_input()
    import scipy

    versions = dict(helicon=helicon.__version__, numpy=np.__version__, scipy=scipy.__version__, python=sys.version.split()[0])
    assert versions == json.loads((OUT / "VERSIONS.json").read_text()), versions   # the other fixtures' versions
    f = OUT / "g17_map_input.npz"
    print(f.name, f.stat().st_size)
