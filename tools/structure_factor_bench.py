#!/usr/bin/env python3
"""Times of the structure-factor profile and match on the device (helicon_amd/structure_factor.py, csrc/structure_factor.inc).

    python tools/structure_factor_bench.py [--out profiles/structure_factor.json] [--repeats 5] [--accuracy LOG]

Per case (128^3, 256^3, a helical box of 96 x 96 x 384, and 16 x 128^3 on one matcher; a smooth signal plus white noise), after
a warm-up of every call that is timed; medians of REPEATS:

* ``profile``: ``StructureFactorMatcher.profile(maps)`` on the resident context: wall (host clock; upload and download
  included) and ``kernel_ms`` from device events (prologue, forward passes, fused sums);
* ``match`` and ``match_masked``: ``.match(maps)`` and ``.match(maps, mask, thresh)``: wall and the device-event times of
  the four phases (profile, the second transform of the raw data, the scaling sweep, the inverse passes), with the share of
  the scaling in the device time;
* ``one_shot``: ``match_structural_factors`` of one map (two contexts made and dropped): wall;
* ``numpy``: the NumPy composition of the reference's lines for one map (tests/structure_factor_oracle.py: ``fftn``,
  ``searchsorted``, ``bincount``, ``interp1d``, ``ifftn`` in float64) in the same run: wall, one run;
* ``fsc_pair_kernel_ms``: ``hh_fsc_3d``'s device time for ONE PAIR of the same cube, beside the profile's, for orientation:
  it transforms two maps (cubes only);
* ``accuracy_here``: per-bin sums relative to the bin's own sum and matched maps relative to max|want|, against the float64
  restatement, on the case's first map.

With ``--accuracy LOG`` the SF_FIGURE lines of a ``pytest tests/test_gpu_structure_factor.py -s`` log are parsed into the
``accuracy`` section: the maxima the tests' bounds were taken from.  A run without a GPU fails: there is nothing to time.
"""
import argparse
import json
import re
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import structure_factor_oracle as O  # noqa: E402
from helicon_amd import fsc as F  # noqa: E402
from helicon_amd import structure_factor as S  # noqa: E402

CASES = [("128^3", (128, 128, 128), 1), ("256^3", (256, 256, 256), 1), ("96x96x384", (96, 96, 384), 1), ("16 x 128^3", (128, 128, 128), 16)]
APIX, APIX_TARGET = 1.2, 1.0


def median_ms(fn, repeats):
    out = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(out))


def run_case(name, shape, batch, repeats):
    data, target, mask = O.make_inputs(shape, 11, noise=4.0)   # the floor of these large boxes: every bin above 1e-4 of the strongest
    maps = data if batch == 1 else np.stack([np.roll(data, j, axis=0) for j in range(batch)])
    t0 = time.perf_counter()
    tbins, tsf = O.calculate_structural_factor(target, APIX_TARGET)
    want = O.set_structural_factors(data, APIX, tbins, tsf)
    numpy_ms = (time.perf_counter() - t0) * 1e3
    want_sf = O.calculate_structural_factor(data, APIX)[1]
    row = {"shape": list(shape), "batch": batch, "nbins": int(len(want_sf)), "numpy": {"wall_ms": numpy_ms}}
    with S.StructureFactorMatcher(shape, APIX, tbins, tsf) as m:
        sf = m.profile(maps)
        out = m.match(maps)
        m.match(maps, mask=mask, thresh=O.THRESH)
        first_sf, first_out = (sf, out) if batch == 1 else (sf[0], out[0])
        row["accuracy_here"] = {"sf_rel": float(np.abs(first_sf / want_sf - 1).max()),
                                "match_rel": float(np.abs(first_out - want).max() / np.abs(want).max()),
                                "floor": O.floor_ratio(shape, APIX, want_sf)}
        kernel = []

        def profile():
            m.profile(maps)
            kernel.append(m.kernel_ms()["profile"])

        row["profile"] = {"wall_ms": median_ms(profile, repeats), "kernel_ms": float(np.median(kernel))}
        for key, kw in (("match", {}), ("match_masked", dict(mask=mask, thresh=O.THRESH))):
            phases = []

            def match():
                m.match(maps, **kw)
                phases.append(m.kernel_ms())

            wall = median_ms(match, repeats)
            ms = {k: float(np.median([p[k] for p in phases])) for k in phases[0]}
            total = sum(ms.values())
            row[key] = {"wall_ms": wall, "kernel_ms": ms, "kernel_total_ms": total, "scaling_share": ms["scaling"] / total}
    if batch == 1:
        row["one_shot"] = {"wall_ms": median_ms(lambda: S.match_structural_factors(data, APIX, target, APIX_TARGET), repeats)}
    if len(set(shape)) == 1 and batch == 1:
        F.fsc_sums_3d(data, target)
        row["fsc_pair_kernel_ms"] = float(np.median([F.fsc_sums_3d(data, target, return_kernel_ms=True)[1] for _ in range(repeats)]))
    print(name, json.dumps(row), flush=True)
    return row


def parse_accuracy(log):
    figures = {"impulse_max_dev": 0.0, "sf_rel": 0.0, "match_rel": 0.0, "spike_sf_rel": 0.0, "spike_match_rel": 0.0, "lines": 0}
    for line in Path(log).read_text().splitlines():
        if "SF_FIGURE" not in line:
            continue
        figures["lines"] += 1
        val = lambda key: [float(v) for v in re.findall(rf"{key}=(\d\.\d+e[-+]\d+)", line)]   # noqa: E731
        if "SF_FIGURE impulse" in line:
            figures["impulse_max_dev"] = max([figures["impulse_max_dev"]] + [float(v) for v in re.findall(r"count\|=(\S+)", line)])
        elif "SF_FIGURE spike" in line:
            figures["spike_sf_rel"] = max([figures["spike_sf_rel"]] + val("sf"))
            figures["spike_match_rel"] = max([figures["spike_match_rel"]] + val("match"))
        elif "SF_FIGURE fixture" in line:   # sf, its restatement, match, its restatement, set
            v = [float(x) for x in re.findall(r"(\d\.\d+e[-+]\d+)", line)]
            figures["sf_rel"] = max([figures["sf_rel"]] + v[:2])
            figures["match_rel"] = max([figures["match_rel"]] + v[2:])
        else:
            figures["sf_rel"] = max([figures["sf_rel"]] + val("sf"))
            figures["match_rel"] = max([figures["match_rel"]] + val("match") + val("set"))
    return figures


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=str(ROOT / "profiles" / "structure_factor.json"))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--accuracy", default=None, help="log of pytest tests/test_gpu_structure_factor.py -s")
    ap.add_argument("--cases", nargs="*", default=None, help="names of the cases to run (default: all)")
    args = ap.parse_args(argv)
    result = {"tool": "tools/structure_factor_bench.py", "apix": APIX, "apix_target": APIX_TARGET, "repeats": args.repeats, "cases": {}}
    for name, shape, batch in CASES:
        if args.cases is None or name in args.cases:
            result["cases"][name] = run_case(name, shape, batch, args.repeats)
    if args.accuracy:
        result["accuracy"] = parse_accuracy(args.accuracy)
        result["accuracy"]["bounds"] = {"TOL_SF": 2e-6, "TOL_MATCH": 2e-6, "TOL_SF_SPIKE": 3e-6, "TOL_MATCH_SPIKE": 4e-6,
                                        "rule": "measurement x 4, rounded up to one significant digit; matched maps never above 4e-6"}
    Path(args.out).write_text(json.dumps(result, indent=1) + "\n")
    print("wrote", args.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
