#!/usr/bin/env python3
"""Times of the local resolution map on the device (helicon_amd/local_resolution.py, csrc/local_resolution.inc).

    python tools/local_fsc_bench.py [--out profiles/local_fsc.json] [--sizes 128 256] [--windows 16 24 32] [--steps 4 8]
                                    [--repeats 3] [--accuracy LOG]

Synthetic half maps (tests/local_fsc_cases.make_halves) of SIZE^3; per (size, window, step) and per route that takes the
window — for w <= 24 both routes, timed in the same run — after one warm-up call:

* ``kernel_ms``: device events around the launches of the call (what ``hh_lres_run`` reports), the median of REPEATS calls,
  ``launches`` chunks of at most ``windows_per_launch`` windows, ``kernel_ms_per_launch`` and ``windows_per_s`` from it;
* ``wall_ms``: host clock around ``LocalFSC.run`` (centres up, kernels, results down), the median;
* LDS route only, ``share_of_f32_vector_peak``: the nominal FLOP of the direct DFTs, 40 w^3 (w / 2 + 1) per window pair (x pass
  2 w^2 rows x (w / 2 + 1) outputs x w terms x 2 FMA, y and z pass 2 w (w / 2 + 1) columns x w outputs x w terms x 4 FMA each),
  over ``kernel_ms`` and the MI355X's f32 vector peak: the whole kernel's rate (gather, products and crossing rule included);
* ``numpy_ms_scaled``: the NumPy composition of the yardstick (clip, taper, ``fftn``, ``bincount``, crossing rule) timed on
  a sample of 512 windows in this process and SCALED to the full window count (``numpy_sample_ms`` is what was measured).

With ``--accuracy LOG`` the LFSC_FIGURE lines of a ``pytest tests/test_gpu_local_fsc.py -s`` log give the ``accuracy`` section:
the largest |curve - yardstick| per route, which the tests' bounds are four times.  A run without a GPU fails.
"""
import argparse
import json
import re
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

F32_VECTOR_PEAK = 157.3e12   # MI355X
APIX = 1.5
SAMPLE = 512


def dft_flops(w: int) -> float:
    """Nominal FLOP of the direct DFTs of ONE window pair on the LDS route (module docstring)."""
    return 40.0 * w**3 * (w // 2 + 1)


def parse_accuracy(path):
    worst, upsample = {}, 0.0
    for line in Path(path).read_text().splitlines():
        m = re.search(r"LFSC_FIGURE (.*) route=(\w+) .*curve=([0-9.e+-]+)", line)
        if m:
            label, route, v = m.group(1), m.group(2), float(m.group(3))
            if v > worst.get(route, (0.0, ""))[0]:
                worst[route] = (v, label)
        m = re.search(r"LFSC_FIGURE upsample .* rel=([0-9.e+-]+)", line)
        if m:
            upsample = max(upsample, float(m.group(1)))
    out = {f"max_abs_curve_difference_{r}": dict(value=v, case=label) for r, (v, label) in worst.items()}
    out["max_rel_upsample_difference"] = upsample
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=None)
    ap.add_argument("--sizes", type=int, nargs="*", default=[128, 256])
    ap.add_argument("--windows", type=int, nargs="*", default=[16, 24, 32])
    ap.add_argument("--steps", type=int, nargs="*", default=[4, 8])
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--accuracy", default=None, help="log of `pytest tests/test_gpu_local_fsc.py -s` to take the measured errors from")
    args = ap.parse_args(argv)

    import local_fsc_cases as Y
    from helicon_amd import _lib
    from helicon_amd.local_resolution import LocalFSC, lds_bytes
    import ctypes as C

    result = {"f32_vector_peak_flops": F32_VECTOR_PEAK, "repeats": args.repeats, "numpy_sample_windows": SAMPLE, "cases": []}
    for n in args.sizes:
        h1, h2 = Y.make_halves((n, n, n), 300 + n)
        with LocalFSC(h1, h2) as ctx:
            for w in args.windows:
                for step in args.steps:
                    axes = [Y.window_centres(n, step)] * 3
                    windows = len(axes[0]) ** 3
                    rng = np.random.default_rng(w * 1000 + step)
                    t3 = Y.taper_profile(w).astype(np.float64)
                    t3 = t3[:, None, None] * t3[None, :, None] * t3[None, None, :]
                    t = time.perf_counter()
                    for cz, cy, cx in rng.choice(axes[0], (SAMPLE, 3)):
                        corner = (cz - w // 2, cy - w // 2, cx - w // 2)
                        f = Y.O.ratio(Y.O.sums_3d(Y.clip(h1, corner, w) * t3, Y.clip(h2, corner, w) * t3, True))
                        Y.resolution_from_curve(f, w, APIX, 0.5)
                    sample_ms = (time.perf_counter() - t) * 1e3
                    case = dict(case=f"{n}^3 w={w} step={step}", n=n, window=w, step=step, windows=windows, numpy_sample_ms=sample_ms,
                                numpy_ms_scaled=sample_ms * windows / SAMPLE, numpy_is_scaled_from_sample=True, routes={})
                    grids = {}
                    for route in (("lds", "passes") if w <= 24 else ("passes",)):
                        per = C.c_int64(0)
                        _lib.check(_lib.lib().hh_lres_plan(w, {"lds": 1, "passes": 2}[route], 0, 0, None, None, C.byref(per)), None)
                        ctx.run(APIX, w, step, route=route)   # warm-up: code objects, first allocations
                        walls, kernels = [], []
                        for _ in range(args.repeats):
                            t = time.perf_counter()
                            r = ctx.run(APIX, w, step, route=route)
                            walls.append((time.perf_counter() - t) * 1e3)
                            kernels.append(r.kernel_ms)
                        grids[route] = r.resolution
                        kern, launches = float(np.median(kernels)), -(-windows // int(per.value))
                        rec = dict(kernel_ms=kern, wall_ms=float(np.median(walls)), windows_per_launch=int(per.value), launches=launches,
                                   kernel_ms_per_launch=kern / launches, windows_per_s=windows / (kern * 1e-3))
                        if route == "lds":
                            rec.update(lds_bytes=lds_bytes(w), dft_gflop=dft_flops(w) * windows / 1e9,
                                       share_of_f32_vector_peak=dft_flops(w) * windows / (kern * 1e-3) / F32_VECTOR_PEAK)
                        case["routes"][route] = rec
                    if len(grids) == 2:
                        case["max_rel_resolution_difference_between_routes"] = float(np.abs(grids["lds"] / grids["passes"] - 1).max())
                        case["lds_over_passes_kernel_time"] = case["routes"]["lds"]["kernel_ms"] / case["routes"]["passes"]["kernel_ms"]
                    best = min(case["routes"], key=lambda k: case["routes"][k]["kernel_ms"])
                    case["speedup_over_numpy_scaled"] = case["numpy_ms_scaled"] / case["routes"][best]["wall_ms"]
                    result["cases"].append(case)
                    print(json.dumps(case), flush=True)
    if args.accuracy:
        result["accuracy"] = parse_accuracy(args.accuracy)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(result, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
