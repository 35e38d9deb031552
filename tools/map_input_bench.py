#!/usr/bin/env python3
"""Timing of the 3-D map input at a size users load: a 384^3 map at 1 Angstrom resampled to 5 Angstrom.

    python tools/map_input_bench.py [n]                  # device: low_high_pass_filter_3d and symmetrize_transform_map
    python tools/map_input_bench.py [n] --calls 3        # the same calls only (run it under rocprofv3 --kernel-trace --stats)
    python tools/map_input_bench.py [n] --stats FILE     # share of the f32 matrix peak from that run's kernel_stats.csv
    python tools/map_input_bench.py [n] --cpu            # the reference's filter (NumPy fftn / ifftn) on the host

The device calls are timed on the host around each synchronous call (median of 3 after a warm-up), so they include the
host <-> device copies of the map; the kernels alone are in the rocprofv3 statistics.  Prints one JSON line."""
import csv
import json
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

F32_MATRIX_PEAK = 157.3e12   # MI355X, f32 in / f32 accumulate MFMA (spec; 155 TF measured)
APIX, NEW_APIX, TWIST, RISE = 1.0, 5.0, 1.2, 4.75   # an amyloid-like pitch: a 140-voxel output length


def blob(n, seed=0):
    rng = np.random.default_rng(seed)
    v = rng.random((n, n, n), dtype=np.float32)
    v[: n // 8] = 0
    v[-n // 8:] = 0
    return v


def filter_flops(shape, terms=1):
    """Multiply-adds x 2 of the circulant products of one call: an even side costs one real product per plane, an odd
    side two (real input) or two K = 2n products (complex input); the last pass computes the real plane only."""
    total = int(np.prod(shape))
    flops, cplx = 0, False
    for ax, n in enumerate(shape):
        last, odd = ax == 2, n % 2 == 1
        if not odd:
            products = (2 if cplx and not last else 1) * n
        elif not cplx:
            products = (1 if last else 2) * n
        else:
            products = (1 if last else 2) * 2 * n
        flops += 2 * products * total
        cplx = (cplx or odd) and not last
    return terms * flops


def main(argv):
    n = int(argv[0]) if argv and argv[0].isdigit() else 384
    shape = (n, n, n)
    frac = APIX / NEW_APIX
    width = int(n * APIX / NEW_APIX) // 4 * 4
    new_size = (int(round(0.5 * 360 * RISE / TWIST / NEW_APIX)) // 4 * 4, width, width)
    out = dict(shape=list(shape), apix=APIX, new_apix=NEW_APIX, low_pass_fraction=frac, new_size=list(new_size),
               filter_gflop=filter_flops(shape) / 1e9)
    if "--cpu" in argv:
        from tests.test_gpu_map_input import np_filter_3d   # the reference's filter, restated in NumPy

        vol = blob(n)
        t0 = time.perf_counter()
        np_filter_3d(vol, frac)
        out["cpu_filter_s"] = time.perf_counter() - t0
        print(json.dumps(out))
        return
    if "--stats" in argv:
        path = argv[argv.index("--stats") + 1]
        calls = int(argv[argv.index("--calls") + 1]) if "--calls" in argv else 3
        with open(path) as f:
            rows = list(csv.DictReader(f))
        name = lambda r: r["Name"].removeprefix("void ").replace("(anonymous namespace)::", "").split("(")[0]  # noqa: E731
        by = {name(r): float(r["TotalDurationNs"]) for r in rows}
        gemm_ns = sum(v for k, v in by.items() if "k_circ_gemm" in k) / calls
        out["kernels_ms_per_call"] = {k: v / calls / 1e6 for k, v in sorted(by.items(), key=lambda kv: -kv[1])}
        out["filter_gemm_ms"] = gemm_ns / 1e6
        out["filter_tflops"] = filter_flops(shape) / (gemm_ns * 1e-9) / 1e12
        out["filter_share_of_f32_matrix_peak"] = filter_flops(shape) / (gemm_ns * 1e-9) / F32_MATRIX_PEAK
        print(json.dumps(out))
        return
    import helicon_amd as H

    vol = blob(n)
    if "--calls" in argv:   # the profiled run: filter and symmetrisation, nothing else
        for _ in range(int(argv[argv.index("--calls") + 1])):
            H.symmetrize_transform_map(vol, APIX, TWIST, RISE, 1, 1.0, new_size, NEW_APIX)
        print(json.dumps(out))
        return

    def timed(fn, reps=3):
        fn()   # warm-up
        ms = []
        for _ in range(reps):
            t0 = time.perf_counter()
            fn()   # synchronous: returns when the result is on the host
            ms.append(1e3 * (time.perf_counter() - t0))
        return float(np.median(ms))

    out["filter_ms"] = timed(lambda: H.low_high_pass_filter_3d(vol, frac))
    out["filter_tflops_incl_copies"] = filter_flops(shape) / (out["filter_ms"] * 1e-3) / 1e12
    out["symmetrize_transform_map_ms"] = timed(lambda: H.symmetrize_transform_map(vol, APIX, TWIST, RISE, 1, 1.0, new_size, NEW_APIX))
    out["symmetrize_transform_map_tilted_ms"] = timed(
        lambda: H.symmetrize_transform_map(vol, APIX, TWIST, RISE, 1, 1.0, new_size, NEW_APIX, 15.0, 5.0))
    print(json.dumps(out))


if __name__ == "__main__":
    main(sys.argv[1:])
