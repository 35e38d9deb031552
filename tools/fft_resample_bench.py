#!/usr/bin/env python3
"""Timing of the Fourier resampling of a map at sizes users load: 256^3 -> 128^3, 384^3 -> 192^3 and 128^3 -> 256^3.

    python tools/fft_resample_bench.py [--out profiles/fft_resample.json] [--reps 3] [--only 256:128]

For every workload and epilogue (abs, real): the wall time of ``fft_resample`` on the host around the synchronous call
(median of --reps after a warm-up; it includes building the operators and the host <-> device copies of the map), the
device-event time of the three passes alone, the products' share of the f32 matrix peak, and the largest difference from
the NumPy composition, which is timed in the same run.  On even sides that composition is fftn, a gather of the
spectrum at the new frequencies (the periodic copy beyond the input's Nyquist frequency when up-sampling) and ifftn:
what proc3d's ``ifftn(fft_rescale(...))`` evaluates.  ``copies_dominate`` records whether the wall time outside the
kernels exceeds the kernels'.  Prints one JSON line."""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

F32_MATRIX_PEAK = 157.3e12   # MI355X, f32 in / f32 accumulate MFMA (spec; 155 TF measured)
WORKLOADS = [(256, 128), (384, 192), (128, 256)]


def blob(n, seed=0):
    rng = np.random.default_rng(seed)
    v = rng.random((n, n, n), dtype=np.float32) - 0.3
    v[: n // 8] = 0
    v[-n // 8:] = 0
    return v


def numpy_resample(x, size, kind):
    """proc3d's composition on even sides, in NumPy at x's precision."""
    spec = np.fft.fftn(x)
    idx = [np.rint(np.fft.fftfreq(on) * on).astype(np.int64) % n for n, on in zip(x.shape, size)]
    inv = np.fft.ifftn(spec[np.ix_(*idx)])
    out = np.abs(inv) if kind == "abs" else inv.real
    return out * (np.prod(size) / np.prod(x.shape))


def product_flops(shape, size, kind):
    """Multiply-adds x 2 of the three passes: two real products on the real input, four on a complex one, half of them
    in the last pass under ``real``."""
    cur, flops, cx = list(shape), 0, False
    for ax in range(3):
        products = (4 if cx else 2) // (2 if ax == 2 and kind == "real" else 1)
        p = cur[0] * cur[1] * cur[2] // cur[ax]
        flops += 2 * products * size[ax] * cur[ax] * p
        cur[ax], cx = size[ax], True
    return flops


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=None, help="also write the JSON here")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--only", default=None, help="one workload, as N:ON")
    args = ap.parse_args(argv)
    import helicon_amd as H
    from helicon_amd.fft_resample import last_kernel_ms

    loads = WORKLOADS if not args.only else [tuple(int(v) for v in args.only.split(":"))]
    result = dict(f32_matrix_peak=F32_MATRIX_PEAK, reps=args.reps, workloads=[])
    for n, on in loads:
        shape, size = (n, n, n), (on, on, on)
        x = blob(n)
        row = dict(shape=list(shape), new_size=list(size))
        t0 = time.perf_counter()
        ops = [H.resample_operator(a, b) for a, b in zip(shape, size)]
        row["operators_ms"] = 1e3 * (time.perf_counter() - t0)
        del ops
        for kind in ("abs", "real"):
            H.fft_resample(x, 1.0, size, output=kind)   # warm-up
            wall, kern = [], []
            for _ in range(args.reps):
                t0 = time.perf_counter()
                got, _ = H.fft_resample(x, 1.0, size, output=kind)   # synchronous: returns when the map is on the host
                wall.append(1e3 * (time.perf_counter() - t0))
                kern.append(last_kernel_ms())
            t0 = time.perf_counter()
            ref32 = numpy_resample(x, size, kind)
            numpy_ms = 1e3 * (time.perf_counter() - t0)
            del ref32
            want = numpy_resample(x.astype(np.float64), size, kind)
            flops = product_flops(shape, size, kind)
            w, k = float(np.median(wall)), float(np.median(kern))
            row[kind] = dict(wall_ms=w, kernel_ms=k, numpy_ms=numpy_ms, product_gflop=flops / 1e9,
                             product_tflops=flops / (k * 1e-3) / 1e12, share_of_f32_matrix_peak=flops / (k * 1e-3) / F32_MATRIX_PEAK,
                             copies_dominate=bool(w - k > k), speedup_over_numpy_wall=numpy_ms / w,
                             max_error_over_max=float(np.abs(got - want).max() / np.abs(want).max()))
            del want
        result["workloads"].append(row)
    line = json.dumps(result)
    print(line)
    if args.out:
        Path(args.out).write_text(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
