#!/usr/bin/env python3
"""Times of the Fourier shell correlation on the device (helicon_amd/fsc.py, csrc/fourier_correlation.inc).

    python tools/fsc_bench.py [--out profiles/fsc.json] [--sizes 64 128 256 512] [--batch 256] [--repeats 5]

Per case — one pair of n^3 maps for every size, and a batch of BATCH pairs of 64^3 — after one warm-up call:

* ``wall_ms``: host clock around ``fsc_sums_3d`` (upload, kernels, download; the call ends in a synchronising copy), the
  median of REPEATS calls;
* ``kernel_ms``: device events around the call's kernels (what the entry point reports), the median;
* ``share_of_f32_matrix_peak``: the DFT products' FLOP, from the shapes, over ``kernel_ms`` and the MI355X's f32 matrix
  peak.  Per map: z pass 2 (n x n)(n x n^2), y pass 2 (n x 2n)(2n x n) per slice, x pass 4 (n^2 x n)(n x n/2+1):
  ``4 n^4 + 8 n^4 + 8 n^3 (n/2 + 1)`` FLOP; it is the whole call's rate over the peak, not one kernel's;
* ``host_ms``: the same sums from ``scipy.fft.rfftn(workers=16)`` + ``bincount`` on the host in this process, and
  ``max_abs_fsc_difference`` between the two curves (the host's transform is float32 too).

For the batch it also times BATCH single calls in the same run: ``singles_wall_ms_per_pair`` against
``wall_ms_per_pair``.  With ``--accuracy FILE`` the FSC_FIGURE lines of a ``pytest tests/test_gpu_fsc.py -s`` log are
parsed into the ``accuracy`` section.  A run without a GPU fails: there is nothing to time.
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

F32_MATRIX_PEAK = 157.3e12   # MI355X, f32 in / f32 accumulate MFMA (= the f32 vector peak)


def product_flops(n: int) -> float:
    """DFT products of ONE pair of n^3 maps (module docstring)."""
    return 2.0 * (4.0 * n**4 + 8.0 * n**4 + 8.0 * n**3 * (n // 2 + 1))


def host_sums(a, b, shell):
    from scipy.fft import rfftn

    f1, f2 = rfftn(a, workers=16), rfftn(b, workers=16)
    s, nb = shell.ravel(), a.shape[0] // 2 + 1
    return np.stack([np.bincount(s, weights=np.real(f1 * np.conj(f2)).ravel(), minlength=nb),
                     np.bincount(s, weights=(np.abs(f1) ** 2).ravel(), minlength=nb),
                     np.bincount(s, weights=(np.abs(f2) ** 2).ravel(), minlength=nb)], axis=1)


def median_ms(fn, repeats):
    walls, kernels = [], []
    for _ in range(repeats):
        t = time.perf_counter()
        _, ms = fn()
        walls.append((time.perf_counter() - t) * 1e3)
        kernels.append(ms)
    return float(np.median(walls)), float(np.median(kernels))


def parse_figures(path):
    out = {}
    for line in Path(path).read_text().splitlines():
        m = re.search(r"FSC_FIGURE (.*)$", line)
        if not m:
            continue
        words = m.group(1).split()
        key = " ".join(w for w in words if "=" not in w or w.split("=")[0] in ("n", "shape", "full", "apix"))
        out[key] = {w.split("=")[0]: w.split("=", 1)[1] for w in words if "=" in w and w.split("=")[0] not in ("n", "shape", "full", "apix")}
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=None)
    ap.add_argument("--sizes", type=int, nargs="*", default=[64, 128, 256, 512])
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--accuracy", default=None, help="log of `pytest tests/test_gpu_fsc.py -s` to take the measured errors from")
    args = ap.parse_args(argv)

    import fsc_oracle as O
    from helicon_amd import fsc as F

    result = {"f32_matrix_peak_flops": F32_MATRIX_PEAK, "repeats": args.repeats, "cases": []}
    for n in args.sizes:
        a, b = O.make_map_pair(n, 300 + n)
        F.fsc_sums_3d(a, b)   # warm-up: code objects, first allocations
        wall, kern = median_ms(lambda: F.fsc_sums_3d(a, b, return_kernel_ms=True), args.repeats)
        shell = O.shell_3d_half(n)
        host_sums(a, b, shell)
        t = time.perf_counter()
        hs = host_sums(a, b, shell)
        host = (time.perf_counter() - t) * 1e3
        diff = float(np.abs(O.ratio(F.fsc_sums_3d(a, b)) - O.ratio(hs)).max())
        case = dict(case=f"1 x {n}^3", n=n, pairs=1, wall_ms=wall, kernel_ms=kern, product_gflop=product_flops(n) / 1e9,
                    share_of_f32_matrix_peak=product_flops(n) / (kern * 1e-3) / F32_MATRIX_PEAK, host_ms=host, max_abs_fsc_difference=diff)
        result["cases"].append(case)
        print(json.dumps(case), flush=True)
    if args.batch > 0:
        n, nb = 64, args.batch
        rng = np.random.default_rng(7)
        sig = rng.standard_normal((nb, n, n, n)).astype(np.float32)
        a = sig + rng.standard_normal(sig.shape).astype(np.float32)
        b = sig + rng.standard_normal(sig.shape).astype(np.float32)
        F.fsc_sums_3d(a, b)
        wall, kern = median_ms(lambda: F.fsc_sums_3d(a, b, return_kernel_ms=True), max(2, args.repeats // 2))
        t = time.perf_counter()
        singles = np.stack([F.fsc_sums_3d(a[i], b[i]) for i in range(nb)])
        singles_wall = (time.perf_counter() - t) * 1e3
        shell = O.shell_3d_half(n)
        t = time.perf_counter()
        for i in range(min(nb, 16)):
            host_sums(a[i], b[i], shell)
        host = (time.perf_counter() - t) * 1e3 / min(nb, 16)
        case = dict(case=f"{nb} x {n}^3", n=n, pairs=nb, wall_ms=wall, kernel_ms=kern, wall_ms_per_pair=wall / nb,
                    kernel_ms_per_pair=kern / nb, singles_wall_ms_per_pair=singles_wall / nb,
                    batch_equals_singles_bitwise=bool(np.array_equal(singles, F.fsc_sums_3d(a, b))),
                    product_gflop=product_flops(n) * nb / 1e9,
                    share_of_f32_matrix_peak=product_flops(n) * nb / (kern * 1e-3) / F32_MATRIX_PEAK, host_ms_per_pair=host)
        result["cases"].append(case)
        print(json.dumps(case), flush=True)
    if args.accuracy:
        result["accuracy"] = parse_figures(args.accuracy)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(result, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
