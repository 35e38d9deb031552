"""Pixel-size calibration (helicon_amd/pixel_size.py, csrc/nudft.inc) on the device: accuracy against the float64 direct sum
and speed.

    python tools/pixel_size_bench.py [--out profiles/pixel_size.json] [--reps 2] [--sample 512] [--accuracy-only] [--speed-only]
    python tools/pixel_size_bench.py --probes [--out profiles/pixel_size.json]

``accuracy``: over every comparison of tests/test_gpu_pixel_size.py (``pixel_size_cases.accuracy_cases``: the point shapes,
counts and stacks, the long sides, the offset image, the full band) the largest ``|F_device - F_yardstick| / sum |f - mean|``
of the complex and of the abs output; the tests' bound ``B`` is four times the largest, rounded up to one significant digit.

``speed``: the ring maximum of the full graphene band at 1.0 A / pixel (3103 angles x 100 radii) of one 4096 x 4096
micrograph and of 256 particles of 256 x 256: wall clock of the call (upload and the host's float64 mean included) and
device-event milliseconds of its kernels, best of ``--reps``; the product's share of the MI355X's f32 matrix peak (4 FLOP
per point, pixel: a real image value times a complex factor, multiply and add); and the NumPy two-stage composition (the
yardstick) timed in the same run on ``--sample`` points and scaled to the band.  A run without a GPU fails.

``--probes``: the closed-form probe list of tests/nudft_probes.py, as tests/test_gpu_nudft_probes.py walks it: per family the
largest error over that list's own allowance (complex and abs outputs), and the probe it occurs on.  Only the ``probes`` key
of ``--out`` is rewritten; the file's other keys stay.  It is a record: no tolerance is derived from it.
"""
import argparse
import json
import math
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

F32_MATRIX_PEAK = 157.3e12   # MI355X, f32 in / f32 accumulate MFMA


def round_up_one_digit(v):
    if v <= 0:
        return 0.0
    e = math.floor(math.log10(v))
    return float(f"{math.ceil(v / 10 ** e - 1e-12) * 10.0 ** e:.1g}")


def accuracy():
    import pixel_size_cases as Y
    from helicon_amd import pixel_size as PS

    out = dict(cases=[], max_error_over_scale=0.0)
    for label, f, x, y in Y.accuracy_cases(PS.nudft_chunk()):
        want = Y.yardstick(x, y, f)
        s = Y.scale(f)[:, None]
        s = np.where(s > 0, s, np.inf)
        e_c = float((np.abs(PS.nudft2d2(x, y, f).astype(np.complex128) - want) / s).max())
        e_a = float((np.abs(PS.nudft2d2(x, y, f, output="abs").astype(np.float64) - np.abs(want)) / s).max())
        out["cases"].append(dict(case=label, points=int(x.size), complex=e_c, abs=e_a))
        if max(e_c, e_a) > out["max_error_over_scale"]:
            out["max_error_over_scale"], out["worst_case"] = max(e_c, e_a), label
        print(f"{label}: complex {e_c:.3e}, abs {e_a:.3e}", flush=True)
    out["B"] = round_up_one_digit(4 * out["max_error_over_scale"])
    out["f32_unit_roundoff"] = float(np.finfo(np.float32).eps / 2)
    return out


def speed(reps, sample):
    import pixel_size_cases as Y
    from helicon_amd import pixel_size as PS

    X, Yp, R, theta = Y.band()
    out = dict(points=int(X.size), theta_samples=int(theta), r_samples=int(len(R)), workloads=[])
    rng = np.random.default_rng(0)
    for name, shape in (("one 4096 x 4096 micrograph", (1, 4096, 4096)), ("256 particles of 256 x 256", (256, 256, 256))):
        f = rng.standard_normal(shape, dtype=np.float32)
        PS.ring_maximum(X[:6400], Yp[:6400], f[:1], 100)                       # first touch of the device and the code object
        wall, kern = [], []
        for _ in range(reps):
            t0 = time.perf_counter()
            ring = PS.ring_maximum(X, Yp, f, 100)
            wall.append(time.perf_counter() - t0)
            kern.append(PS.last_kernel_ms() * 1e-3)
        flop = 4.0 * X.size * f.size
        pick = np.linspace(0, X.size - 1, sample).astype(np.int64)
        t0 = time.perf_counter()
        want = Y.yardstick(X[pick], Yp[pick], f[:4])
        numpy_s = (time.perf_counter() - t0) * (X.size / sample) * (len(f) / len(f[:4]))
        got = PS.nudft2d2(X[pick], Yp[pick], f[:4], output="abs")
        err = float((np.abs(got - np.abs(want)) / Y.scale(f[:4])[:, None]).max())
        row = dict(workload=name, wall_s=min(wall), kernel_s=min(kern), product_flop=flop, product_tflops=flop / min(kern) / 1e12,
                   share_of_f32_matrix_peak=flop / min(kern) / F32_MATRIX_PEAK, numpy_two_stage_s_scaled=numpy_s,
                   numpy_sample_points=int(sample), numpy_sample_images=int(len(f[:4])), sample_error_over_scale=err,
                   ring_maximum_range=[float(ring.min()), float(ring.max())])
        out["workloads"].append(row)
        print(json.dumps(row), flush=True)
    return out


def probes():
    import nudft_probes as Q
    from helicon_amd import pixel_size as PS

    assert PS.nudft_chunk() == Q.CHUNK
    out = dict(bound="B sum|f - mean| + 2^-23 |want| + ny nx (ny + nx) 2^-53 |mean|", families={})
    for probe in Q.probes():
        f, (x, y) = Q.images(probe), Q.points(probe)
        idx = slice(None) if probe.pick is None else np.array(probe.pick)
        want = Q.expect(probe, None if probe.pick is None else idx)
        lim = Q.allowance(f, want)
        e_c = Q.share(PS.nudft2d2(x, y, f)[:, idx].astype(np.complex128), want, lim)
        e_a = Q.share(PS.nudft2d2(x, y, f, output="abs")[:, idx].astype(np.float64), np.abs(want), lim)
        row = out["families"].setdefault(probe.family, dict(probes=0, images=0, complex=0.0, abs=0.0, worst_probe=None))
        if max(e_c, e_a) > max(row["complex"], row["abs"]) or row["worst_probe"] is None:
            row["worst_probe"] = probe.label
        row.update(probes=row["probes"] + 1, images=row["images"] + len(f), complex=max(row["complex"], e_c), abs=max(row["abs"], e_a))
    for family, row in out["families"].items():
        print(f"{family}: {json.dumps(row)}", flush=True)
    out["max_error_over_allowance"] = max(max(r["complex"], r["abs"]) for r in out["families"].values())
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--sample", type=int, default=512)
    ap.add_argument("--accuracy-only", action="store_true")
    ap.add_argument("--speed-only", action="store_true")
    ap.add_argument("--probes", action="store_true", help="walk tests/nudft_probes.py and rewrite the 'probes' key of --out alone")
    args = ap.parse_args(argv)
    if args.probes:
        res = json.loads(Path(args.out).read_text()) if args.out and Path(args.out).exists() else {}
        res["probes"] = probes()
        if args.out:
            Path(args.out).parent.mkdir(parents=True, exist_ok=True)
            Path(args.out).write_text(json.dumps(res, indent=1) + "\n")
        print(json.dumps({k: v for k, v in res["probes"].items() if k != "families"}))
        return 0
    res = dict(f32_matrix_peak_flops=F32_MATRIX_PEAK)
    if not args.speed_only:
        res["accuracy"] = accuracy()
    if not args.accuracy_only:
        res["speed"] = speed(args.reps, args.sample)
    text = json.dumps(res, indent=1)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(text + "\n")
    print(json.dumps({k: v for k, v in res.get("accuracy", {}).items() if k != "cases"}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
