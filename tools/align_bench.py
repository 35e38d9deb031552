"""Batched image alignment (helicon_amd/align.py) on the device: accuracy against the float64 yardstick and speed.

    python tools/align_bench.py [--out profiles/align.json] [--side 256] [--reps 3] [--sample 24] [--accuracy-only]

``accuracy``: over the cases of tests/align_cases.py (13 angles x 4 scales x 2 polarities on an image and its flip, five
shapes) the largest ``|c_device - c_yardstick| / peak`` of the correlation surface and, over the candidates whose shift
agrees and that have no borderline pixel, the largest ``|score_device - score_yardstick|``; the tests' two bounds are four
times these figures.  Also the candidates whose shift or mask count differs, with the yardstick's gap at each.

``speed``: one side x side class average against one reference, 361 angles x 9 scales x 2 polarities x 2 flips through one
``evaluate`` call: candidates per second (wall clock, best of ``--reps``), device-event milliseconds per phase, the DFT
products' share of the MI355X's f32 matrix peak (their FLOP from the shapes over the forward, inverse and c2r phases), and,
timed in the same run on ``--sample`` candidates, the per-candidate loop over the existing single-image device call
(``transform_image`` for the first warp, the rest of the evaluation in NumPy) and the NumPy yardstick alone.  A run without a
GPU fails.
"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

F32_MATRIX_PEAK = 157.3e12   # MI355X, f32 in / f32 accumulate MFMA


def product_flops(ny, nx):
    """FLOP of one candidate's DFT products: x pass (two real products), the complex y pass forward and inverse (four
    each), the c2r pass (two)."""
    ncol = nx // 2 + 1
    return 2.0 * (2 * ncol * nx * ny) + 2 * 4.0 * (2 * ny * ny * ncol) + 2.0 * (2 * ny * ncol * nx)


def accuracy():
    import align_cases as Y
    from helicon_amd.align import AlignContext

    cand = Y.candidates()
    sc, an, pl = (np.array(v) for v in zip(*cand))
    out = dict(cases=[], max_rel_surface_difference=0.0, max_abs_score_difference=0.0)
    for k, (ref_shape, mov_shape) in enumerate(Y.CASES):
        ref_work, work, taper, _ = Y.case_planes(k)
        yard = Y.case_yardstick(k)
        with AlignContext.from_planes(ref_work, work, taper) as ctx:
            dev = ctx.evaluate(sc, an, pl)
            surf = max(float(np.abs(ctx.correlation(s, a, p).astype(np.float64) - e["surface"]).max() / e["peak"])
                       for (s, a, p), e in zip(cand, yard))
        agree = np.array([tuple(dev.shifts[i]) == e["shift"] for i, e in enumerate(yard)])
        clean = agree & np.array([e["borderline"] == 0 for e in yard])
        dscore = np.abs(dev.scores - np.array([e["score"] for e in yard]))
        nm_equal = dev.nmask == np.array([e["nmask"] for e in yard])
        dpeak = np.abs(dev.peaks - np.array([e["peak"] for e in yard])) / np.array([e["peak"] for e in yard])
        case = dict(ref_shape=list(ref_shape), moving_shape=list(mov_shape), candidates=len(cand),
                    max_rel_surface_difference=surf, max_abs_score_difference=float(dscore[clean].max()),
                    max_rel_peak_difference=float(dpeak.max()),
                    shifts_differ=[dict(candidate=list(cand[i]), gap=yard[i]["gap"]) for i in np.flatnonzero(~agree)],
                    mask_counts_differ=[dict(candidate=list(cand[i]), borderline=yard[i]["borderline"]) for i in np.flatnonzero(agree & ~nm_equal)],
                    smallest_gap=float(min(e["gap"] for e in yard)))
        print("ALIGN_FIGURE", json.dumps(case), flush=True)
        out["cases"].append(case)
        out["max_rel_surface_difference"] = max(out["max_rel_surface_difference"], surf)
        out["max_abs_score_difference"] = max(out["max_abs_score_difference"], case["max_abs_score_difference"])
    return out


def speed(side, reps, sample):
    import align_cases as Y
    import helicon_amd as H
    from helicon_amd.align import AlignContext

    ref, mov = Y.make_pair((side, side), (side, side), 500 + side)
    angles, scales = np.arange(-180.0, 181.0, 1.0), 1.0 + 0.0125 * np.arange(-4, 5)
    with AlignContext(ref, [mov, mov[::-1, :]]) as ctx:
        shape = (2, 2, scales.size, angles.size)
        pl = np.broadcast_to(np.arange(2).reshape(2, 1, 1, 1), shape).ravel()
        sc = np.broadcast_to(scales.reshape(1, 1, -1, 1), shape).ravel()
        an = np.broadcast_to(angles.reshape(1, 1, 1, -1) + 180.0 * np.arange(2).reshape(1, 2, 1, 1), shape).ravel()
        from helicon_amd.align import inverse_matrices

        inv = inverse_matrices(ctx.shape, sc, an)
        ctx.evaluate_matrices(inv[:128], pl[:128])       # warm-up
        walls = []
        for _ in range(reps):
            t0 = time.perf_counter()
            first = ctx.evaluate_matrices(inv, pl)
            walls.append(time.perf_counter() - t0)
        ctx.profile(True)
        again = ctx.evaluate_matrices(inv, pl)
        phases = ctx.profile(False)
        identical = bool(np.array_equal(first.shifts, again.shifts) and np.array_equal(first.scores, again.scores, equal_nan=True))
        n = len(inv)
        prod_ms = phases["forward"] + phases["inverse_y"] + phases["c2r_argmax"]
        # the per-candidate loop a caller had before: the first warp on the device, everything else on the host
        ref_work, work, taper = ctx.ref_work, ctx.moving_work, ctx.taper
        pick = np.linspace(0, n - 1, sample).astype(int)
        t0 = time.perf_counter()
        for i in pick:
            w = H.transform_image(work[pl[i]], scale=float(sc[i]), rotation=float(an[i]))
            _, c = Y.cross_power(ref_work, w)
            h = Y.shifted(Y.inverse_matrix(ref_work.shape, sc[i], an[i]), Y.shift_of(c))
            m = Y.warp_wrap(taper[pl[i]], h) > 0
            Y.pearson(ref_work[m].astype(np.float64), Y.warp_wrap(work[pl[i]], h)[m])
        loop_s = (time.perf_counter() - t0) / sample
        t0 = time.perf_counter()
        for i in pick:
            Y.evaluate(ref_work, work[pl[i]], taper[pl[i]], sc[i], an[i])
        numpy_s = (time.perf_counter() - t0) / sample
    best = min(walls)
    return dict(side=side, candidates=n, angles=int(angles.size), scales=int(scales.size), reps=reps, wall_s=walls,
                candidates_per_s=n / best, phase_ms=phases, kernel_ms=sum(phases.values()),
                product_tflops=product_flops(side, side) * n / (prod_ms * 1e-3) / 1e12,
                products_share_of_f32_matrix_peak=product_flops(side, side) * n / (prod_ms * 1e-3) / F32_MATRIX_PEAK,
                two_runs_identical=identical, sample=sample,
                single_image_loop_s_per_candidate=loop_s, numpy_yardstick_s_per_candidate=numpy_s,
                speedup_over_single_image_loop=loop_s * n / best, speedup_over_numpy=numpy_s * n / best)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=None)
    ap.add_argument("--side", type=int, default=256)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--sample", type=int, default=24)
    ap.add_argument("--accuracy-only", action="store_true")
    args = ap.parse_args(argv)
    result = dict(f32_matrix_peak_flops=F32_MATRIX_PEAK, accuracy=accuracy())
    if not args.accuracy_only:
        result["speed"] = speed(args.side, args.reps, args.sample)
        print("ALIGN_SPEED", json.dumps(result["speed"]), flush=True)
    text = json.dumps(result, indent=1)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(text + "\n")
    print(json.dumps({k: v for k, v in result["accuracy"].items() if k != "cases"}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
