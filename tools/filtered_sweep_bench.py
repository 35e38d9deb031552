#!/usr/bin/env python3
"""Timing of the sweep on low / high-pass filtered spectra: the workload of tools/zoom_sweep_bench.py (the benchmark's
512 x 512 image, truth 1.2 degrees / 4.75 A, apix 1, cutoff_res = (4 apix, 4 apix), output_size = (256, 256), a twist-major
grid of 100 x 250 candidates) for high_pass_fraction = 0.02 alone and for low_pass_fraction = 0.3 with it.

    python tools/filtered_sweep_bench.py                            # filtered sweeps, the unfiltered zoom sweep, the per-candidate loop
    python tools/filtered_sweep_bench.py --calls 3 --filter 0 0.02  # that filter's batched sweep only (run it under rocprofv3 --kernel-trace --stats)
    python tools/filtered_sweep_bench.py --stats FILE --calls 3 --filter 0 0.02   # per-kernel times and the filter passes' share of the f32 matrix peak

The per-candidate loop is the only route to these scores without the batched form: ``simulate_helical_projection`` ->
``compute_power_spectra(..., low_pass_fraction, high_pass_fraction)`` -> ``cross_correlation_coefficient``, timed over 64
candidates of the same grid.  Prints one JSON line (profiles/filtered_sweep.json keeps the lines of one such session)."""
import csv
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

F32_MATRIX_PEAK = 157.3e12   # MI355X, f32 in / f32 accumulate MFMA
N, APIX, TRUTH = 512, 1.0, (1.2, 4.75, 1)
SIZE = (256, 256)
CUTOFF = (4 * APIX, 4 * APIX)
FILTERS = [(0.0, 0.02), (0.3, 0.02)]
TERM_FLOP = 2 * 2 * SIZE[0] * SIZE[1] * SIZE[1]   # one separable term of one candidate: the y pass and the x pass


def workload():
    from helicon_amd.grid import build_grid, sweep_axis

    return build_grid(sweep_axis(0.71, 1.70, 0.01), sweep_axis(4.000, 5.245, 0.005), (1,), tube_length=N * APIX)


def terms(lp, hp):
    """Separable terms of the operator on even sides: one per Gaussian (low pass alone, high pass alone: 1; both: 2)."""
    return 2 if (0 < lp < 1 and 0 < hp < 1) else 1


def kernel_name(row):
    return row["Name"].removeprefix("void ").replace("(anonymous namespace)::", "").split("(")[0]


def main(argv):
    grid = workload()
    d, br = 0.4 * N * APIX, 2 * APIX
    out = dict(image=[N, N], apix=APIX, cutoff_res=list(CUTOFF), output_size=list(SIZE), candidates=len(grid),
               filter_mflop_per_term_and_candidate=TERM_FLOP / 1e6)
    one = tuple(float(v) for v in argv[argv.index("--filter") + 1: argv.index("--filter") + 3]) if "--filter" in argv else FILTERS[0]
    calls = int(argv[argv.index("--calls") + 1]) if "--calls" in argv else 3
    if "--stats" in argv:
        with open(argv[argv.index("--stats") + 1]) as f:
            rows = list(csv.DictReader(f))
        by = {}
        for r in rows:
            by[kernel_name(r)] = by.get(kernel_name(r), 0.0) + float(r["TotalDurationNs"])
        out["filter"] = list(one)
        out["kernels_ms_per_call"] = {k: v / calls / 1e6 for k, v in sorted(by.items(), key=lambda kv: -kv[1])}
        ns = sum(v for k, v in by.items() if "k_circ_gemm" in k or "k_filter_xpass" in k) / calls
        out["filter_kernels_ms"] = ns / 1e6
        out["filter_share_of_f32_matrix_peak"] = terms(*one) * TERM_FLOP * len(grid) / (ns * 1e-9) / F32_MATRIX_PEAK
        print(json.dumps(out))
        return
    import helicon_amd as H
    from helicon_amd.grid import radial_band_mask

    clean = H.simulate_helical_projection(1, *TRUTH, d, br, 0, 0, N, N, APIX)
    img = (clean + np.random.default_rng(0).normal(0, 0.5 * clean.std(), clean.shape)).astype(np.float32)
    mask = radial_band_mask(*SIZE)
    eng = H.SweepEngine(N)
    eng.set_geometry(apix=APIX, helical_diameter=d, ball_radius=br)
    eng.set_zoom(CUTOFF, SIZE)
    if "--calls" in argv:   # the profiled run: one filter's batched sweep, nothing else
        eng.set_filter(*one)
        eng.set_reference(img, mask)
        for _ in range(calls):
            eng.sweep(grid.params)
        out["filter"] = list(one)
        print(json.dumps(out))
        return

    def timed(fn, reps=3):
        fn()   # warm-up
        s = []
        for _ in range(reps):
            t0 = time.perf_counter()
            fn()   # synchronous: returns when the scores are on the host
            s.append(time.perf_counter() - t0)
        return float(np.median(s))

    eng.set_reference(img, mask)
    eng.sweep(grid.params)
    assert eng.last_first_pass == "zoom"
    t = timed(lambda: eng.sweep(grid.params))
    out["unfiltered_zoom_candidates_per_s"] = len(grid) / t
    pick = np.arange(64) * (len(grid) // 64)   # every 390th candidate: spread over twists and rises
    out["filters"] = []
    for lp, hp in FILTERS:
        rec = dict(low_pass_fraction=lp, high_pass_fraction=hp, terms=terms(lp, hp))
        eng.set_filter(lp, hp)
        eng.set_reference(img, mask)
        scores = eng.sweep(grid.params)[0]
        assert eng.last_first_pass == "filtered"
        t = timed(lambda: eng.sweep(grid.params))
        rec["sweep_s"] = t
        rec["candidates_per_s"] = len(grid) / t
        rec["fraction_of_unfiltered"] = rec["candidates_per_s"] / out["unfiltered_zoom_candidates_per_s"]
        rec["best"] = [float(v) for v in grid.params[int(np.argmax(scores)), :2]]
        e_ref = H.compute_power_spectra(img, APIX, CUTOFF, SIZE, True, lp, hp)[0]

        def loop():
            res = []
            for tw, rs, cs, _ in grid.params[pick]:
                sim = H.simulate_helical_projection(1, tw, rs, int(cs), d, br, 0, 0, N, N, APIX)
                p = H.compute_power_spectra(sim, APIX, CUTOFF, SIZE, True, lp, hp)[0]
                res.append(H.cross_correlation_coefficient(e_ref[mask], p[mask]))
            return np.array(res)

        looped = loop()
        rec["loop_max_abs_score_difference"] = float(np.abs(looped - scores[pick]).max())
        rec["loop_candidates_per_s"] = len(pick) / timed(loop, reps=2)
        rec["sweep_over_loop"] = rec["candidates_per_s"] / rec["loop_candidates_per_s"]
        out["filters"].append(rec)
    eng.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main(sys.argv[1:])
