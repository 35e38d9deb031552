#!/usr/bin/env python3
"""Timing of the sweep on Fourier-zoomed spectra: the benchmark workload's 512 x 512 image (truth 1.2 degrees, 4.75 A,
apix 1), cutoff_res = (4 apix, 4 apix), output_size = (256, 256), a twist-major grid of 100 x 250 candidates.

    python tools/zoom_sweep_bench.py                     # batched sweep, the three-call loop, the default-sampling sweep
    python tools/zoom_sweep_bench.py --calls 3           # the batched sweep only (run it under rocprofv3 --kernel-trace --stats)
    python tools/zoom_sweep_bench.py --stats FILE        # k_zoom_sweep's share of the f32 matrix peak from that run's kernel_stats.csv

The three-call loop is what a user had before the batched form: per candidate ``simulate_helical_projection`` ->
``compute_power_spectra(cutoff_res=..., output_size=...)`` -> ``cross_correlation_coefficient``, timed over 64 candidates of
the same grid.  The default-sampling sweep under ``radial_band_mask(512, 512, r_hi=128)`` covers the same band of
frequencies at half the sampling density: it is NOT the same computation and is printed for orientation only.
Prints one JSON line."""
import csv
import json
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

F32_MATRIX_PEAK = 157.3e12   # MI355X, f32 in / f32 accumulate MFMA (= the f32 vector peak)
N, APIX, TRUTH = 512, 1.0, (1.2, 4.75, 1)
SIZE = (256, 256)
CUTOFF = (4 * APIX, 4 * APIX)
TILE_U, TILE_V, K_SLICE = 128, 128, 32   # k_zoom_sweep's output tile and K slice (csrc/zoom_sweep.inc)


def workload():
    from helicon_amd.grid import build_grid, sweep_axis

    twists = sweep_axis(0.71, 1.70, 0.01)        # 100 twists around the truth
    rises = sweep_axis(4.000, 5.245, 0.005)      # 250 rises: the benchmark's own axis
    return build_grid(twists, rises, (1,), tube_length=N * APIX)


def centres_in_image(rise, rpx):
    """Lattice centres of one candidate whose footprint meets the image (no tilt: the axial coordinate is i * rise)."""
    imax = int(np.ceil(N * APIX / rise))
    return int(2 * min(imax, np.floor((N / 2 + rpx) * APIX / rise)) + 1)


def product_flops(params, rpx):
    """8 x rows x C x onx per candidate: (useful, issued) — issued counts whole output tiles and K slices."""
    c = np.array([centres_in_image(r, rpx) for r in params[:, 1]], dtype=np.float64)
    rows_i = -(-SIZE[0] // TILE_U) * TILE_U
    cols_i = -(-SIZE[1] // TILE_V) * TILE_V
    return float(np.mean(8.0 * SIZE[0] * c * SIZE[1])), float(np.mean(8.0 * rows_i * (np.ceil(c / K_SLICE) * K_SLICE) * cols_i))


def main(argv):
    grid = workload()
    d, br = 0.4 * N * APIX, 2 * APIX
    rpx = int(np.ceil(np.sqrt(br * br / np.log(2) * 24 * np.log(2)) / APIX))
    useful, issued = product_flops(grid.params, rpx)
    out = dict(image=[N, N], apix=APIX, cutoff_res=list(CUTOFF), output_size=list(SIZE), candidates=len(grid),
               product_mflop_per_candidate=useful / 1e6, product_mflop_issued_per_candidate=issued / 1e6,
               # by arithmetic: the candidate's parameters in (32 B), one score out (4 B); per output tile three float64
               # partial moments written and read once; the weights {w, w (E - Ebar)} (2 x 4 B x 256 x 256) stay in L2
               hbm_bytes_per_candidate=32 + 4 + 2 * 24 * (-(-SIZE[0] // TILE_U)) * (-(-SIZE[1] // TILE_V)))
    if "--stats" in argv:
        path = argv[argv.index("--stats") + 1]
        calls = int(argv[argv.index("--calls") + 1]) if "--calls" in argv else 3
        with open(path) as f:
            rows = list(csv.DictReader(f))
        name = lambda r: r["Name"].removeprefix("void ").replace("(anonymous namespace)::", "").split("(")[0]  # noqa: E731
        by = {}
        for r in rows:
            by[name(r)] = by.get(name(r), 0.0) + float(r["TotalDurationNs"])
        ns = sum(v for k, v in by.items() if "k_zoom_sweep" in k) / calls
        out["kernels_ms_per_call"] = {k: v / calls / 1e6 for k, v in sorted(by.items(), key=lambda kv: -kv[1])}
        out["zoom_kernel_ms"] = ns / 1e6
        out["zoom_kernel_candidates_per_s"] = len(grid) / (ns * 1e-9)
        out["product_share_of_f32_matrix_peak"] = useful * len(grid) / (ns * 1e-9) / F32_MATRIX_PEAK
        out["product_share_of_f32_matrix_peak_issued"] = issued * len(grid) / (ns * 1e-9) / F32_MATRIX_PEAK
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
    eng.set_reference(img, mask)
    if "--calls" in argv:   # the profiled run: the batched sweep, nothing else
        for _ in range(int(argv[argv.index("--calls") + 1])):
            eng.sweep(grid.params)
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

    scores = eng.sweep(grid.params)[0]
    assert eng.last_first_pass == "zoom"
    t = timed(lambda: eng.sweep(grid.params))
    out["zoom_sweep_s"] = t
    out["zoom_candidates_per_s"] = len(grid) / t
    out["zoom_best"] = [float(v) for v in grid.params[int(np.argmax(scores)), :2]]

    # the three-call loop over 64 candidates of the same grid (every 390th: spread over twists and rises)
    pick = np.arange(64) * (len(grid) // 64)
    e_ref = H.compute_power_spectra(img, APIX, CUTOFF, SIZE)[0]

    def loop():
        res = []
        for tw, rs, cs, _ in grid.params[pick]:
            sim = H.simulate_helical_projection(1, tw, rs, int(cs), d, br, 0, 0, N, N, APIX)
            p = H.compute_power_spectra(sim, APIX, CUTOFF, SIZE)[0]
            res.append(H.cross_correlation_coefficient(e_ref[mask], p[mask]))
        return np.array(res)

    looped = loop()
    out["loop_max_abs_score_difference"] = float(np.abs(looped - scores[pick]).max())
    t = timed(loop, reps=2)
    out["loop_candidates_per_s"] = len(pick) / t
    out["zoom_over_loop"] = out["zoom_candidates_per_s"] / out["loop_candidates_per_s"]

    # orientation only: the default sampling under the band r < 128 — the same frequencies at half the density
    eng.set_zoom()
    eng.set_reference(img, radial_band_mask(N, N, r_hi=128))
    eng.sweep(grid.params)
    out["default_sampling_first_pass"] = eng.last_first_pass
    t = timed(lambda: eng.sweep(grid.params))
    out["default_sampling_candidates_per_s"] = len(grid) / t
    eng.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main(sys.argv[1:])
