#!/usr/bin/env python3
"""Timing of the sweep's phase score on the zoom bench's workload (tools/zoom_sweep_bench.py): the 512 x 512 image (truth
1.2 degrees, 4.75 A, apix 1), cutoff_res = (4 apix, 4 apix), output_size = (256, 256), 100 x 250 candidates.

    python tools/phase_sweep_bench.py                  # host-timed: the sweep with the phase score, then the zoomed sweep
    python tools/phase_sweep_bench.py --calls 3        # the two sweeps only (run it under rocprofv3 --kernel-trace --stats)
    python tools/phase_sweep_bench.py --stats DIR --calls 3
                                                       # both kernels' times from that run's *kernel_stats.csv, k_phase_sweep's
                                                       # registers from its *kernel_trace.csv, and their ratio

k_phase_sweep does k_zoom_sweep's factor and MFMA work with four accumulator sets instead of two and a longer epilogue;
the ratio of the two kernels' times in one run is what the design sets at 1.25 at the most.  Prints one JSON line."""
import csv
import json
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from tools.zoom_sweep_bench import APIX, CUTOFF, N, SIZE, TRUTH, workload  # noqa: E402

WEIGHT = 0.5


def kernel_name(r):
    return r["Name"].removeprefix("void ").replace("(anonymous namespace)::", "").split("(")[0]


def from_stats(directory, calls, n_cand):
    out = {}
    stats = sorted(Path(directory).rglob("*kernel_stats.csv"))
    by = {}
    with open(stats[0]) as f:
        for r in csv.DictReader(f):
            by[kernel_name(r)] = by.get(kernel_name(r), 0.0) + float(r["TotalDurationNs"])
    out["kernels_ms_per_call"] = {k: v / calls / 1e6 for k, v in sorted(by.items(), key=lambda kv: -kv[1])}
    phase = sum(v for k, v in by.items() if "k_phase_sweep" in k) / calls
    zoom = sum(v for k, v in by.items() if "k_zoom_sweep" in k) / calls
    out["phase_kernel_ms"], out["zoom_kernel_ms"] = phase / 1e6, zoom / 1e6
    out["phase_kernel_candidates_per_s"] = n_cand / (phase * 1e-9)
    out["phase_over_zoom_kernel_time"] = phase / zoom
    for trace in sorted(Path(directory).rglob("*kernel_trace.csv")):
        with open(trace) as f:
            for r in csv.DictReader(f):
                if "k_phase_sweep" in r.get("Kernel_Name", ""):
                    out["phase_kernel_registers"] = {k: int(r[k]) for k in r if "GPR" in k.upper() and r[k].lstrip("-").isdigit()}
                    out["phase_kernel_lds_bytes"] = int(r.get("LDS_Block_Size", 0) or 0)
                    out["phase_kernel_scratch_bytes"] = int(r.get("Scratch_Size", 0) or 0)
                    return out
    return out


def main(argv):
    grid = workload()
    calls = int(argv[argv.index("--calls") + 1]) if "--calls" in argv else 3
    out = dict(image=[N, N], apix=APIX, cutoff_res=list(CUTOFF), output_size=list(SIZE), candidates=len(grid), phase_weight=WEIGHT)
    if "--stats" in argv:
        out.update(from_stats(argv[argv.index("--stats") + 1], calls, len(grid)))
        print(json.dumps(out))
        return
    import helicon_amd as H
    from helicon_amd.grid import radial_band_mask

    d, br = 0.4 * N * APIX, 2 * APIX
    clean = H.simulate_helical_projection(1, *TRUTH, d, br, 0, 0, N, N, APIX)
    img = (clean + np.random.default_rng(0).normal(0, 0.5 * clean.std(), clean.shape)).astype(np.float32)
    mask = radial_band_mask(*SIZE)
    eng = H.SweepEngine(N)
    eng.set_geometry(apix=APIX, helical_diameter=d, ball_radius=br)
    eng.set_zoom(CUTOFF, SIZE)

    def timed(fn, reps):
        fn()   # warm-up
        s = []
        for _ in range(reps):
            t0 = time.perf_counter()
            fn()   # synchronous: returns when the scores are on the host
            s.append(time.perf_counter() - t0)
        return float(np.median(s))

    for name, weight in (("phase", WEIGHT), ("zoom", 0)):
        eng.set_phase_score(weight)
        eng.set_reference(img, mask)
        scores = eng.sweep(grid.params)[0]
        assert eng.last_first_pass == name
        if "--calls" in argv:   # the profiled run: the sweeps, nothing else
            for _ in range(calls - 1):
                eng.sweep(grid.params)
            continue
        t = timed(lambda: eng.sweep(grid.params), 5)
        out[f"{name}_sweep_s"] = t
        out[f"{name}_candidates_per_s"] = len(grid) / t
        out[f"{name}_best"] = [float(v) for v in grid.params[int(np.argmax(scores)), :2]]
    if "--calls" not in argv:
        out["phase_over_zoom_sweep_time"] = out["phase_sweep_s"] / out["zoom_sweep_s"]
    eng.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main(sys.argv[1:])
