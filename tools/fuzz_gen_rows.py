#!/usr/bin/env python3
"""Every row length the row-transform kernels serve (109 two-step pairs of gen_rows.hip, 326 Stockham-only lengths)
against the NumPy oracle under the kx-band masks of tests/spectrum_bands.py — masks that together see every spectrum
column, on the probe geometry whose spectrum has no empty column — and against the other device paths (run on the GPU
box; the suite's own census is tests/test_gpu_row_lengths.py, this prints the figures per length):
    python tools/fuzz_gen_rows.py [two-step|stockham|all] [ny]"""
import os
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "tests")]
import helicon_amd as H  # noqa: E402
import spectrum_bands as SB  # noqa: E402

family = sys.argv[1] if len(sys.argv) > 1 else "two-step"
ny = int(sys.argv[2]) if len(sys.argv) > 2 else SB.NY
two, stockham, _ = SB.census()
sizes = sorted(two) * (family in ("two-step", "all")) + stockham * (family in ("stockham", "all"))
print(f"{len(sizes)} row lengths, ny = {ny}", flush=True)


def swept(eng, probe, masks, log, switch=None):
    if switch:
        os.environ[switch] = "1"
    try:
        got, kernel = SB.device_scores(eng, probe, masks, log)
        return got[:, 0], kernel
    finally:
        if switch:
            del os.environ[switch]


worst, worst_vs = 0.0, 0.0
for nx in sorted(sizes):
    probe = SB.probe_for_length(nx, ny)
    with H.SweepEngine((ny, nx)) as eng:
        eng.set_geometry(**probe.geometry())
        for log in (True, False):
            o = SB.OracleSide(probe, log)
            got, kernel = swept(eng, probe, o.masks, log)
            err = np.abs(got - o.scores).max(axis=1)
            vs = float(np.abs(swept(eng, probe, o.masks, log, "HH_GEN_DIRECT")[0] - got).max())
            if kernel[0] and probe.stockham_lds() <= SB.LDS_LIMIT:
                vs = max(vs, float(np.abs(swept(eng, probe, o.masks, log, "HH_GEN_STOCKHAM")[0] - got).max()))
            worst, worst_vs = max(worst, float(err.max())), max(worst_vs, vs)
            flag = "" if (err <= o.tol).all() and vs <= SB.PATHS_TOL else "   <-- CHECK"
            print(f"nx {nx:4d} kernel {kernel} log {int(log)}: |score - oracle| {err.max():.2e} (band {int(err.argmax())} of {len(err)}, "
                  f"tolerance {o.tol[int(err.argmax())]:.1e}), between device paths {vs:.2e}{flag}", flush=True)
print(f"done: {len(sizes)} sizes, worst against the oracle {worst:.2e}, between device paths {worst_vs:.2e}")
