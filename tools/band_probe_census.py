#!/usr/bin/env python3
"""The band-mask probe of tests/spectrum_bands.py over every row length 8 ... 1024 (CPU only, the reference alone): per
length the smallest change of a band's oracle score over all adjacent-column swaps, the same for a kx <-> -kx mirror, the
float32 floor of the reference pipeline and the tolerance that follows from it, for both experimental images of the probe
(each with the candidate it was made from); prints the worst of each (DESIGN.md,
"Row-length census").  With --square: the same figures on the square planes N = 32 ... 1024 of the tuned sweep with the
4 x 8 list of tests/square_bands.py, and the one-line-shift sensitivity of the quadrant masks ("Square-plane
census"; about a minute, N = 1024 most of it).
    python tools/band_probe_census.py [--jobs 8] [--lo 8] [--hi 1024]
    python tools/band_probe_census.py --square [--sizes 32 64 128]"""
import argparse
import sys
from concurrent.futures import ProcessPoolExecutor
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "tests")]
import spectrum_bands as SB  # noqa: E402


def one(nx):
    probe = SB.probe_for_length(nx)
    rows = []
    for log, second in ((True, False), (False, False), (True, True), (False, True)):
        o = SB.OracleSide(probe, log, image=probe.image2 if second else None)
        cand = probe.cand2 if second else 0
        swap, mirror = o.swap_sensitivity(cand), o.mirror_sensitivity(cand)
        band, k = SB.band_of_frequency(nx), np.abs(np.arange(nx) - nx // 2)
        paired = [b for b in range(len(mirror)) if np.any((band == b) & (k > 0) & (2 * k != nx))]   # more than self-mirrored columns
        rows.append((nx, (log, second), len(probe.units), float(swap.min()), float(mirror[paired].min()), float(o.floor.max()), float(o.tol.max()),
                     float((swap / o.tol).min())))
    return rows


def square(sizes):
    """The host table of the square-plane census: one row per size, the worst of log1p|F| and |F|."""
    import square_bands as Q

    print("| N | subunits | kg | smallest swap, \\|kx\\| bands (cand 0 / last) | smallest swap, \\|ky\\| bands (cand 0 / last) | smallest mirror | "
          "largest floor | smallest own score | quadrant masks | smallest one-line shift (image / image2) |")
    print("|---|---|---|---|---|---|---|---|---|---|")
    bad = 0
    for n in sizes or Q.SIZES:
        (_, units, kg, kx0, kx1, ky0, ky1, mirror, floor, own), = Q.host_table((n,))
        f = Q.fold_side(n)
        s0, s1 = f.shift_sensitivity(0), f.shift_sensitivity(1)
        tol = max(SB.ORACLE_TOL, SB.FLOOR_FACTOR * floor)
        bad += min(kx0, kx1, ky0, ky1, mirror) < SB.MARGIN * tol or bool((np.minimum(s0, s1) < SB.MARGIN * f.tol).any()) or own < Q.MIN_OWN_SCORE
        print(f"| {n} | {units} | {kg} | {kx0:.1e} / {kx1:.1e} | {ky0:.1e} / {ky1:.1e} | {mirror:.1e} | {floor:.1e} | {own:.3f} | {len(f.masks)} | "
              f"{s0.min():.1e} / {s1.min():.1e} |", flush=True)
    print(f"{bad} sizes below {SB.MARGIN:.0f} x tolerance or below an own-candidate score of {Q.MIN_OWN_SCORE}")
    return 1 if bad else 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--square", action="store_true", help="the square planes of the tuned sweep (tests/square_bands.py)")
    ap.add_argument("--sizes", type=int, nargs="*", default=None, help="with --square: the sizes (default: all six)")
    ap.add_argument("--jobs", type=int, default=8)
    ap.add_argument("--lo", type=int, default=8)
    ap.add_argument("--hi", type=int, default=1024)
    a = ap.parse_args()
    if a.square:
        return square(a.sizes)
    two, stockham, direct = SB.census()
    family = {**{n: "two-step" for n in two}, **{n: "stockham" for n in stockham}, **{n: "direct" for n in direct}}
    with ProcessPoolExecutor(a.jobs) as ex:
        rows = [r for rs in ex.map(one, range(a.lo, a.hi + 1), chunksize=8) for r in rs]
    for fam in ("two-step", "stockham", "direct"):
        for log in ((True, False), (False, False), (True, True), (False, True)):
            sel = [r for r in rows if family[r[0]] == fam and r[1] == log]
            if not sel:
                continue
            w = min(sel, key=lambda r: r[7])
            print(f"{fam:9s} log={int(log[0])} image {2 if log[1] else 1}: {len(sel)} lengths; smallest swap change {min(r[3] for r in sel):.2e}, smallest mirror change "
                  f"{min(r[4] for r in sel):.2e}, largest float32 floor {max(r[5] for r in sel):.2e}, largest tolerance {max(r[6] for r in sel):.2e}, "
                  f"smallest swap / tolerance {w[7]:.0f} (nx = {w[0]}, {w[2]} subunits)")
    bad = [r for r in rows if r[7] < SB.MARGIN]
    print(f"{len(rows) // 4} lengths, {len(bad)} (length, spectrum) cases below {SB.MARGIN:.0f} x tolerance" + (f": {bad}" if bad else ""))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
