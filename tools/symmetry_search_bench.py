#!/usr/bin/env python3
"""Timing of the helical symmetry search of a 3-D map at a size users search: a seeded synthetic helix, 128^3 voxels at
2 Angstrom, 60 twists x 50 rises, Csym 1.

    python tools/symmetry_search_bench.py [--n 128] [--repeats 5] [--out profiles/symmetry_search.json]
    python tools/symmetry_search_bench.py --calls 3      # three searches of the grid and nothing else (for rocprofv3 --kernel-trace --stats)

What is measured (medians of --repeats runs after a warm-up of each shape; host clocks end in a device synchronise):
  * end to end, default region: candidates / s of ``SymmetrySearch.search`` on the whole grid, list upload and the copy of
    the scores included (the map is uploaded once, outside);
  * the same for 64 candidates of that grid through the loop there was before the search: ``apply_helical_symmetry`` +
    ``cross_correlation_coefficient`` per candidate on the same device, with the largest score difference of the two;
  * like for like, the whole volume scored (rmax none, z_fraction 1): per candidate, the search's device time (events
    around its kernels, one candidate per search) beside ``hh_apply_helical_symmetry``'s own ``kernel_ms``, back to back in
    this process, and the median over the 64 candidates of each and of their ratio;
  * samples / s and gathers / s of the search kernel from the number of (voxel, repeat, copy) samples it tests, counted
    on the host from the shapes (8 gathers for a sample inside the plane; the count includes those that fall outside).
Prints one JSON line and writes it to --out."""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

APIX, TWIST, RISE, RADIUS, SIGMA = 2.0, 29.0, 6.0, 40.0, 4.0


def helix_map(n, seed=0, noise=0.5):
    """Gaussian balls on a helix (twist 29 degrees, rise 6 Angstrom, two balls per unit), noise 0.5 sigma of the foreground."""
    ax = (np.arange(n) - n // 2) * APIX
    vol = np.zeros((n, n, n))
    imax = int(np.ceil(n * APIX / RISE))
    for i in range(-imax, imax + 1):
        for rho, az, dz in ((1.0, 0.0, 0.0), (0.6, 40.0, 1.5)):
            a = np.deg2rad(TWIST * i + az)
            ez = np.exp(-((ax - (i * RISE + dz)) ** 2) / SIGMA**2)
            ey = np.exp(-((ax - rho * RADIUS * np.sin(a)) ** 2) / SIGMA**2)
            ex = np.exp(-((ax - rho * RADIUS * np.cos(a)) ** 2) / SIGMA**2)
            vol += ez[:, None, None] * ey[None, :, None] * ex[None, None, :]
    vol = vol.astype(np.float32)
    sd = noise * np.std(vol[vol > 1e-3])
    return (vol + np.random.default_rng(seed).normal(scale=sd, size=vol.shape)).astype(np.float32)


def samples_tested(shape, z_range, k_range, plane_voxels, params):
    """(voxel, repeat, copy) samples the scoring kernel tests per candidate: for every scored plane the repeats whose
    source plane lies in [z0, z1) (the reference's expression), times the in-plane voxels of the region, times csym."""
    nz = shape[0]
    k = np.arange(k_range[0], k_range[1], dtype=np.float64)[:, None]
    out = []
    for tw, rs, cs in params:
        hmax = max(1, int(nz * APIX / rs))
        hi = np.arange(-hmax, hmax + 1, dtype=np.float64)[None, :]
        k2 = ((k - nz // 2) * APIX + hi * rs) / APIX + nz // 2
        out.append(int(((k2 >= z_range[0]) & (k2 < z_range[1])).sum()) * plane_voxels * int(cs))
    return np.asarray(out, dtype=np.float64)


def median_time(fn, repeats):
    fn()   # warm-up
    t = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()   # synchronous: returns with the result on the host
        t.append(time.perf_counter() - t0)
    return float(np.median(t))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--n", type=int, default=128)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--calls", type=int, default=0, help="only this many searches of the grid (the profiled run)")
    ap.add_argument("--out", default=str(Path(__file__).resolve().parent.parent / "profiles" / "symmetry_search.json"))
    args = ap.parse_args(argv)
    if args.repeats < 5 and not args.calls:
        ap.error("--repeats must be at least 5")

    import helicon_amd as H
    from helicon_amd.symmetry_search import SymmetrySearch, region_spec

    n = args.n
    vol = helix_map(n)
    twists, rises = 20.0 + 0.5 * np.arange(60), 3.0 + 0.1 * np.arange(50)
    grid = H.build_grid(twists, rises, (1,), tube_length=n * APIX)
    assert grid.valid.all()
    params = np.ascontiguousarray(grid.params[:, :3])
    sub = params[np.linspace(0, len(params) - 1, 64).round().astype(int)]   # 64 candidates spread over the grid
    out = dict(map=[n, n, n], apix=APIX, truth=[TWIST, RISE, 1], grid=dict(twists=len(twists), rises=len(rises), csyms=1),
               candidates=len(params), repeats=args.repeats)

    with SymmetrySearch(vol, APIX, device=args.device) as ss:
        if args.calls:
            for _ in range(args.calls):
                ss.search(params)
            print(json.dumps(out))
            return
        # ---- end to end, default region
        spec = ss.region
        out["default_region"] = dict(rmax=spec["rmax"], z_fraction=spec["z_fraction"], voxels=spec["region_voxels"])
        scores = ss.search(params)
        best = int(np.argmax(scores))
        out["best"] = [float(v) for v in params[best]] + [float(scores[best])]
        t = median_time(lambda: ss.search(params), args.repeats)
        out["search_s"] = t
        out["search_candidates_per_s"] = len(params) / t
        out["search_kernel_ms_per_candidate"] = ss.kernel_ms / len(params)
        smp = samples_tested(vol.shape, ss.z_range, spec["k_range"], spec["plane_voxels"], params).sum()
        out["search_samples_per_s"] = smp / (ss.kernel_ms * 1e-3)
        out["search_gathers_per_s"] = 8 * smp / (ss.kernel_ms * 1e-3)
        t64 = median_time(lambda: ss.search(sub), args.repeats)
        got64 = ss.search(sub)

        # ---- the per-candidate loop on the same 64 candidates
        k0, k1 = spec["k_range"]
        jj, ii = np.meshgrid(np.arange(n) - n // 2, np.arange(n) - n // 2, indexing="ij")
        mask = np.zeros(vol.shape, bool)
        mask[k0:k1] = (jj * jj + ii * ii < spec["rmax"] ** 2)[None]
        vm = vol[mask]

        def loop():
            return np.array([H.cross_correlation_coefficient(vm, H.apply_helical_symmetry(vol, APIX, tw, rs, int(cs), device=args.device)[mask],
                                                             device=args.device) for tw, rs, cs in sub])

        ref64 = loop()
        tl = median_time(loop, args.repeats)
        out["loop_64_s"], out["search_64_s"] = tl, t64
        out["loop_candidates_per_s"] = 64 / tl
        out["search_64_candidates_per_s"] = 64 / t64
        out["end_to_end_ratio_grid"] = out["search_candidates_per_s"] / out["loop_candidates_per_s"]
        out["end_to_end_ratio_same_64"] = tl / t64
        out["max_score_difference_search_vs_loop"] = float(np.abs(got64 - ref64).max())

        # ---- like for like: the whole volume scored, kernel against kernel, candidate by candidate
        whole = ss.set_region(0, None, 1.0)
        ss.search(sub)                                                        # warm-up of this shape
        H.apply_helical_symmetry(vol, APIX, *sub[0][:2], 1, device=args.device)   # ... and of the operator
        ms_search, ms_apply = [], []
        for tw, rs, cs in sub:
            one = np.array([[tw, rs, cs]])
            a, b = [], []
            for _ in range(args.repeats):   # alternating, back to back
                ss.search(one)
                a.append(ss.kernel_ms)
                b.append(H.apply_helical_symmetry(vol, APIX, tw, rs, int(cs), device=args.device, return_kernel_ms=True)[1])
            ms_search.append(float(np.median(a)))
            ms_apply.append(float(np.median(b)))
        ms_search, ms_apply = np.array(ms_search), np.array(ms_apply)
        ss.search(sub)
        batch_ms = ss.kernel_ms / len(sub)
        smp = samples_tested(vol.shape, ss.z_range, whole["k_range"], whole["plane_voxels"], sub)
        out["like_for_like"] = dict(
            region_voxels=whole["region_voxels"],
            search_kernel_ms_median=float(np.median(ms_search)), apply_kernel_ms_median=float(np.median(ms_apply)),
            ratio_apply_over_search_median=float(np.median(ms_apply / ms_search)),
            ratio_apply_over_search_min=float((ms_apply / ms_search).min()),
            candidates_where_search_is_slower=int((ms_search > ms_apply).sum()),
            search_kernel_ms_per_candidate_in_a_batch_of_64=batch_ms,
            search_samples_per_s=float(np.median(smp / (ms_search * 1e-3))),
            search_gathers_per_s=float(np.median(8 * smp / (ms_search * 1e-3))),
            apply_gathers_per_s=float(np.median(8 * smp / (ms_apply * 1e-3))),
        )
    line = json.dumps(out)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
