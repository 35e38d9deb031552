#!/usr/bin/env python3
"""Times of the phase-randomised true FSC on the device (helicon_amd/true_fsc.py, csrc/true_fsc.inc).

    python tools/true_fsc_bench.py [--out profiles/true_fsc.json] [--sizes 64 128 256] [--repeats 5] [--accuracy LOG]
                                   [--soft-out profiles/soft_mask.json] [--soft-only]
                                   [--adaptive-out profiles/adaptive_mask.json] [--adaptive-only]

Per size, one pair of n^3 maps (a blob plus noise, so that the adaptive mask has something to find), after a warm-up of every
call that is timed; medians of REPEATS:

* ``create``: ``TrueFSC(map1, map2, apix, cutoff, seed=1)`` — upload of two maps, forward passes, substitution, inverse
  passes; wall (host clock; the call ends in a device synchronise) only;
* ``masked``: one ``.masked(mask, per_shell=True)`` on the resident context — wall, and ``kernel_ms`` from device events;
* ``masked_batch_8``: one ``.masked_batch`` of 8 masks — the same two numbers, also per mask;
* ``parent_one_mask``: what the parent commit offers for one mask: four host multiplies and two ``calc_fsc_per_shell`` calls
  (the randomised maps taken from the context beforehand, outside the timing) — wall;
* ``host_composition``: ``scipy.fft.rfftn`` / ``irfftn`` / ``fftn(workers=16)`` + ``bincount`` for the whole method with one
  mask on the host — wall;
* ``refine``: a whole ``true_fsc(one_mask=True, refine_mask=True, seed=1)`` run — wall, the seconds of it spent in the host's
  mask helpers (``host_mask_s``), the number of ``.masked`` evaluations, one run.

With ``--soft-out`` (``--soft-only``: nothing else) the soft masks built on the device (csrc/soft_mask.inc), per size:

* ``refine``: a whole ``true_fsc(one_mask=True, refine_mask=True, seed=1)`` run with ``device_masks=True`` and without: wall,
  ``host_mask_s``, the share of the wall that is not the host's mask helpers, the widths the refinement visited;
* ``trials``: at every width the device run visited, alternating in one loop, ``soft_masked(w, per_shell=True)`` beside the
  parent's trial, ``soft_mask(support, w)`` on the host + ``.masked(trial, per_shell=True)`` — wall, and the device's
  ``kernel_ms``; every width is listed, none is folded into a median over widths;
* ``kernels``: per visited step, device-event times of the three transform passes (``distance_transform_edt_sq``) and of
  transform + mask kernel (``soft_mask_device``); their difference is the mask kernel.

ITS GATE: at 128^3 and 256^3 the device trial's wall must not exceed the parent trial's at ANY visited width.

With ``--adaptive-out`` (``--adaptive-only``: nothing else) the adaptive mask built on the device (csrc/adaptive_mask.inc),
per size, on the average of the two maps:

* ``calls``: alternating in one loop after a warm-up, the host's ``adaptive_mask``, the standalone ``adaptive_mask_device``
  (upload of the float64 volume included) and the resident context's ``adaptive_support(one_mask=True)`` (download of the
  support included) — wall, medians; whether the three masks are equal;
* ``stages``: device-event times of the context's call per stage (``adaptive_stage_ms``): the three Gaussian passes, the
  statistics (minimum, maximum, histogram, selection), runs, unions, flatten, pick — medians;
* ``refine``: a whole ``true_fsc(one_mask=True, refine_mask=True, seed=1)`` run three ways — host masks, ``device_masks``,
  ``device_masks`` + ``device_support`` — each with its wall and ``host_mask_s``.

ITS GATE: at 128^3 and 256^3 the context's call must take less wall time than the host's ``adaptive_mask`` of the same run.

THE GATE: at 128^3 and 256^3 ``masked.wall_ms`` must not exceed ``parent_one_mask.wall_ms`` of the same run (same kernels,
one mask uploaded instead of four maps): both are printed, and the tool exits 1 if it is missed.  With ``--accuracy LOG`` the
TFSC_FIGURE lines of a ``pytest tests/test_gpu_true_fsc.py -s`` log are parsed into the ``accuracy`` section.  A run without
a GPU fails: there is nothing to time.
"""
import argparse
import importlib
import json
import re
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))


def median_wall(fn, repeats):
    walls = []
    for _ in range(repeats):
        t = time.perf_counter()
        fn()
        walls.append((time.perf_counter() - t) * 1e3)
    return float(np.median(walls))


def parse_figures(path):
    out = {}
    keys = ("n", "map", "per_shell")
    for line in Path(path).read_text().splitlines():
        m = re.search(r"TFSC_FIGURE (.*)$", line)
        if not m:
            continue
        words = m.group(1).split()
        name = " ".join(w for w in words if "=" not in w or w.split("=")[0] in keys)
        out[name] = {w.split("=")[0]: w.split("=", 1)[1] for w in words if "=" in w and w.split("=")[0] not in keys}
    return out


def host_composition(a, b, mask, m_sel, shell_full, angles):
    """The whole method with one mask on the host: 2 rfftn, substitution, 2 irfftn, 4 multiplies, 4 fftn, 2 x 3 bincounts."""
    from scipy.fft import fftn, irfftn, rfftn

    out = []
    maps = []
    for x, th in zip((a, b), angles):
        F = rfftn(x, workers=16)
        F[m_sel] = np.abs(F[m_sel]) * np.exp(1j * th[m_sel])
        maps.append(irfftn(F, workers=16))
    nb = a.shape[0] // 2 + 1
    s = shell_full.ravel()
    for p, q in ((a, b), maps):
        f1, f2 = fftn(p * mask, workers=16), fftn(q * mask, workers=16)
        out.append(np.stack([np.bincount(s, weights=np.real(f1 * np.conj(f2)).ravel(), minlength=nb),
                             np.bincount(s, weights=(np.abs(f1) ** 2).ravel(), minlength=nb),
                             np.bincount(s, weights=(np.abs(f2) ** 2).ravel(), minlength=nb)], axis=1))
    return out


def soft_mask_legs(n, a, b, apix, cutoff, repeats):
    """The legs of the device soft masks for one size; (case, gate passed)."""
    import helicon_amd as H

    T = importlib.import_module("helicon_amd.true_fsc")
    case = {"case": f"1 x {n}^3", "n": n}
    visited = []

    class Recording(H.TrueFSC):
        def soft_masked(self, width, per_shell=False):
            if per_shell:
                visited.append(float(width))
            return super().soft_masked(width, per_shell)

    T.true_fsc(a, b, apix, cutoff_res=cutoff, one_mask=True, mask_soft=3 * apix, seed=1, device_masks=True)      # warm-up
    runs = {}
    for name, flag, ctx in (("device_masks", True, Recording), ("host_masks", False, H.TrueFSC)):
        t0 = time.perf_counter()
        out = T.true_fsc(a, b, apix, cutoff_res=cutoff, one_mask=True, refine_mask=True, seed=1, device_masks=flag, context=ctx)
        wall = time.perf_counter() - t0
        runs[name] = {"wall_s": wall, "host_mask_s": out["host_mask_s"], "rest_s": wall - out["host_mask_s"],
                      "share_outside_host_masks": (wall - out["host_mask_s"]) / wall, "mask_soft_px": out["mask_soft_px"],
                      "resolution_true": out["resolution"]["true"]}
    runs["speedup"] = runs["host_masks"]["wall_s"] / runs["device_masks"]["wall_s"]
    runs["widths_visited"] = list(visited)
    case["refine"] = runs
    support = T.adaptive_mask((a.astype(np.float64) + b) / 2, apix, cutoff)
    trials, ok = [], True
    with H.TrueFSC(a, b, apix, cutoff, seed=1) as ctx:
        ctx.set_support(support)
        for w in visited:
            ctx.soft_masked(w, per_shell=True)
            ctx.masked(T.soft_mask(support, w), per_shell=True)
            w_dev, k_dev, w_par, w_host = [], [], [], []
            for _ in range(repeats):
                t0 = time.perf_counter()
                ctx.soft_masked(w, per_shell=True)
                w_dev.append((time.perf_counter() - t0) * 1e3)
                k_dev.append(ctx.kernel_ms)
                t0 = time.perf_counter()
                trial = T.soft_mask(support, w)
                t1 = time.perf_counter()
                ctx.masked(trial, per_shell=True)
                w_par.append((time.perf_counter() - t0) * 1e3)
                w_host.append((t1 - t0) * 1e3)
            row = {"width": w, "step": T.soft_step(w), "device_wall_ms": float(np.median(w_dev)), "device_kernel_ms": float(np.median(k_dev)),
                   "parent_wall_ms": float(np.median(w_par)), "parent_host_soft_mask_ms": float(np.median(w_host))}
            row["ratio"] = row["parent_wall_ms"] / row["device_wall_ms"]
            ok = ok and row["device_wall_ms"] <= row["parent_wall_ms"]
            trials.append(row)
    case["trials"] = trials
    kernels = []
    for step in sorted({T.soft_step(w) for w in visited}):
        w = max(v for v in visited if T.soft_step(v) == step)
        T.distance_transform_edt_sq(support, step)
        T.soft_mask_device(support, w)
        edt, both = [], []
        for _ in range(repeats):
            T.distance_transform_edt_sq(support, step)
            edt.append(T.distance_transform_edt_sq.kernel_ms)
            T.soft_mask_device(support, w)
            both.append(T.soft_mask_device.kernel_ms)
        kernels.append({"step": step, "width": w, "decimated_side": -(-n // step), "transform_ms": float(np.median(edt)),
                        "transform_and_mask_ms": float(np.median(both)), "mask_kernel_ms": float(np.median(both) - np.median(edt))})
    case["kernels"] = kernels
    return case, ok


def adaptive_mask_legs(n, a, b, apix, cutoff, repeats):
    """The legs of the device adaptive mask for one size; (case, gate passed)."""
    import helicon_amd as H

    T = importlib.import_module("helicon_amd.true_fsc")
    case = {"case": f"1 x {n}^3", "n": n, "sigma": cutoff / (3.81 * apix) if cutoff > 2 * apix else 0.0}
    avg = (a.astype(np.float64) + b) / 2
    with H.TrueFSC(a, b, apix, cutoff, seed=1) as ctx:
        host = T.adaptive_mask(avg, apix, cutoff)                 # warm-up of all three
        alone = T.adaptive_mask_device(avg, apix, cutoff)
        info = ctx.adaptive_support(one_mask=True)
        case["info"] = info[0]
        case["masks_equal"] = bool(np.array_equal(alone, host != 0) and np.array_equal(ctx.support(0), host != 0))
        w_host, w_alone, w_ctx, stages = [], [], [], []
        for _ in range(repeats):
            t0 = time.perf_counter()
            T.adaptive_mask(avg, apix, cutoff)
            w_host.append((time.perf_counter() - t0) * 1e3)
            t0 = time.perf_counter()
            T.adaptive_mask_device(avg, apix, cutoff)
            w_alone.append((time.perf_counter() - t0) * 1e3)
            T.adaptive_stage_ms(reset=True)
            t0 = time.perf_counter()
            ctx.adaptive_support(one_mask=True)
            w_ctx.append((time.perf_counter() - t0) * 1e3)
            stages.append(T.adaptive_stage_ms(reset=True))
    case["calls"] = {"host_wall_ms": float(np.median(w_host)), "standalone_wall_ms": float(np.median(w_alone)), "context_wall_ms": float(np.median(w_ctx))}
    case["calls"]["host_over_context"] = case["calls"]["host_wall_ms"] / case["calls"]["context_wall_ms"]
    case["stages_ms"] = {k: float(np.median([s[k] for s in stages])) for k in stages[0]}
    runs = {}
    for name, kw in (("host_masks", dict()), ("device_masks", dict(device_masks=True)), ("device_masks_and_support", dict(device_masks=True, device_support=True))):
        t0 = time.perf_counter()
        out = T.true_fsc(a, b, apix, cutoff_res=cutoff, one_mask=True, refine_mask=True, seed=1, **kw)
        wall = time.perf_counter() - t0
        runs[name] = {"wall_s": wall, "host_mask_s": out["host_mask_s"], "mask_soft_px": out["mask_soft_px"], "resolution_true": out["resolution"]["true"]}
    case["refine"] = runs
    return case, case["calls"]["context_wall_ms"] < case["calls"]["host_wall_ms"]


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=None)
    ap.add_argument("--sizes", type=int, nargs="*", default=[64, 128, 256])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--accuracy", default=None, help="log of `pytest tests/test_gpu_true_fsc.py -s` to take the measured errors from")
    ap.add_argument("--no-refine", action="store_true", help="leave the whole-run timing out")
    ap.add_argument("--soft-out", default=None, help="also time the soft masks built on the device and write this file")
    ap.add_argument("--soft-only", action="store_true", help="only the soft-mask legs")
    ap.add_argument("--adaptive-out", default=None, help="also time the adaptive mask built on the device and write this file")
    ap.add_argument("--adaptive-only", action="store_true", help="only the adaptive-mask legs")
    args = ap.parse_args(argv)

    import fsc_oracle as O
    import true_fsc_oracle as TO
    import helicon_amd as H

    T = importlib.import_module("helicon_amd.true_fsc")
    apix = 2.0
    result = {"repeats": args.repeats, "cases": [], "gate": {}}
    soft = {"repeats": args.repeats, "cases": [], "gate": {}}
    adaptive = {"repeats": args.repeats, "cases": [], "gate": {}}
    missed = False
    for n in args.sizes:
        a, b = O.make_map_pair(n, 500 + n, dc="auto")
        g = np.arange(n) - n // 2
        blob = 6.0 * np.exp(-(g[:, None, None] ** 2 + g[None, :, None] ** 2 + g[None, None, :] ** 2) / (2.0 * (n / 6.0) ** 2))
        a, b = (a + blob).astype(np.float32), (b + blob).astype(np.float32)
        cutoff = apix * n / (n / 4 + 0.5)
        if args.adaptive_out or args.adaptive_only:
            case, ok = adaptive_mask_legs(n, a, b, apix, cutoff, args.repeats)
            adaptive["cases"].append(case)
            print(json.dumps(case), flush=True)
            if n >= 128:
                adaptive["gate"][str(n)] = {"passed": bool(ok), "host_wall_ms": case["calls"]["host_wall_ms"], "context_wall_ms": case["calls"]["context_wall_ms"]}
                print(f"ADAPTIVE GATE n={n}: the context's call {case['calls']['context_wall_ms']:.3f} ms, the host's adaptive_mask "
                      f"{case['calls']['host_wall_ms']:.3f} ms: {'ok' if ok else 'MISSED'}", flush=True)
                missed = missed or not ok
            if args.adaptive_only:
                continue
        if args.soft_out or args.soft_only:
            case, ok = soft_mask_legs(n, a, b, apix, cutoff, args.repeats)
            soft["cases"].append(case)
            print(json.dumps(case), flush=True)
            if n >= 128:
                worst = min(case["trials"], key=lambda r: r["ratio"])
                soft["gate"][str(n)] = {"passed": bool(ok), "slowest_ratio": worst["ratio"], "at_width": worst["width"]}
                print(f"SOFT GATE n={n}: device trial no slower than the parent's at every visited width: {'ok' if ok else 'MISSED'} "
                      f"(smallest parent / device = {worst['ratio']:.2f} at w = {worst['width']:.2f})", flush=True)
                missed = missed or not ok
            if args.soft_only:
                continue
        masks = np.stack([TO.sphere_mask(n, (0.2 + 0.02 * j) * n, 4.0) for j in range(8)]).astype(np.float32)
        mask = masks[5]
        case = {"case": f"1 x {n}^3", "n": n}

        def create():
            H.TrueFSC(a, b, apix, cutoff, seed=1).close()

        create()
        case["create"] = {"wall_ms": median_wall(create, args.repeats)}
        with H.TrueFSC(a, b, apix, cutoff, seed=1) as ctx:
            ar, br = ctx.randomized_map(0), ctx.randomized_map(1)

            def parent():
                t = H.calc_fsc_per_shell(a * mask, b * mask, apix)
                nz = H.calc_fsc_per_shell(ar * mask, br * mask, apix)
                return t, nz

            # alternate the two sides of the gate: other work shares the host
            ctx.masked(mask, per_shell=True)
            parent()
            w_dev, w_par, k_dev = [], [], []
            for _ in range(args.repeats):
                t0 = time.perf_counter()
                got = ctx.masked(mask, per_shell=True)
                w_dev.append((time.perf_counter() - t0) * 1e3)
                k_dev.append(ctx.kernel_ms)
                t0 = time.perf_counter()
                want = parent()
                w_par.append((time.perf_counter() - t0) * 1e3)
            case["masked"] = {"wall_ms": float(np.median(w_dev)), "kernel_ms": float(np.median(k_dev))}
            case["parent_one_mask"] = {"wall_ms": float(np.median(w_par))}
            case["masked_equals_parent_bitwise"] = bool(np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]))
            ctx.masked_batch(masks, per_shell=True)
            k8 = []

            def batch8():
                ctx.masked_batch(masks, per_shell=True)
                k8.append(ctx.kernel_ms)

            w8 = median_wall(batch8, args.repeats)
            case["masked_batch_8"] = {"wall_ms": w8, "kernel_ms": float(np.median(k8)), "wall_ms_per_mask": w8 / 8,
                                      "kernel_ms_per_mask": float(np.median(k8)) / 8}
        m_sel = TO.m_half(n) >= T.cutoff_m(n, apix, cutoff)
        shell_full = O.shell_3d_full(n)
        rng = np.random.RandomState(1)
        angles = [rng.uniform(0, 2 * np.pi, size=m_sel.shape) for _ in range(2)]
        host_composition(a, b, mask, m_sel, shell_full, angles)
        case["host_composition"] = {"wall_ms": median_wall(lambda: host_composition(a, b, mask, m_sel, shell_full, angles), max(1, args.repeats // 2))}
        if not args.no_refine:
            calls = [0]

            class Counting(H.TrueFSC):
                def masked(self, *p, **k):
                    calls[0] += 1
                    return super().masked(*p, **k)

            t0 = time.perf_counter()
            out = T.true_fsc(a, b, apix, cutoff_res=cutoff, one_mask=True, refine_mask=True, seed=1, context=Counting)
            wall = time.perf_counter() - t0
            case["refine"] = {"wall_s": wall, "host_mask_s": out["host_mask_s"], "device_and_rest_s": wall - out["host_mask_s"],
                              "masked_calls": calls[0], "mask_soft_px": out["mask_soft_px"], "resolution": out["resolution"]}
        if n >= 128:
            ok = case["masked"]["wall_ms"] <= case["parent_one_mask"]["wall_ms"]
            result["gate"][str(n)] = {"masked_wall_ms": case["masked"]["wall_ms"], "parent_wall_ms": case["parent_one_mask"]["wall_ms"],
                                      "passed": bool(ok)}
            print(f"GATE n={n}: masked {case['masked']['wall_ms']:.3f} ms, parent {case['parent_one_mask']['wall_ms']:.3f} ms: "
                  f"{'ok' if ok else 'MISSED'}", flush=True)
            missed = missed or not ok
        result["cases"].append(case)
        print(json.dumps(case), flush=True)
    if args.accuracy:
        result["accuracy"] = parse_figures(args.accuracy)
    if args.adaptive_out:
        Path(args.adaptive_out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.adaptive_out).write_text(json.dumps(adaptive, indent=1) + "\n")
    if args.soft_out:
        Path(args.soft_out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.soft_out).write_text(json.dumps(soft, indent=1) + "\n")
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(result, indent=1) + "\n")
    return 1 if missed else 0


if __name__ == "__main__":
    raise SystemExit(main())
