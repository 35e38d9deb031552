"""Fourier shell correlation of two maps and Fourier ring correlation of two images, on the device.

The reference's four functions (lib/analysis.py:116-484), with their names, positional order, return shapes and quirks:

``calc_fsc(map1, map2, apix)``
    cubic maps; the three shell sums run over the ``rfftn`` HALF spectrum with every bin counted once (no Hermitian
    weight), ``shell = clip(round(sqrt(kz^2 + ky^2 + kx^2)), 0, n // 2)``, ``fsc = num / sqrt(den1 den2)`` where that is
    positive and 1.0 elsewhere; rows ``[saxis, fsc]`` of the shells with ``saxis = i / (apix n) <= rfftfreq(n).max()`` (a
    frequency in 1/Angstrom against one in cycles per pixel: with ``apix < 1`` rows are cut, as in the reference).
``calc_fsc_per_shell(map1, map2, apix)``
    the same sums over the FULL spectrum, as a 1-D array of length ``n // 2 + 1``.
``calc_frc_2d(img1, img2, apix)``
    any ``(h, w)``, full ``fft2``, ``n_shells = min(h, w) // 2``, ``shell = clip(round(kr * n_shells), 0, n_shells)`` with
    ``kr`` in cycles per pixel (the factor is ``n_shells``, not the side: the upper shells hold no bin and are exactly 1.0);
    returns ``(saxis, fsc)``.
``frc_score(img1, img2, apix, use_fit=False)``
    the mean of the curve's values in [-1, 1]; ``use_fit=True`` fits the reference's Fermi / Butterworth curves to the
    device's curve on the host (SciPy's Nelder-Mead) and returns the normalised area under the better one.

Precision: like the reference on float32 maps, the transforms are float32 and the shell sums float64 (``hh_fsc_3d`` /
``hh_frc_2d``, csrc/fourier_correlation.inc); float64 input is converted to float32.  Results are float64 arrays.  The sums
are bit-identical from run to run and do not depend on the batch a pair is part of.  Sides: cubes 8 ... 512, images
8 ... 1024.

Added here: ``calc_fsc_batch`` (stacks of pairs in one call), ``fsc_resolution`` (the threshold rule of
commands/trueFSC.py:427-462) and ``half_map_fsc`` / ``half_map_fsc_batch`` (the FSC of the two half reconstructions of
``lsq_reconstruct(..., fsc_test=...)`` after ``apply_helical_symmetry`` onto a cube).

    python -m helicon_amd.fsc half1.mrc half2.mrc [--apix A] [--per-shell] [--threshold 0.143 0.5] [--out curve.txt] [--device 0]

reads two maps (``.mrc`` / ``.map`` / ``.npy``; the header's voxel size unless ``--apix``), prints a JSON report (the curve
and the resolution at every threshold) and, with ``--out``, writes ``saxis fsc`` rows.
"""
from __future__ import annotations

import argparse
import ctypes as C
import functools
import json
import sys

import numpy as np

from . import _lib

__all__ = ["calc_fsc", "calc_fsc_per_shell", "calc_fsc_batch", "calc_frc_2d", "frc_score", "fsc_resolution", "half_map_fsc",
           "half_map_fsc_batch", "fsc_sums_3d", "frc_sums_2d", "frc_shell_table", "shell_index_3d", "main"]

_MIN_SIDE, _MAX_SIDE_3D, _MAX_SIDE_2D = 8, 512, 1024


# ------------------------------------------------------------------------------------------
# shells
# ------------------------------------------------------------------------------------------
def shell_index_3d(m):
    """``round(sqrt(m))`` of integers ``m >= 0`` in integer arithmetic: ``k`` with ``k (k - 1) < m <= k (k + 1)`` (and 0 for
    ``m = 0``).  ``sqrt(m)`` is never ``k + 1/2``, so there are no ties; this is the rule the kernel applies to
    ``m = kz^2 + ky^2 + kx^2`` before clipping to ``n // 2``."""
    m = np.asarray(m, dtype=np.int64)
    k = np.floor(np.sqrt(m.astype(np.float64))).astype(np.int64)
    k += (k * (k + 1) < m)
    k -= (k > 0) & (k * (k - 1) >= m)
    return k


@functools.lru_cache(maxsize=16)
def _frc_shell_table(h: int, w: int):
    n_shells = min(h, w) // 2
    kx = np.fft.fftfreq(w) ** 2
    ky = np.fft.fftfreq(h) ** 2
    kr = np.sqrt(ky[:, None] + kx[None, :])
    shell = np.round(kr * n_shells).astype(np.int32)   # ties are real here: NumPy's float64 value decides, half to even
    np.clip(shell, 0, n_shells, out=shell)
    shell = np.ascontiguousarray(shell)
    shell.setflags(write=False)
    return shell


def frc_shell_table(h, w):
    """The ring of every bin of the full ``(h, w)`` spectrum: the reference's NumPy expression (analysis.py:331-335), built
    on the host, cached per shape (read-only int32) and uploaded with every call."""
    return _frc_shell_table(int(h), int(w))


# ------------------------------------------------------------------------------------------
# the library calls
# ------------------------------------------------------------------------------------------
def _f32(a, name):
    a = np.asarray(a)
    if a.dtype.kind not in "biuf":
        raise ValueError(f"{name}: the data must be real; got dtype {a.dtype}")
    a = np.ascontiguousarray(a, dtype=np.float32)
    if not np.isfinite(a).all():
        raise ValueError(f"{name}: the data holds NaN or infinite values")
    return a


def fsc_sums_3d(maps1, maps2, full_spectrum=False, *, device=0, return_kernel_ms=False):
    """``[B, n // 2 + 1, 3]`` float64: ``num, den1, den2`` of every shell for ``B`` pairs of ``n x n x n`` maps (``[B, n, n,
    n]`` stacks, or one pair ``[n, n, n]`` -> ``[n // 2 + 1, 3]``).  ``full_spectrum``: the sums of ``calc_fsc_per_shell``
    instead of ``calc_fsc``'s."""
    a, b = np.asarray(maps1), np.asarray(maps2)
    single = a.ndim == 3
    if a.shape != b.shape:
        raise ValueError(f"fsc_sums_3d: the two maps must have one shape; got {a.shape} and {b.shape}")
    if a.ndim not in (3, 4) or len(set(a.shape[-3:])) != 1:
        raise ValueError(f"fsc_sums_3d: cubic maps only (n x n x n, or stacks [B, n, n, n]); got {a.shape}")
    batch, n = (1 if single else a.shape[0]), a.shape[-1]
    if batch < 1 or n < _MIN_SIDE or n > _MAX_SIDE_3D:
        raise ValueError(f"fsc_sums_3d: the side must lie in [{_MIN_SIDE}, {_MAX_SIDE_3D}] and the batch be >= 1; got {a.shape}")
    a, b = _f32(a, "fsc_sums_3d"), _f32(b, "fsc_sums_3d")
    sums = np.empty((batch, n // 2 + 1, 3), dtype=np.float64)
    ms = C.c_double(0.0)
    f32p, f64p = C.POINTER(C.c_float), C.POINTER(C.c_double)
    _lib.check(_lib.lib().hh_fsc_3d(int(device), a.ctypes.data_as(f32p), b.ctypes.data_as(f32p), batch, n, 1 if full_spectrum else 0,
                                    sums.ctypes.data_as(f64p), C.byref(ms)), None)
    out = sums[0] if single else sums
    return (out, ms.value) if return_kernel_ms else out


def frc_sums_2d(imgs1, imgs2, *, device=0, return_kernel_ms=False):
    """``[B, n_shells + 1, 3]`` float64 ring sums of ``B`` image pairs ``[B, h, w]`` (or one pair ``[h, w]``)."""
    a, b = np.asarray(imgs1), np.asarray(imgs2)
    if a.shape != b.shape:
        raise ValueError(f"Image shapes must match: {a.shape} vs {b.shape}")
    single = a.ndim == 2
    if a.ndim not in (2, 3):
        raise ValueError(f"frc_sums_2d: images [h, w] or stacks [B, h, w]; got {a.shape}")
    batch, (h, w) = (1 if single else a.shape[0]), a.shape[-2:]
    if batch < 1 or min(h, w) < _MIN_SIDE or max(h, w) > _MAX_SIDE_2D:
        raise ValueError(f"frc_sums_2d: both sides must lie in [{_MIN_SIDE}, {_MAX_SIDE_2D}] and the batch be >= 1; got {a.shape}")
    a, b = _f32(a, "frc_sums_2d"), _f32(b, "frc_sums_2d")
    table = frc_shell_table(h, w)
    n_shells = min(h, w) // 2
    sums = np.empty((batch, n_shells + 1, 3), dtype=np.float64)
    ms = C.c_double(0.0)
    f32p, f64p = C.POINTER(C.c_float), C.POINTER(C.c_double)
    _lib.check(_lib.lib().hh_frc_2d(int(device), a.ctypes.data_as(f32p), b.ctypes.data_as(f32p), batch, h, w,
                                    table.ctypes.data_as(C.POINTER(C.c_int32)), n_shells, sums.ctypes.data_as(f64p), C.byref(ms)), None)
    out = sums[0] if single else sums
    return (out, ms.value) if return_kernel_ms else out


def _ratio(sums):
    """``num / sqrt(den1 den2)`` where the denominator is positive, 1.0 elsewhere (analysis.py:174-177)."""
    sums = np.asarray(sums, dtype=np.float64)
    denom = np.sqrt(sums[..., 1] * sums[..., 2])
    fsc = np.ones(denom.shape, dtype=np.float64)
    ok = denom > 0
    fsc[ok] = sums[..., 0][ok] / denom[ok]
    return fsc


def _fsc_rows(fsc, n, apix):
    saxis = np.arange(n // 2 + 1) * (1.0 / (apix * n))
    keep = np.where(saxis <= np.fft.rfftfreq(n).max())   # 1/Angstrom against cycles per pixel, as the reference compares them
    return np.vstack((saxis[keep], fsc[keep])).T


# ------------------------------------------------------------------------------------------
# the reference's functions
# ------------------------------------------------------------------------------------------
def _cube_pair(map1, map2, name):
    a, b = np.asarray(map1), np.asarray(map2)
    if a.ndim != 3 or len(set(a.shape)) != 1 or a.shape != b.shape:
        raise ValueError(f"{name}: two cubic maps of one shape (n x n x n) are needed; got {a.shape} and {b.shape}")
    return a, b


def calc_fsc(map1, map2, apix, F1=None, F2=None, shell_flat=None, n=None, *, device=0):
    """analysis.py:116-182 on the device: a two-column array ``[saxis (1/Angstrom), fsc]``.  Cubic maps of side 8 ... 512;
    float64 input is converted to float32 (the reference's own transform of a float32 map is single precision too).
    Precomputed spectra (``F1``, ``F2``, ``shell_flat``) are outside the accelerated path: ``NotImplementedError``."""
    if F1 is not None or F2 is not None or shell_flat is not None:
        raise NotImplementedError("calc_fsc: precomputed spectra (F1, F2, shell_flat) are not accepted: pass the maps")
    a, b = _cube_pair(map1, map2, "calc_fsc")
    if n is not None and int(n) != a.shape[0]:
        raise ValueError(f"calc_fsc: n = {n} is not the maps' side {a.shape[0]}")
    return _fsc_rows(_ratio(fsc_sums_3d(a, b, False, device=device)), a.shape[0], apix)


def calc_fsc_per_shell(map1, map2, apix, *, device=0):
    """analysis.py:235-290 on the device: the FSC over the full spectrum, indexed by shell (``n // 2 + 1`` values; the
    frequency of shell ``i`` is ``i / (n apix)``).  Cubic maps of side 8 ... 512, computed in float32."""
    a, b = _cube_pair(map1, map2, "calc_fsc_per_shell")
    return _ratio(fsc_sums_3d(a, b, True, device=device))


def calc_fsc_batch(maps1, maps2, apix, per_shell=False, *, device=0):
    """The curves of ``B`` pairs ``[B, n, n, n]`` in one call: ``[B, rows, 2]`` (``calc_fsc``) or ``[B, n // 2 + 1]``
    (``per_shell``).  Every curve is bit for bit the one the single call gives."""
    a, b = np.asarray(maps1), np.asarray(maps2)
    if a.ndim != 4 or a.shape != b.shape:
        raise ValueError(f"calc_fsc_batch: two stacks [B, n, n, n] of one shape are needed; got {a.shape} and {b.shape}")
    fsc = _ratio(fsc_sums_3d(a, b, bool(per_shell), device=device))
    if per_shell:
        return fsc
    return np.stack([_fsc_rows(f, a.shape[1], apix) for f in fsc])


def calc_frc_2d(img1, img2, apix, *, device=0):
    """analysis.py:293-356 on the device: ``(saxis, fsc)``, both of length ``min(h, w) // 2 + 1``.  Sides 8 ... 1024,
    computed in float32."""
    a, b = np.asarray(img1), np.asarray(img2)
    if a.shape != b.shape:
        raise ValueError(f"Image shapes must match: {a.shape} vs {b.shape}")
    if a.ndim != 2:
        raise ValueError(f"calc_frc_2d: 2-D images are needed; got {a.shape}")
    h, w = a.shape
    fsc = _ratio(frc_sums_2d(a, b, device=device))
    return np.arange(min(h, w) // 2 + 1) / (min(h, w) * apix), fsc


def _fit_frc_curve(saxis, fsc):
    """analysis.py:359-439 on the host: a Fermi and a Butterworth curve fitted (mean absolute deviation, Nelder-Mead) to the
    points with -0.1 <= fsc <= 1.1; the better one on 500 frequencies from ``saxis[1]`` to ``saxis[-1]``, clipped to
    [-1, 1].  Fewer than three usable points: the curve itself."""
    from scipy.optimize import minimize

    use = np.isfinite(fsc) & (fsc >= -0.1) & (fsc <= 1.1)
    s, f = saxis[use], fsc[use]
    if len(s) < 3:
        return saxis, fsc

    def fermi(mu, t, x):
        return 1.0 / (np.exp((x - mu) / t) + 1.0)

    def butterworth(omega, order, x):
        return 1.0 / (1.0 + (x / omega) ** order)

    def fermi_cost(p):
        if p[1] <= 0:
            return 1e10
        return np.mean(np.abs(f - 1.0 / fermi(p[0], p[1], 0.0) * fermi(p[0], p[1], s)))

    def butterworth_cost(p):
        if p[0] <= 0 or p[1] <= 0:
            return 1e10
        return np.mean(np.abs(f - butterworth(p[0], p[1], s)))

    fine = np.linspace(saxis[1], saxis[-1], 500)
    options = {"maxiter": 1000, "xatol": 1e-6}
    best, out = np.inf, (s.copy(), f.copy())
    fit = minimize(fermi_cost, x0=[s[len(s) // 2], 0.01], method="Nelder-Mead", options=options)
    if fit.fun < best:
        best = fit.fun
        out = (fine, np.clip(1.0 / fermi(fit.x[0], fit.x[1], 0.0) * fermi(fit.x[0], fit.x[1], fine), -1, 1))
    fit = minimize(butterworth_cost, x0=[s[len(s) // 2], 2.0], method="Nelder-Mead", options=options)
    if fit.fun < best:
        out = (fine, np.clip(butterworth(fit.x[0], fit.x[1], fine), -1, 1))
    return out


def _score_of_curve(saxis, fsc, use_fit):
    if use_fit:
        s, f = _fit_frc_curve(saxis, fsc)
        ok = np.isfinite(f) & (f >= -1) & (f <= 1)
        if not ok.any():
            return 0.0
        s, f = s[ok], f[ok]
        span = s[-1] - s[0]
        if span <= 0:
            return 0.0
        return float(np.sum(np.diff(s) * (f[1:] + f[:-1]) / 2.0) / span)   # the trapezoid rule, in np.trapz's order
    ok = np.isfinite(fsc) & (fsc >= -1) & (fsc <= 1)
    return float(np.mean(fsc[ok])) if ok.any() else 0.0


def frc_score(img1, img2, apix, use_fit=False, *, device=0):
    """analysis.py:442-484: the mean of the ring correlation's values in [-1, 1], or with ``use_fit`` the normalised area
    under the fitted Fermi / Butterworth curve (the fit runs on the host on the device's curve)."""
    saxis, fsc = calc_frc_2d(img1, img2, apix, device=device)
    return _score_of_curve(saxis, fsc, use_fit)


# ------------------------------------------------------------------------------------------
# resolution, half maps
# ------------------------------------------------------------------------------------------
def fsc_resolution(saxis, fsc, threshold=0.143):
    """commands/trueFSC.py:427-462: the resolution (Angstrom) at which the curve first goes below ``threshold``, linearly
    interpolated between that shell and the one before; 999.0 when it never does (or crosses at a frequency <= 0)."""
    f, s = np.asarray(fsc, dtype=np.float64), np.asarray(saxis, dtype=np.float64)
    below = np.flatnonzero(f < threshold)
    if below.size == 0:
        return 999.0
    i = int(below[0])
    if i == 0:
        return float(1.0 / s[0]) if s[0] > 0 else 999.0
    x = s[i] if f[i - 1] == f[i] else s[i - 1] + (threshold - f[i - 1]) * (s[i] - s[i - 1]) / (f[i] - f[i - 1])
    return float(1.0 / x) if x > 0 else 999.0


def _resolutions(curve, n, apix, per_shell):
    if per_shell:
        saxis, f = np.arange(n // 2 + 1) / (n * apix), curve
    else:
        saxis, f = curve[:, 0], curve[:, 1]
    return {"0.5": fsc_resolution(saxis, f, 0.5), "0.143": fsc_resolution(saxis, f, 0.143)}


def half_map_fsc_batch(halves1, halves2, apix3d, symmetries, *, size=None, new_apix=None, fraction=1.0, per_shell=False, device=0,
                       symmetrize=None, fsc_batch=None):
    """``half_map_fsc`` for a list of half-map pairs of one shape: ``symmetries[i] = (twist_degree, rise_angstrom, csym)`` of
    pair ``i``.  Every half is symmetrised on its own, the cubes are stacked and all curves come from ONE ``calc_fsc_batch``
    call.  Returns ``[(curve, resolutions), ...]``.  ``symmetrize`` / ``fsc_batch`` stand in for ``apply_helical_symmetry`` /
    ``calc_fsc_batch`` (tests)."""
    if symmetrize is None:
        from .denovo3D import apply_helical_symmetry as symmetrize
    fsc_batch = fsc_batch or calc_fsc_batch
    if not (len(halves1) == len(halves2) == len(symmetries)) or len(symmetries) == 0:
        raise ValueError("half_map_fsc: one (twist, rise, csym) per pair of halves, and at least one pair")
    new_apix = float(apix3d if new_apix is None else new_apix)
    cubes = ([], [])
    for h1, h2, (twist, rise, csym) in zip(halves1, halves2, symmetries):
        h1, h2 = np.asarray(h1), np.asarray(h2)
        if h1.ndim != 3 or h1.shape != h2.shape:
            raise ValueError(f"half_map_fsc: the halves must be 3-D maps of one shape; got {h1.shape} and {h2.shape}")
        n = int(h1.shape[1]) // 2 * 2 if size is None else int(size)   # transforms.py:158-164 crops by // 2 on both sides
        for k, h in enumerate((h1, h2)):
            cube = np.asarray(symmetrize(h, float(apix3d), float(twist), float(rise), int(csym), float(fraction), (n, n, n), new_apix,
                                         device=device))
            if cube.shape != (n, n, n):
                raise ValueError(f"half_map_fsc: apply_helical_symmetry returned {cube.shape}, not the {n}^3 cube that was asked "
                                 "for (an odd size is cropped to even: pass an even `size`)")
            cubes[k].append(cube)
    if len({c.shape for c in cubes[0]}) != 1:
        raise ValueError("half_map_fsc: the pairs of one call must give cubes of one size")
    n = cubes[0][0].shape[0]
    curves = fsc_batch(np.stack(cubes[0]), np.stack(cubes[1]), new_apix, per_shell, device=device)
    return [(np.asarray(c), _resolutions(np.asarray(c), n, new_apix, per_shell)) for c in curves]


def half_map_fsc(half1, half2, apix3d, twist_degree, rise_angstrom, csym=1, *, size=None, new_apix=None, fraction=1.0,
                 per_shell=False, device=0):
    """The FSC of two half reconstructions (``h1``, ``h2`` of ``lsq_reconstruct(..., fsc_test=...)``): each half goes through
    ``apply_helical_symmetry(half, apix3d, twist, rise, csym, fraction, (size, size, size), new_apix)`` (``size`` defaults
    to the halves' ``shape[1]``, the box diameter, rounded down to even; ``new_apix`` to ``apix3d``), then ``calc_fsc`` (or
    ``calc_fsc_per_shell``) of the two cubes at ``new_apix``.  Returns ``(curve, {"0.5": A, "0.143": A})``.  ``ValueError``
    if the symmetrised map is not the requested cube."""
    return half_map_fsc_batch([half1], [half2], apix3d, [(twist_degree, rise_angstrom, csym)], size=size, new_apix=new_apix,
                              fraction=fraction, per_shell=per_shell, device=device)[0]


# ------------------------------------------------------------------------------------------
# command line
# ------------------------------------------------------------------------------------------
def add_args(parser: argparse.ArgumentParser) -> argparse.ArgumentParser:
    parser.add_argument("half1", help=".mrc / .map / .npy file with one cubic 3-D map")
    parser.add_argument("half2", help="the second map, of the same shape")
    parser.add_argument("--apix", type=float, default=None, help="voxel size, Angstrom (default: the first map's MRC header)")
    parser.add_argument("--per-shell", action="store_true", help="sums over the full spectrum (calc_fsc_per_shell) instead of calc_fsc's")
    parser.add_argument("--threshold", type=float, nargs="+", default=[0.143, 0.5], help="FSC thresholds of the reported resolutions")
    parser.add_argument("--out", default=None, help="text file with `saxis fsc` rows")
    parser.add_argument("--device", type=int, default=0)
    return parser


def _read_map(path, apix=None):
    if str(path).lower().endswith((".mrc", ".mrcs", ".map")):
        from .mrc import read_mrc

        vol, header_apix = read_mrc(path)
        if apix is None:
            apix = header_apix
    else:
        vol = np.load(path)
    return np.asarray(vol), apix


def run(args, fsc_fn=None) -> dict:
    """``fsc_fn(map1, map2, apix, per_shell, device=)`` stands in for the library calls (tests): it returns what
    ``calc_fsc`` (rows) or ``calc_fsc_per_shell`` (values) returns."""
    m1, apix = _read_map(args.half1, args.apix)
    m2, _ = _read_map(args.half2, args.apix)
    if not apix or apix <= 0:
        raise SystemExit("--apix is required (the maps carry no voxel size)")
    if m1.ndim != 3 or len(set(m1.shape)) != 1 or m1.shape != m2.shape:
        raise SystemExit(f"two cubic maps of one shape are needed; got {tuple(m1.shape)} and {tuple(m2.shape)}")
    n = int(m1.shape[0])
    if n < _MIN_SIDE or n > _MAX_SIDE_3D:
        raise SystemExit(f"the side of the maps must lie in [{_MIN_SIDE}, {_MAX_SIDE_3D}]; got {n}")
    if fsc_fn is None:
        def fsc_fn(a, b, apix_, per_shell, device=0):
            return calc_fsc_per_shell(a, b, apix_, device=device) if per_shell else calc_fsc(a, b, apix_, device=device)
    try:
        curve = np.asarray(fsc_fn(m1, m2, float(apix), bool(args.per_shell), device=args.device))
    except ValueError as e:
        raise SystemExit(str(e))
    if args.per_shell:
        saxis, fsc = np.arange(n // 2 + 1) / (n * float(apix)), curve
    else:
        saxis, fsc = curve[:, 0], curve[:, 1]
    report = {
        "maps": dict(half1=str(args.half1), half2=str(args.half2), shape=[int(v) for v in m1.shape], apix=float(apix)),
        "per_shell": bool(args.per_shell),
        "saxis": [float(v) for v in saxis], "fsc": [float(v) for v in fsc],
        "resolution": {f"{t:g}": fsc_resolution(saxis, fsc, t) for t in args.threshold},
    }
    if args.out:
        np.savetxt(args.out, np.column_stack((saxis, fsc)), fmt="%.9g", header="saxis(1/Angstrom) fsc")
    return report


def main(argv=None) -> int:
    args = add_args(argparse.ArgumentParser(prog="helicon_amd.fsc", description=__doc__.split("\n\n")[0])).parse_args(argv)
    json.dump(run(args), sys.stdout, indent=1)
    sys.stdout.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
