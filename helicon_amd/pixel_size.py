"""Pixel-size calibration from the diffraction ring of a standard (graphene, gold, ice) on the device.

``images2star --calibratePixelSize`` (plugins/images2star/calibratepixelsize.py) evaluates the images' Fourier transform on
a polar band of +-5 % around the standard's ring with ``finufft.nufft2d2``, takes the maximum of ``|F|`` over images and
angles at each radius, and reads the pixel size off the radius of the peak.  Here the transform is the direct sum finufft
approximates, on the f32 MFMA (``csrc/nudft.inc``, ``hh_nudft2d2``), and the maximum is taken on the device; the host
keeps the reference's float64 arithmetic on the 100-sample curve.  STAR files are not read: the functions take arrays,
the command line takes MRC files::

    python -m helicon_amd.pixel_size a.mrc [b.mrc ...] --standard graphene [--apix A] [--curve out.txt]
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import sys

import numpy as np

from . import _lib

__all__ = ["STANDARDS", "nudft2d2", "nudft_chunk", "last_kernel_ms", "fft_resolution_range", "polar_band_points", "ring_maximum",
           "ring_power_curve", "curve_from_ring_maximum", "calibration_band", "calibrate_pixel_size"]

# calibratepixelsize.py:52-54; ice ring at 3.661 A: https://journals.iucr.org/d/issues/2021/04/00/tz5104/index.html
STANDARDS = dict(graphene=2.13, graphene_oxide=2.13, go=2.13, gold=2.355, ice=3.661)   # Angstrom
_MODES = {"complex": 0, "abs": 1}


def nudft_chunk() -> int:
    """Points, and images, of one launch group (compiled in)."""
    return int(_lib.lib().hh_nudft_chunk())


def last_kernel_ms() -> float:
    """Device-event milliseconds of this thread's last transform (kernels only, no copies)."""
    ms = C.c_double(0.0)
    _lib.check(_lib.lib().hh_nudft_kernel_ms(C.byref(ms)))
    return float(ms.value)


def _stack(f):
    f = np.asarray(f)
    if f.ndim not in (2, 3) or np.iscomplexobj(f):
        raise ValueError(f"images must be a real [ny, nx] or [B, ny, nx] array, got shape {f.shape}, dtype {f.dtype}")
    a = np.ascontiguousarray(f if f.ndim == 3 else f[None], dtype=np.float32)
    if a.shape[0] < 1:
        raise ValueError("an empty stack")
    return a, f.ndim == 3


def _points(x, y):
    x = np.ascontiguousarray(np.asarray(x, dtype=np.float64).reshape(-1))
    y = np.ascontiguousarray(np.asarray(y, dtype=np.float64).reshape(-1))
    if x.shape != y.shape:
        raise ValueError(f"x and y differ in length: {x.size} and {y.size}")
    return x, y


def _call(a, x, y, mode, group, out, device):
    f64p, f32p = C.POINTER(C.c_double), C.POINTER(C.c_float)
    _lib.check(_lib.lib().hh_nudft2d2(int(device), a.shape[0], a.shape[1], a.shape[2], a.ctypes.data_as(f32p), x.size,
                                      x.ctypes.data_as(f64p), y.ctypes.data_as(f64p), mode, int(group), out.ctypes.data_as(C.c_void_p)))


def nudft2d2(x, y, f, *, output="complex", device=0):
    """``finufft.nufft2d2(x, y, f)`` as its direct sum: ``F[b, p] = sum_a sum_c f[b, a, c] exp(-i (x[p] (a - ny // 2) +
    y[p] (c - nx // 2)))``, ``x`` with the FIRST image axis.  ``f``: [ny, nx] or [B, ny, nx], any real dtype, carried as
    float32; ``x``, ``y``: float64 radians per pixel, any real value.  Returns complex64 (``output="complex"``) or float32
    ``|F|`` (``"abs"``) of shape [P] or [B, P]."""
    if output not in _MODES:
        raise ValueError(f"output must be 'complex' or 'abs', got {output!r}")
    a, stacked = _stack(f)
    x, y = _points(x, y)
    out = np.empty((a.shape[0], x.size), np.complex64 if output == "complex" else np.float32)
    if x.size:
        _call(a, x, y, _MODES[output], 1, out, device)
    return out if stacked else out[0]


def ring_maximum(x, y, f, group, *, device=0):
    """float32 [group]: the maximum of ``|F|`` over the images and over the points ``p`` with ``p % group == r``, taken on
    the device (no ``F`` is stored); bit for bit the maximum of ``nudft2d2(..., output="abs")``."""
    a, _ = _stack(f)
    x, y = _points(x, y)
    out = np.empty(int(group), np.float32)
    _call(a, x, y, 2, group, out, device)
    return out


def polar_band_points(shape, apix, res_low=0, res_high=0, r_samples=-1, theta_samples=180):
    """(X, Y, R): the band's points as calibratepixelsize.py:100-110 forms them (X, with the cosine, goes with the rows),
    flattened [theta][r], and the radii in 1 / Angstrom."""
    R0 = 1 / res_low if res_low > 0 else 0
    R1 = 1 / res_high if res_high > 0 else 1 / (2 * apix)
    nr = r_samples if r_samples > 0 else min(shape[-2:]) // 2
    R = np.linspace(start=R0, stop=R1, num=nr, endpoint=True)
    Theta = np.linspace(start=0, stop=np.pi, num=theta_samples, endpoint=False)
    Theta, Rg = np.meshgrid(Theta, R, indexing="ij")
    Y = (2 * np.pi * apix * Rg * np.sin(Theta)).flatten(order="C")
    X = (2 * np.pi * apix * Rg * np.cos(Theta)).flatten(order="C")
    return X, Y, R


def fft_resolution_range(images, apix, res_low=0, res_high=0, r_samples=-1, theta_samples=180, return_R_only=False, *, device=0):
    """calibratepixelsize.py:88-127: the transform of ``images`` ([ny, nx] or [B, ny, nx]) on ``theta_samples`` angles in
    [0, pi) x the radii ``linspace(1 / res_low or 0, 1 / res_high or Nyquist, r_samples or min(side) // 2)``; complex64
    [..., theta, r] (a stack of one keeps its axis).  ``return_R_only``: the radii, without touching the device."""
    images = np.asarray(images)
    X, Y, R = polar_band_points(images.shape, apix, res_low, res_high, r_samples, theta_samples)
    if return_R_only:
        return R
    fft = nudft2d2(X, Y, images, device=device)
    return fft.reshape(list(images.shape[:-2]) + [theta_samples, len(R)])


def curve_from_ring_maximum(pwr_1d):
    """calibratepixelsize.py:151-154 in float64: ``pwr_1d - median``, over ``scipy.stats.median_abs_deviation`` (default
    scale).  A constant curve gives NumPy's inf / NaN, as in the reference."""
    from scipy.stats import median_abs_deviation

    pwr_1d = np.array(pwr_1d, dtype=np.float64)
    pwr_1d -= np.median(pwr_1d)
    with np.errstate(divide="ignore", invalid="ignore"):
        return pwr_1d / median_abs_deviation(pwr_1d)


def ring_power_curve(images, apix, res_low, res_high, r_samples, theta_samples, *, device=0, _ring_maximum=None):
    """calibrateMag_process_one_micrograph (calibratepixelsize.py:129-156) without the file read: ``(curve, n_images)``."""
    images = np.asarray(images)
    if images.ndim == 2:
        images = images[None]
    X, Y, R = polar_band_points(images.shape, apix, res_low, res_high, r_samples, theta_samples)
    ring = (_ring_maximum or (lambda x, y, f, group: ring_maximum(x, y, f, group, device=device)))(X, Y, images, len(R))
    return curve_from_ring_maximum(ring), len(images)


def calibration_band(apix, target_res, search_range=0.05, r_samples=100):
    """calibratepixelsize.py:61-78: ``(res_low, res_high, theta_samples)`` of the band searched for a ring at
    ``target_res``; ValueError when the ring lies beyond (1 + sqrt 2) / 2 of the Nyquist resolution."""
    half_corner_res = 1.0 / (1 / (2 * apix) * (1 + np.sqrt(2)) / 2)
    if target_res <= half_corner_res:
        raise ValueError(f"target resolution {target_res} A is beyond the limit ({half_corner_res:.2f} A = (1+sqrt(2))/2 * "
                         f"Nyquist resolution) at {apix} A/pixel")
    corner_res = 2 * apix / np.sqrt(2)
    res_low = target_res * (1 + search_range)
    res_high = max(corner_res, target_res * (1 - search_range))
    theta_samples = int(np.pi / ((1 / res_high - 1 / res_low) / (r_samples - 1) / (1 / target_res))) + 1
    return float(res_low), float(res_high), int(theta_samples)


def calibrate_pixel_size(stacks, apix, standard=None, target_res=None, search_range=0.05, r_samples=100, *, device=0,
                         _ring_maximum=None):
    """The handler's arithmetic (calibratepixelsize.py:50-78, 191-220).  ``stacks``: one array ([ny, nx] or [B, ny, nx]) or a
    sequence of them, one per micrograph or particle file; ``standard``: a key of ``STANDARDS``, or give ``target_res`` in
    Angstrom.  Each stack's curve is weighted by its image count, the mean is detrended (``scipy.signal.detrend``), and
    ``apix_new = round(apix * target_res / res_peak, 3)``.  Returns a dict: apix_new, res_peak, R, pwr_mean, res_low,
    res_high, theta_samples, n_images, changed."""
    from scipy.signal import detrend

    if (standard is None) == (target_res is None):
        raise ValueError("give exactly one of standard and target_res")
    if standard is not None:
        if str(standard).lower() not in STANDARDS:
            raise ValueError(f"unknown standard {standard!r}: one of {sorted(STANDARDS)}")
        target_res = STANDARDS[str(standard).lower()]
    if isinstance(stacks, np.ndarray):
        stacks = [stacks]
    stacks = [np.asarray(s) for s in stacks]
    if not stacks:
        raise ValueError("no images")
    res_low, res_high, theta_samples = calibration_band(apix, target_res, search_range, r_samples)
    pwr_curves, n_ptcls = [], []
    for s in stacks:
        curve, n = ring_power_curve(s, apix, res_low, res_high, r_samples, theta_samples, device=device, _ring_maximum=_ring_maximum)
        pwr_curves.append(curve)
        n_ptcls.append(n)
    pwr_curves = np.vstack(pwr_curves)
    n_ptcls = np.array(n_ptcls)
    pwr_mean = np.sum(pwr_curves * np.expand_dims(n_ptcls, axis=1), axis=0) / n_ptcls.sum()
    pwr_mean = detrend(pwr_mean)
    R = fft_resolution_range(stacks[0], apix, res_low, res_high, r_samples, theta_samples=180, return_R_only=True)
    res_peak = 1 / R[np.argmax(pwr_mean)]
    apix_new = round(apix * target_res / res_peak, 3)   # precision: 0.1 %
    return dict(apix_new=float(apix_new), res_peak=float(res_peak), R=R, pwr_mean=pwr_mean, res_low=res_low, res_high=res_high,
                theta_samples=theta_samples, n_images=[int(n) for n in n_ptcls], changed=bool(apix_new != apix))


def add_args(parser: argparse.ArgumentParser) -> argparse.ArgumentParser:
    parser.add_argument("inputs", nargs="+", help=".mrc files: a micrograph [ny, nx] or a stack [B, ny, nx] each")
    parser.add_argument("--standard", required=True, choices=sorted(STANDARDS), help="the sample whose diffraction ring is sought")
    parser.add_argument("--apix", type=float, default=None, help="the nominal pixel size in Angstrom (default: the first file's header)")
    parser.add_argument("--curve", default=None, help="write the detrended mean curve as two columns (1 / Angstrom, power)")
    parser.add_argument("--device", type=int, default=0)
    return parser


def main(argv=None) -> int:
    from .mrc import read_mrc

    args = add_args(argparse.ArgumentParser(prog="helicon_amd.pixel_size", description=__doc__.split("\n\n")[0])).parse_args(argv)
    stacks, apix = [], args.apix
    for path in args.inputs:
        data, header_apix = read_mrc(path)
        if apix is None:
            apix = header_apix
        stacks.append(np.asarray(data, dtype=np.float32))
    if not apix or not apix > 0:
        raise SystemExit("no pixel size in the header: give --apix")
    res = calibrate_pixel_size(stacks, apix, standard=args.standard, device=args.device)
    R, pwr = res["R"], res["pwr_mean"]
    if args.curve:
        np.savetxt(args.curve, np.hstack((R.reshape((len(R), 1)), pwr.reshape((len(R), 1)))))   # calibratepixelsize.py:224-227
    print(json.dumps(dict(inputs=[str(p) for p in args.inputs], standard=args.standard, target_res=STANDARDS[args.standard], apix=float(apix),
                          apix_new=res["apix_new"], changed=res["changed"], res_peak=res["res_peak"], res_low=res["res_low"],
                          res_high=res["res_high"], theta_samples=res["theta_samples"], r_samples=len(R), n_images=res["n_images"],
                          curve=args.curve)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
