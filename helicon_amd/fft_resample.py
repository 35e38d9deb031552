"""Fourier resampling of a 3-D map (or a 2-D image) on the device: ``fft_rescale`` (lib/transforms.py:663-743),
``fft_crop`` (:610-660) and proc3d's ``--fft_resample`` (plugins/proc3d/fft_resample.py:97-109).

All three are one separable transform: a complex operator per axis, ``[out side, in side]``, applied along z, then y, then
x, and a pointwise epilogue (``hh_separable_transform_3d``, csrc/fourier_resample.inc).  The operators are built here in
float64 and rounded once to float32; the three forms, for an axis of length ``n`` and output length ``on``:

``rescale_operator``   ``E[u, j] = (-1)^u exp(-2 pi i f_u (j - n // 2))``, ``f = fftfreq(on) * 2 * apix / cutoff_res``: the direct
                       sum that ``finufft.nufft3d2(eps=1e-6)`` approximates, with its ``n // 2``-centred modes, times the
                       reference's checkerboard.  With the default arguments on an even side it is the DFT matrix; on an
                       odd side it keeps a phase factor, which is reproduced.
``resample_operator``  ``R = F^-1_on E`` with ``cutoff_res = 2 apix n / on``: proc3d's composition
                       ``ifftn(fft_rescale(...))`` along one axis.  For even ``n`` and ``on`` it is Fourier cropping or
                       padding with the origin at voxel 0 (``on > n``: the spectrum beyond the input's Nyquist frequency is
                       the periodic copy, not zeros); it is the identity for ``on == n`` even.
``crop_operator``      bins ``-h .. h - 1`` (``h = on // 2``) and an inverse of size ``m = 2 h`` on the leading axes; bins
                       ``0 .. h`` with irfft's weights (1, 2, ..., 2, 1) on the last: ``fft_crop`` is the real part of the
                       product.  An odd ``on`` therefore gives ``on - 1`` samples, as in the reference.

Deviations from the reference, on purpose: ``fft_rescale`` returns complex64, not complex128 (the products are float32);
the 3-D branch of ``fft_crop`` is ``irfftn`` of the cropped spectrum, where the reference calls ``irfft2`` and leaves z
untransformed (tests/test_fft_resample_host.py pins the difference on a fixture).

    python -m helicon_amd.fft_resample in.mrc out.mrc --size NZ NY NX [--output abs|real] [--apix A] [--device 0]

resamples a map, writes it with its new voxel size and prints one JSON line.
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import sys

import numpy as np

from . import _lib

__all__ = ["rescale_operator", "resample_operator", "crop_operator", "fft_rescale", "fft_resample", "fft_crop", "last_kernel_ms", "main"]

_MAX_SIDE = 1024
_EPILOGUE = {"store": 0, "abs": 1, "real": 2}


def _side(v, what):
    if int(v) != v or not 1 <= int(v) <= _MAX_SIDE:
        raise ValueError(f"{what}: every side must be an integer in [1, {_MAX_SIDE}]; got {v}")
    return int(v)


def rescale_operator(n, on, apix=1.0, cutoff_res=None):
    """``fft_rescale`` along one axis: complex128 ``[on, n]`` (module docstring); ``cutoff_res=None``: ``2 * apix``."""
    n, on = _side(n, "rescale_operator"), _side(on, "rescale_operator")
    cutoff = 2.0 * apix if cutoff_res is None else float(cutoff_res)
    if not float(apix) > 0 or not cutoff > 0:
        raise ValueError(f"rescale_operator: apix and cutoff_res must be positive; got {apix}, {cutoff_res}")
    f = np.fft.fftfreq(on) * 2.0 * float(apix) / cutoff
    sign = 1.0 - 2.0 * (np.arange(on) % 2)
    return sign[:, None] * np.exp(-2j * np.pi * np.outer(f, np.arange(n) - n // 2))


def resample_operator(n, on):
    """proc3d's ``ifftn(fft_rescale(x, apix, 2 apix n / on, on))`` along one axis, without its scale ``on / n``:
    complex128 ``[on, n]``."""
    n, on = _side(n, "resample_operator"), _side(on, "resample_operator")
    e = rescale_operator(n, on, 1.0, 2.0 * n / on)
    inv = np.exp(2j * np.pi * np.outer(np.arange(on), np.arange(on)) / on) / on
    return inv @ e


def crop_operator(n, on, last):
    """``fft_crop`` along one axis: complex128 ``[2 * (on // 2), n]``; ``last``: the axis rfft / irfft run along."""
    n, on = _side(n, "crop_operator"), _side(on, "crop_operator")
    if on > n or on < 2:
        raise ValueError(f"crop_operator: the output side must lie in [2, {n}]; got {on}")
    h = on // 2
    m = 2 * h
    u = np.arange(0, h + 1) if last else np.arange(-h, h)
    w = np.ones(len(u))
    if last:
        w[1:h] = 2.0
    inv = np.exp(2j * np.pi * np.outer(np.arange(m), u) / m) * (w / m)
    fwd = np.exp(-2j * np.pi * np.outer(u, np.arange(n)) / n)
    return inv @ fwd


def _is_identity(op):
    return op.shape[0] == op.shape[1] and float(np.abs(op - np.eye(op.shape[0])).max()) <= 1e-12


def _real_array(data, name, ndims):
    d = np.asarray(data)
    if d.ndim not in ndims:
        raise ValueError(f"{name}: data must have {' or '.join(str(v) for v in ndims)} dimensions; got {d.ndim}")
    if d.dtype.kind not in "biuf":
        raise ValueError(f"{name}: data must be real; got dtype {d.dtype}")
    if min(d.shape) < 1 or max(d.shape) > _MAX_SIDE:
        raise ValueError(f"{name}: every side must lie in [1, {_MAX_SIDE}]; got {d.shape}")
    return d


def _sizes(size, ndim, name):
    try:
        sides = tuple(size)
    except TypeError:
        raise ValueError(f"{name}: a size is one side per axis; got {size!r}") from None
    if len(sides) != ndim:
        raise ValueError(f"{name}: {len(sides)} sides for a {ndim}-D input")
    return tuple(_side(v, name) for v in sides)


def _apply(d, ops, epilogue, scale, device):
    """The device call: ``ops`` one complex128 ``[out, in]`` operator per axis of ``d`` (2-D: the z pass is skipped);
    operators that are the identity (to 1e-12) are skipped too.  Returns the float32 plane(s) of the epilogue."""
    vol = np.ascontiguousarray(d, dtype=np.float32)
    if vol.ndim == 2:
        vol, ops = vol[None], [np.ones((1, 1), np.complex128), *ops]
    planes_re, planes_im = [], []
    for op, n in zip(ops, vol.shape):
        assert op.shape[1] == n
        if _is_identity(op):
            planes_re.append(None)
            planes_im.append(None)
        else:
            planes_re.append(np.ascontiguousarray(op.real, dtype=np.float32))
            planes_im.append(np.ascontiguousarray(op.imag, dtype=np.float32))
    out_shape = tuple(int(op.shape[0]) for op in ops)
    ptr = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_float))   # noqa: E731
    f32pp = C.POINTER(C.c_float) * 3
    out0 = np.empty(out_shape, np.float32)
    out1 = np.empty(out_shape, np.float32) if epilogue == "store" else None
    _lib.check(_lib.lib().hh_separable_transform_3d(
        int(device), ptr(vol), (C.c_int32 * 3)(*vol.shape), (C.c_int32 * 3)(*out_shape), f32pp(*map(ptr, planes_re)),
        f32pp(*map(ptr, planes_im)), _EPILOGUE[epilogue], float(scale), ptr(out0), ptr(out1)), None)
    keep = slice(None) if d.ndim == 3 else 0
    return out0[keep], None if out1 is None else out1[keep]


def last_kernel_ms() -> float:
    """Device-event time of the last call's passes, milliseconds (the copies of the map excluded)."""
    ms = C.c_double(0.0)
    _lib.check(_lib.lib().hh_separable_transform_kernel_ms(C.byref(ms)), None)
    return ms.value


def fft_rescale(data, apix=1.0, cutoff_res=None, output_size=None, *, device=0):
    """``helicon.fft_rescale`` (lib/transforms.py:663-743) of a 2-D image or a 3-D map: its Fourier coefficients at
    ``output_size`` frequencies ``fftfreq(on) * 2 * apix / cutoff_res`` per axis.  complex64 (the reference: complex128)."""
    d = _real_array(data, "fft_rescale", (2, 3))
    if not float(apix) > 0:
        raise ValueError(f"fft_rescale: apix must be positive; got {apix}")
    cut = (2.0 * apix,) * d.ndim if not cutoff_res else tuple(float(c) for c in cutoff_res)
    if len(cut) != d.ndim or not all(c > 0 for c in cut):
        raise ValueError(f"fft_rescale: cutoff_res must be {d.ndim} positive values; got {cutoff_res}")
    size = d.shape if not output_size else _sizes(output_size, d.ndim, "fft_rescale")
    ops = [rescale_operator(n, on, apix, c) for n, on, c in zip(d.shape, size, cut)]
    re, im = _apply(d, ops, "store", 1.0, device)
    out = np.empty(re.shape, np.complex64)
    out.real, out.imag = re, im
    return out


def fft_resample(data, apix, new_size, *, output="abs", device=0):
    """proc3d's ``--fft_resample`` of a 3-D map to ``new_size`` = (nz, ny, nx), up or down: returns ``(map, new_apix)``,
    the map float32 and ``new_apix = round(apix * nx / new_nx, 4)``.

    ``output="abs"`` is the reference's ``|ifftn(fft_rescale(...))| * prod(new) / prod(old)``, which makes negative
    density positive; ``output="real"`` keeps the sign (the real part).  On an odd side, old or new, the transform keeps
    a phase factor (module docstring), so the result is the reference's but not a resampled map."""
    if output not in ("abs", "real"):
        raise ValueError(f"fft_resample: output must be 'abs' or 'real'; got {output!r}")
    d = _real_array(data, "fft_resample", (3,))
    if not float(apix) > 0:
        raise ValueError(f"fft_resample: apix must be positive; got {apix}")
    size = _sizes(new_size, 3, "fft_resample")
    ops = [resample_operator(n, on) for n, on in zip(d.shape, size)]
    scale = float(np.prod(size, dtype=np.float64) / np.prod(d.shape, dtype=np.float64))
    out, _ = _apply(d, ops, output, scale, device)
    return out, round(float(apix) * d.shape[2] / size[2], 4)


def fft_crop(data, output_size=None, *, device=0):
    """``helicon.fft_crop`` (lib/transforms.py:610-660): crop a 2-D image or a 3-D map in Fourier space.  float32 with
    ``2 * (on // 2)`` samples per axis; the input itself when ``output_size`` is ``None`` or the shape.  The reference's
    assertions (2-D or 3-D, one side per axis, none larger than the input's) are ``ValueError`` here.  3-D: ``irfftn`` of
    the cropped spectrum (the reference's ``irfft2`` there leaves z untransformed)."""
    if output_size is None or tuple(np.shape(data)) == tuple(output_size):
        return data
    d = _real_array(data, "fft_crop", (2, 3))
    size = _sizes(output_size, d.ndim, "fft_crop")
    if any(on > n for on, n in zip(size, d.shape)) or min(size) < 2:
        raise ValueError(f"fft_crop: every output side must lie in [2, the input's]; got {size} for {d.shape}")
    ops = [crop_operator(n, on, ax == d.ndim - 1) for ax, (n, on) in enumerate(zip(d.shape, size))]
    out, _ = _apply(d, ops, "real", 1.0, device)
    return out


# ------------------------------------------------------------------------------------------
# command line
# ------------------------------------------------------------------------------------------
def add_args(parser: argparse.ArgumentParser) -> argparse.ArgumentParser:
    parser.add_argument("input", help=".mrc / .map file with one 3-D map [nz, ny, nx]")
    parser.add_argument("output", help=".mrc file to write")
    parser.add_argument("--size", type=int, nargs=3, metavar=("NZ", "NY", "NX"), required=True, help="the new sides")
    parser.add_argument("--output", dest="kind", choices=("abs", "real"), default="abs",
                        help="abs: the reference's |.| (default); real: the signed map")
    parser.add_argument("--apix", type=float, default=None, help="voxel size, Angstrom (default: the MRC header's)")
    parser.add_argument("--device", type=int, default=0)
    return parser


def main(argv=None) -> int:
    from .mrc import read_mrc, write_mrc

    args = add_args(argparse.ArgumentParser(prog="helicon_amd.fft_resample", description=__doc__.split("\n\n")[0])).parse_args(argv)
    vol, apix = read_mrc(args.input)
    if args.apix is not None:
        apix = args.apix
    if not apix or apix <= 0:
        raise SystemExit("--apix is required (the map carries no voxel size)")
    try:
        out, new_apix = fft_resample(np.asarray(vol), apix, args.size, output=args.kind, device=args.device)
    except ValueError as e:
        raise SystemExit(str(e))
    write_mrc(args.output, out, new_apix)
    print(json.dumps(dict(input=str(args.input), output=str(args.output), shape=[int(v) for v in vol.shape], apix=float(apix),
                          new_shape=[int(v) for v in out.shape], new_apix=new_apix, kind=args.kind, kernel_ms=last_kernel_ms())))
    return 0


if __name__ == "__main__":
    sys.exit(main())
