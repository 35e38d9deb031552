"""Structure factors of maps and images on the device: the radially binned power of the spectrum, and amplitude scaling onto
a target profile.

The reference's three functions (lib/filters.py:22-208), with their names, positional order and quirks:

``calculate_structural_factor(data, apix, thresh=None, mask=None, return_fft=False)``
    ``(qbins, sf[, F])``.  ``if thresh:`` the data becomes ``clip(data, thresh, None) - thresh`` (``None`` and ``0``: as it
    is), then ``* mask``.  ``qr = sqrt(qx^2 + qy^2 [+ qz^2]) / apix`` on ``np.fft.fftfreq`` grids, ``qstep = min(qr[qr > 0])``,
    ``nbins = int(qmax / qstep) // 2 * 2``, ``qbins = np.linspace(0, nbins * qstep, nbins)`` (the bin width is
    ``nbins / (nbins - 1)`` times ``qstep``), ``label = searchsorted(qbins, qr, "right") - 1`` (the last bin is open-ended),
    ``sf[i]`` the sum of ``|F|^2`` over the FULL spectrum for label ``i``.
``set_structural_factors(data, apix, target_bins, target_structural_factors, thresh=None, mask=None)``
    ``ratio = sqrt(target(qbins) / sf)`` where ``sf != 0`` else 0, the target interpolated linearly onto ``qbins`` with 0
    outside its range; the spectrum times ``interp1d(qbins, ratio, fill_value=0)(qr)`` (0 for ``qr > qbins[-1]``), inverted.
    With a mask the spectrum that is scaled is that of the RAW data; without one, that of the thresholded data.
``match_structural_factors(data, apix, data_target, apix_target, thresh=None, thresh_target=None, mask=None)``
    the target's profile (with the same mask), then ``set_structural_factors``.

2-D images (sides 2 ... 1024) and 3-D maps (sides 2 ... 512) of any sides, odd and unequal included.  ``qbins``, ``nbins`` and
the target on ``qbins`` are computed here on the host in float64 exactly as the reference does; the device takes the tables
(``qbins`` and the per-axis ``fftfreq``) and reproduces the float64 radius and the search bit for bit, so a voxel that ties
with a bin edge falls where NumPy puts it (csrc/structure_factor.inc).  The transforms are float32 (per-axis DFT products
on the exact-f32 MFMA), ``|F|^2`` and the sums float64; the sums are bit-identical from run to run and independent of the
batch.  Results are float64 arrays.  ``StructureFactorMatcher`` is the resident, batched form: many maps of one shape onto
one target.

    python -m helicon_amd.structure_factor in.mrc out.mrc --target target.mrc [--target-apix A] [--mask m.mrc] [--thresh T] [--thresh-target T]
    python -m helicon_amd.structure_factor in.mrc --profile

The voxel sizes come from the headers.
"""
from __future__ import annotations

import argparse
import ctypes as C
import sys

import numpy as np

from . import _lib

__all__ = ["calculate_structural_factor", "set_structural_factors", "match_structural_factors", "StructureFactorMatcher",
           "structure_factor_bins", "main"]

_MAX_SIDE = {2: 1024, 3: 512}
_MAX_BINS = 726

_f32p, _f64p = C.POINTER(C.c_float), C.POINTER(C.c_double)


def _check_shape(shape, who):
    shape = tuple(int(s) for s in shape)
    if len(shape) not in (2, 3):
        raise ValueError("Input data must be a 2D or 3D array.")
    top = _MAX_SIDE[len(shape)]
    if min(shape) < 2 or max(shape) > top:
        raise ValueError(f"{who}: the sides must lie in [2, {top}]; got {shape}")
    return shape


def structure_factor_bins(shape, apix):
    """``(qbins, freqs)``: the reference's ``np.linspace(0, nbins * qstep, nbins)`` and the ``np.fft.fftfreq`` table of every
    axis, without the full grid.  ``qr`` is monotone in every ``|q_axis|`` (each rounding is), so ``qmax`` is the reference's
    expression at the per-axis largest squares and ``qstep`` the smallest of its values at one axis' smallest non-zero
    frequency with the others at 0: the same float64 numbers as ``np.max(qr)`` and ``np.min(qr[qr > 0])``."""
    shape = _check_shape(shape, "structure_factor_bins")
    apix = float(apix)
    if not (apix > 0 and np.isfinite(apix)):
        raise ValueError(f"apix must be positive and finite; got {apix}")
    freqs = [np.fft.fftfreq(n) for n in shape]

    def radius(qx, qy, qz):
        s = qx**2 + qy**2
        if len(shape) == 3:
            s = s + qz**2
        return np.sqrt(s) / apix

    far = [f[np.argmax(f**2)] for f in freqs]
    near = [f[1] for f in freqs]   # fftfreq(n)[1] = 1 / n: the smallest non-zero |q| of the axis
    zero = np.float64(0.0)
    qz_far = far[0] if len(shape) == 3 else zero
    qmax = radius(far[-1], far[-2], qz_far)
    steps = [radius(near[-1], zero, zero), radius(zero, near[-2], zero)]
    if len(shape) == 3:
        steps.append(radius(zero, zero, near[0]))
    qstep = min(steps)
    nbins = int(qmax / qstep) // 2 * 2
    if nbins < 2:
        raise ValueError(f"a box of shape {shape} gives nbins = {nbins}: the structure factor needs at least 2 bins")
    if nbins > _MAX_BINS:
        raise ValueError(f"a box of shape {shape} gives nbins = {nbins} > {_MAX_BINS}")
    return np.linspace(0, nbins * qstep, nbins), freqs


def _target_on(qbins, target_bins, target_sf):
    from scipy import interpolate

    target_bins = np.asarray(target_bins, dtype=np.float64)
    target_sf = np.asarray(target_sf, dtype=np.float64)
    if target_bins.ndim != 1 or target_bins.shape != target_sf.shape or target_bins.size < 2:
        raise ValueError(f"target_bins and target_structural_factors must be 1-D and of one length >= 2; got {target_bins.shape} and "
                         f"{target_sf.shape}")
    return np.ascontiguousarray(interpolate.interp1d(target_bins, target_sf, bounds_error=False, fill_value=0)(qbins), dtype=np.float64)


def _f32(a, name):
    a = np.asarray(a)
    if a.dtype.kind not in "biuf":
        raise ValueError(f"{name}: the data must be real; got dtype {a.dtype}")
    return np.ascontiguousarray(a, dtype=np.float32)


def _full_spectrum(half, shape):
    """The full complex spectrum from the half ``[..., nx // 2 + 1]`` of a real array: F(-k) = conj F(k)."""
    nx = shape[-1]
    ncol = nx // 2 + 1
    full = np.empty(tuple(shape), dtype=np.complex128)
    full[..., :ncol] = half
    if ncol < nx:
        kx = nx - np.arange(ncol, nx)
        mirror = half
        for axis, n in enumerate(shape[:-1]):
            mirror = np.take(mirror, (-np.arange(n)) % n, axis=axis)
        full[..., ncol:] = np.conj(mirror[..., kx])
    return full


class StructureFactorMatcher:
    """A resident context for maps (or images) of one ``shape`` and voxel size: ``profile(maps)`` and, when a target profile
    ``(target_bins, target_sf)`` was given, ``match(maps, mask=None, thresh=None)`` for a stack ``[B, *shape]`` (or one map)
    in one call.  Every map has its own sums and ratio; the batch shares the target.  ``close()`` frees the device memory
    (also a context manager)."""

    def __init__(self, shape, apix, target_bins=None, target_sf=None, *, device=0):
        self.shape = _check_shape(shape, "StructureFactorMatcher")
        self.apix = float(apix)
        self.qbins, self._freqs = structure_factor_bins(self.shape, self.apix)
        self.nbins = len(self.qbins)
        if (target_bins is None) != (target_sf is None):
            raise ValueError("target_bins and target_sf go together")
        self.target = None if target_bins is None else _target_on(self.qbins, target_bins, target_sf)
        self.device = int(device)
        self._ctx = C.c_void_p(None)
        dims = (C.c_int32 * len(self.shape))(*self.shape)
        freq = np.ascontiguousarray(np.concatenate(self._freqs), dtype=np.float64)
        qb = np.ascontiguousarray(self.qbins, dtype=np.float64)
        tp = self.target.ctypes.data_as(_f64p) if self.target is not None else None
        _lib.check(_lib.lib().hh_sf_create(C.byref(self._ctx), self.device, len(self.shape), dims, self.apix, self.nbins,
                                           qb.ctypes.data_as(_f64p), tp, freq.ctypes.data_as(_f64p)), None)

    # -- arguments -------------------------------------------------------------------------------------------------------
    def _maps(self, maps, who):
        a = _f32(maps, who)
        nd = len(self.shape)
        if a.ndim not in (nd, nd + 1) or tuple(a.shape[-nd:]) != self.shape:
            raise ValueError(f"{who}: maps of shape {self.shape} or stacks [B, {', '.join(map(str, self.shape))}]; got {a.shape}")
        single = a.ndim == nd
        if not single and a.shape[0] < 1:
            raise ValueError(f"{who}: an empty batch")
        return a, single, (1 if single else a.shape[0])

    def _mask(self, mask, who):
        if mask is None:
            return None
        m = _f32(mask, who)
        if tuple(m.shape) != self.shape:
            raise ValueError(f"{who}: the mask must have the maps' shape {self.shape}; got {m.shape}")
        return m

    @staticmethod
    def _thresh(thresh):
        if not thresh:   # the reference's `if thresh:`: None and 0 leave the data as it is
            return 0, 0.0
        t = float(thresh)
        if t != t:
            raise ValueError("thresh is NaN")
        return 1, t

    def _handle(self):
        if not self._ctx:
            raise _lib.HeliconHipError("the StructureFactorMatcher is closed")
        return self._ctx

    # -- calls -----------------------------------------------------------------------------------------------------------
    def profile(self, maps, mask=None, thresh=None, return_fft=False):
        """``sf`` ``[B, nbins]`` float64 (``[nbins]`` for one map); with ``return_fft`` also the full complex spectrum of the
        thresholded and masked maps."""
        a, single, batch = self._maps(maps, "profile")
        m = self._mask(mask, "profile")
        has_t, t = self._thresh(thresh)
        ctx = self._handle()
        sums = np.empty((batch, self.nbins), dtype=np.float64)
        half_shape = self.shape[:-1] + (self.shape[-1] // 2 + 1,)
        spec = np.empty((batch,) + half_shape + (2,), dtype=np.float32) if return_fft else None
        _lib.check(_lib.lib().hh_sf_profile(ctx, a.ctypes.data_as(_f32p), batch, m.ctypes.data_as(_f32p) if m is not None else None, has_t, t,
                                            sums.ctypes.data_as(_f64p), spec.ctypes.data_as(_f32p) if spec is not None else None), None)
        out = sums[0] if single else sums
        if not return_fft:
            return out
        half = spec[..., 0].astype(np.float64) + 1j * spec[..., 1].astype(np.float64)
        full = np.stack([_full_spectrum(h, self.shape) for h in half])
        return out, (full[0] if single else full)

    def match(self, maps, mask=None, thresh=None, return_profile=False):
        """The maps with their profile scaled onto the target, float64, of the input's shape."""
        if self.target is None:
            raise ValueError("match: the StructureFactorMatcher was made without a target profile")
        a, single, batch = self._maps(maps, "match")
        m = self._mask(mask, "match")
        has_t, t = self._thresh(thresh)
        ctx = self._handle()
        out = np.empty(a.shape, dtype=np.float32)
        sums = np.empty((batch, self.nbins), dtype=np.float64)
        _lib.check(_lib.lib().hh_sf_match(ctx, a.ctypes.data_as(_f32p), batch, m.ctypes.data_as(_f32p) if m is not None else None, has_t, t,
                                          out.ctypes.data_as(_f32p), sums.ctypes.data_as(_f64p)), None)
        out = out.astype(np.float64)
        if return_profile:
            return out, (sums[0] if single else sums)
        return out

    def kernel_ms(self):
        """Device milliseconds of the last call: ``dict(profile, second_transform, scaling, inverse)``."""
        ms = (C.c_double * 4)()
        _lib.check(_lib.lib().hh_sf_kernel_ms(self._handle(), ms), None)
        return dict(zip(("profile", "second_transform", "scaling", "inverse"), (float(v) for v in ms)))

    def close(self):
        if self._ctx:
            _lib.lib().hh_sf_destroy(self._ctx)
            self._ctx = C.c_void_p(None)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _data(data, who):
    a = np.asarray(data)
    if a.ndim not in (2, 3):
        raise ValueError("Input data must be a 2D or 3D array.")
    _check_shape(a.shape, who)
    return _f32(a, who)


def _same_shape(mask, a, who):
    if mask is None:
        return
    _f32(mask, who)
    if tuple(np.shape(mask)) != tuple(a.shape):
        raise ValueError(f"{who}: the mask must have the data's shape {a.shape}; got {np.shape(mask)}")


def calculate_structural_factor(data, apix, thresh=None, mask=None, return_fft=False, *, device=0):
    """``(qbins, structural_factor)`` or, with ``return_fft``, ``(qbins, structural_factor, F)``."""
    a = _data(data, "calculate_structural_factor")
    _same_shape(mask, a, "calculate_structural_factor")
    with StructureFactorMatcher(a.shape, apix, device=device) as m:
        got = m.profile(a, mask=mask, thresh=thresh, return_fft=return_fft)
        return (m.qbins, got[0], got[1]) if return_fft else (m.qbins, got)


def set_structural_factors(data, apix, target_bins, target_structural_factors, thresh=None, mask=None, *, device=0):
    """The data with its structure factors scaled onto the target's."""
    a = _data(data, "set_structural_factors")
    _same_shape(mask, a, "set_structural_factors")
    with StructureFactorMatcher(a.shape, apix, target_bins, target_structural_factors, device=device) as m:
        return m.match(a, mask=mask, thresh=thresh)


def match_structural_factors(data, apix, data_target, apix_target, thresh=None, thresh_target=None, mask=None, *, device=0):
    """The data with its structure factors scaled onto those of ``data_target`` (the reference applies the one mask to both,
    so with a mask the two must have one shape)."""
    a, b = _data(data, "match_structural_factors"), _data(data_target, "match_structural_factors")
    _same_shape(mask, a, "match_structural_factors")
    _same_shape(mask, b, "match_structural_factors")
    target_bins, target_sf = calculate_structural_factor(b, apix_target, thresh=thresh_target, mask=mask, device=device)
    return set_structural_factors(a, apix, target_bins, target_sf, thresh=thresh, mask=mask, device=device)


# ------------------------------------------------------------------------------------------
# command line
# ------------------------------------------------------------------------------------------
def _read(path):
    from .mrc import read_mrc

    data, apix = read_mrc(path)
    data = np.asarray(data, dtype=np.float32)
    return (data[0] if data.shape[0] == 1 else data), apix


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m helicon_amd.structure_factor", description=__doc__.split("\n\n")[0])
    ap.add_argument("input")
    ap.add_argument("output", nargs="?")
    ap.add_argument("--target")
    ap.add_argument("--target-apix", type=float, default=None, help="voxel size of the target (default: its header's)")
    ap.add_argument("--mask")
    ap.add_argument("--thresh", type=float, default=None)
    ap.add_argument("--thresh-target", type=float, default=None)
    ap.add_argument("--profile", action="store_true", help="print qbins and sf of the input and stop")
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args(argv)
    data, apix = _read(args.input)
    if not apix > 0:
        ap.error(f"{args.input}: the header holds no voxel size")
    mask = _read(args.mask)[0] if args.mask else None
    if args.profile:
        qbins, sf = calculate_structural_factor(data, apix, thresh=args.thresh, mask=mask, device=args.device)
        for q, s in zip(qbins, sf):
            print(f"{q:.17g} {s:.17g}")
        return 0
    if not args.output or not args.target:
        ap.error("an output file and --target are needed (or --profile)")
    target, apix_target = _read(args.target)
    if args.target_apix is not None:
        apix_target = args.target_apix
    if not apix_target > 0:
        ap.error(f"{args.target}: the header holds no voxel size (give --target-apix)")
    out = match_structural_factors(data, apix, target, apix_target, thresh=args.thresh, thresh_target=args.thresh_target, mask=mask,
                                   device=args.device)
    from .mrc import write_mrc

    write_mrc(args.output, out.astype(np.float32), apix)
    return 0


if __name__ == "__main__":
    sys.exit(main())
