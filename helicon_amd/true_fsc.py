"""Phase-randomised ("true") FSC of two half maps, on the device: the noise-substitution method of Chen et al. 2013
(Ultramicroscopy 135:24-35) as the reference runs it (commands/trueFSC.py, lib/filters.py:469-520).

A mask correlates the two half maps in Fourier space and inflates their FSC.  The method measures that inflation:

1. the phases of both maps are randomised beyond a cutoff resolution (``randomize_phases_lowpass``);
2. ``fsc_t`` is the FSC of the masked maps, ``fsc_n`` the FSC of the masked phase-randomised maps;
3. beyond the cutoff ``fsc_true = (fsc_t - fsc_n) / (1 - fsc_n)``.

``randomize_phases_lowpass(data, apix, cutoff_res, return_fft=False)``
    the reference's function: name, positional order and return shape.  Without ``phases=`` / ``seed=`` it draws
    ``np.random.uniform(0, 2 pi, size=(n, n, n // 2 + 1))`` on the host exactly as the reference does, so after
    ``np.random.seed(k)`` it consumes the same stream and gives the reference's result.  ``phases=`` takes the angles,
    ``seed=`` uses the device's counter-based generator (no host draw, no upload).
``TrueFSC(map1, map2, apix, cutoff_res=0)``
    the resident context (``hh_tfsc_*``, csrc/true_fsc.inc): both maps and both randomised maps stay on the device; every
    ``.masked(mask)`` uploads the mask only.
``true_fsc(map1, map2, apix, ...)``
    the composition of ``trueFSC.py:main`` (lines 102-366): cutoff rule, masks (given, or adaptive with a soft edge that is
    given, defaulted or refined), the five curves, the fitted curve and the resolutions at 0.143.

Two deliberate deviations from the reference, both at inputs it handles by accident:

* the randomised set is ``m = kz^2 + ky^2 + kx^2 >= m_cut`` in integers, ``m_cut`` the smallest integer
  ``>= (apix / cutoff_res)^2 n^2``.  The reference compares a float64 sum of three rounded squares of ``fftfreq`` values with
  ``(apix / cutoff_res)^2``; the two rules differ only on a TIE, a bin whose ``m / n^2`` equals the threshold to within
  float64 rounding, which the reference decides by that rounding.  Here a product within 1e-9 (relative) of an integer is
  that integer, so a tie is always inside the randomised set;
* odd sides raise ``ValueError``: the reference's ``irfftn`` returns a map whose last axis is ``n - 1`` there.

Precision: float32 transforms, float64 shell sums, like ``helicon_amd.fsc``.  The mask helpers (``soft_mask``,
``adaptive_mask``, ``otsu_threshold_eman``, ``fit_fsc_curve``) run on the host and call SciPy where the reference does.

Soft masks on the device (csrc/soft_mask.inc): ``soft_mask``'s definition with its quirks (the 1 -> 0.5 -> 0 edge, the planes
``zoom`` leaves at 0 distance) from a binary support that is uploaded once.

``distance_transform_edt_sq(support, stride=1)``
    the exact squared Euclidean distance transform (int32) of ``~support[::stride, ::stride, ::stride]``.
``soft_mask_device(mask, soft_width)``
    ``soft_mask`` of any 3-D box on the device, float32.
``TrueFSC.set_support`` / ``.soft_mask`` / ``.soft_masked`` / ``.soft_masked_batch``
    the supports stay on the context; every width becomes a mask in device memory that feeds the masked curves directly.
``true_fsc(..., device_masks=True)``
    the soft edge and every trial of ``refine_mask`` on the device; ``adaptive_mask`` stays on the host.

Adaptive masks on the device (csrc/adaptive_mask.inc): ``adaptive_mask``'s definition from the volume in float64 (a float32
volume is widened exactly).  One deviation: ``np.argpartition`` keeps an arbitrary 1000 of the voxels tied at the 1000th
largest value ``v*``; the device takes every voxel ``>= v*`` as a seed.  Fewer than 1000 voxels, a NaN or infinite voxel and
a constant volume in Otsu mode raise ``ValueError``.

``gaussian_taps(sigma)``
    the half kernel ``w[0 ... r]`` of ``scipy.ndimage.gaussian_filter``, ``r = int(4 sigma + 0.5)``, by SciPy's NumPy expression.
``gaussian_filter_device(volume, sigma)``
    ``gaussian_filter(volume.astype(float64), sigma)`` (mode ``reflect``): the same taps, passes z, y, x, unfused float64.
``label_components(binary)``
    ``scipy.ndimage.label(binary, structure=np.ones((3, 3, 3)))``: ``(labels, n)``, numbered in order of first occurrence.
``otsu_from_counts(counts, hmin, hmax)``
    ``otsu_threshold_eman`` from the histogram on.
``adaptive_mask_device(volume, apix, cutoff_res, ...)``
    the mask as uint8 0 / 1; ``info=True`` adds the threshold, ``v*`` and the counts.
``TrueFSC.adaptive_support`` / ``.support``
    the support(s) built from the context's resident maps, left where ``set_support`` leaves them, and downloaded.
``true_fsc(..., device_masks=True, device_support=True)``
    nothing of the masks runs on the host: ``host_mask_s`` is 0.  The maps must be exactly representable in float32 (the
    context holds float32; the host path filters the caller's float64).

    python -m helicon_amd.true_fsc half1.mrc half2.mrc [--apix A] [--mask M [M2]] [--one-mask] [--cutoff-res R]
        [--mask-soft W] [--refine-mask] [--mask-fraction-thresh F | --mask-thresh T | --mask-mass KDA] [--seed S]
        [--out-prefix P] [--device 0] [--device-masks [--device-support]]

prints a JSON report and, with ``--out-prefix``, writes ``P.unmasked.txt``, ``P.randomized-unmasked.txt``, ``P.masked.txt``,
``P.randomized-masked.txt``, ``P.true.txt``, ``P.true.fit.txt`` (the reference's six text files) and the mask(s).
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import math
import sys

import numpy as np

from . import _lib
from .fsc import _f32, _fsc_rows, _ratio, _read_map, calc_fsc, fsc_resolution

__all__ = ["randomize_phases_lowpass", "TrueFSC", "true_fsc", "cutoff_m", "choose_cutoff", "soft_mask", "adaptive_mask",
           "otsu_threshold_eman", "fit_fsc_curve", "distance_transform_edt_sq", "soft_mask_device", "soft_step", "zoom_taps",
           "gaussian_taps", "gaussian_filter_device", "label_components", "otsu_from_counts", "adaptive_mask_device", "adaptive_stage_ms", "main"]

_MIN_SIDE, _MAX_SIDE = 8, 512
_f32p, _f64p = C.POINTER(C.c_float), C.POINTER(C.c_double)
_u8p, _i32p = C.POINTER(C.c_uint8), C.POINTER(C.c_int32)
_MAX_BOX = 1024
_i64p = C.POINTER(C.c_int64)
_MAX_VOXELS, _MAX_RADIUS, _N_SEEDS = 2**28, 4096, 1000


# ------------------------------------------------------------------------------------------
# the cutoff
# ------------------------------------------------------------------------------------------
def cutoff_m(n, apix, cutoff_res):
    """``m_cut``: bins with ``kz^2 + ky^2 + kx^2 >= m_cut`` are randomised.  The smallest integer ``>= (apix / cutoff_res)^2
    n^2``; a product within 1e-9 (relative) of an integer counts as that integer (a tie is randomised)."""
    if not cutoff_res > 0:
        raise ValueError(f"the cutoff resolution must be positive; got {cutoff_res}")
    t = (float(apix) / float(cutoff_res)) ** 2 * float(n) * float(n)
    r = round(t)
    if abs(t - r) <= 1e-9 * max(1.0, t):
        return int(min(r, 2**62))
    return int(min(math.ceil(t), 2**62))


def choose_cutoff(saxis, fsc_unmasked, cutoff_res=0):
    """trueFSC.py:122-135: a given value > 2 as it is; else the resolution at 0.8 of the unmasked curve (of the fitted curve
    if that is above 100 Angstrom), rounded to 1 (> 10), 1/2 (> 5) or 1/4 Angstrom steps."""
    if cutoff_res > 2:
        return cutoff_res
    res = fsc_resolution(saxis, fsc_unmasked, 0.8)
    if res > 100:
        s_fit, f_fit, _ = fit_fsc_curve(saxis, fsc_unmasked)
        res = fsc_resolution(s_fit, f_fit, 0.8)
    if res > 10:
        return round(res)
    if res > 5:
        return round(res * 2) / 2
    return round(res * 4) / 4


def fit_fsc_curve(saxis, fsc, order=4):
    """trueFSC.py:465-566 on the host: ``(saxis_fine, fsc_fine, resolution at 0.143)`` of the better of a Fermi and a
    Butterworth curve fitted (mean absolute deviation, Nelder-Mead) to the points with -0.1 <= fsc <= 1.1; fewer than three
    such points: the curve itself."""
    from scipy.optimize import minimize

    saxis, fsc = np.asarray(saxis, dtype=np.float64), np.asarray(fsc, dtype=np.float64)
    use = np.isfinite(fsc) & (fsc >= -0.1) & (fsc <= 1.1)
    s_fit, f_fit = saxis[use], fsc[use]
    if len(s_fit) < 3:
        return saxis, fsc, fsc_resolution(saxis, fsc, 0.143)

    def fermi(mu, t, x):
        return 1.0 / (np.exp((x - mu) / t) + 1.0)

    def butterworth(omega, n, x):
        return 1.0 / (1.0 + (x / omega) ** n)

    def fit_score_fermi(params):
        mu, t = params
        if t <= 0:
            return 1e10
        return np.mean(np.abs(f_fit - 1.0 / fermi(mu, t, 0.0) * fermi(mu, t, s_fit)))

    def fit_score_butterworth(params):
        omega, n = params
        if omega <= 0 or n <= 0:
            return 1e10
        return np.mean(np.abs(f_fit - butterworth(omega, n, s_fit)))

    def crossing(s_fine, f_fine, res):
        idx = np.where(f_fine < 0.143)[0]
        if len(idx) > 0 and idx[0] > 0:
            i = idx[0]
            cross = s_fine[i - 1] + (0.143 - f_fine[i - 1]) * (s_fine[i] - s_fine[i - 1]) / (f_fine[i] - f_fine[i - 1])
            return 1.0 / cross if cross > 0 else 999.0
        return res

    best_error = np.inf
    best_s, best_f = s_fit.copy(), f_fit.copy()
    best_res = fsc_resolution(s_fit, f_fit, 0.143)
    options = {"maxiter": 1000, "xatol": 1e-6}
    s_fine = np.linspace(saxis[1], saxis[-1], 500)
    fit = minimize(fit_score_fermi, x0=[s_fit[len(s_fit) // 2], 0.01], method="Nelder-Mead", options=options)
    if fit.fun < best_error:
        best_error = fit.fun
        mu, t = fit.x
        best_s, best_f = s_fine, np.clip(1.0 / fermi(mu, t, 0.0) * fermi(mu, t, s_fine), -1, 1)
        best_res = crossing(best_s, best_f, best_res)
    fit = minimize(fit_score_butterworth, x0=[s_fit[len(s_fit) // 2], 2.0], method="Nelder-Mead", options=options)
    if fit.fun < best_error:
        omega, n = fit.x
        best_s, best_f = s_fine, np.clip(butterworth(omega, n, s_fine), -1, 1)
        best_res = crossing(best_s, best_f, best_res)
    return best_s, best_f, best_res


# ------------------------------------------------------------------------------------------
# masks (host)
# ------------------------------------------------------------------------------------------
def otsu_threshold_eman(volume, n_bins=256, ignore_zero=True):
    """trueFSC.py:608-657: Otsu's threshold on a 256-bin histogram, zero voxels left out, the first bin skipped."""
    hmin, hmax = float(np.min(volume)), float(np.max(volume))
    bin_width = (hmax - hmin) / n_bins
    flat = volume.ravel()
    if ignore_zero:
        flat = flat[flat != 0]
    if len(flat) == 0:
        return hmin
    hist, _ = np.histogram(flat, bins=n_bins, range=(hmin, hmax))
    hist = hist.astype(np.float64)
    total = hist.sum()
    if total == 0:
        return hmin
    sum_all = np.dot(np.arange(n_bins, dtype=np.float64), hist)
    cumsum = np.cumsum(hist)
    cumsum_val = np.cumsum(np.arange(n_bins, dtype=np.float64) * hist)
    w_b, w_f = cumsum, total - cumsum
    m_b, m_f = np.zeros(n_bins), np.zeros(n_bins)
    valid = (w_b > 0) & (w_f > 0)
    m_b[valid] = cumsum_val[valid] / w_b[valid]
    m_f[valid] = (sum_all - cumsum_val[valid]) / w_f[valid]
    between = w_b * w_f * (m_b - m_f) ** 2
    max_bi = np.argmax(between[1:]) + 1
    return hmin + (max_bi + 1) * bin_width


def adaptive_mask(volume, apix, cutoff_res, mask_fraction_thresh=0, mask_thresh=0, mask_mass=0):
    """trueFSC.py:660-735: the map low-passed (``gaussian_filter``, sigma = cutoff_res / (3.81 apix)) when ``cutoff_res > 2
    apix``, thresholded (a fraction of the maximum, a value, the value that encloses ``mask_mass`` kDa, or Otsu's), and the
    connected components (26-neighbourhood) that hold one of the 1000 brightest voxels kept.  A float64 0 / 1 map."""
    from scipy.ndimage import gaussian_filter, label

    volume = np.asarray(volume)
    if cutoff_res > 2 * apix:
        volume_lp = gaussian_filter(volume, sigma=cutoff_res / (3.81 * apix))
    else:
        volume_lp = volume.copy()
    if mask_fraction_thresh > 0:
        thresh = mask_fraction_thresh * np.max(volume_lp)
    elif mask_thresh and mask_thresh > 0:
        thresh = mask_thresh
    elif mask_mass > 0:
        vol_voxels = mask_mass * 1e3 / (0.81 * apix**3)
        sorted_vals = np.sort(volume_lp.ravel())[::-1]
        thresh = sorted_vals[min(int(vol_voxels), len(sorted_vals) - 1)]
    else:
        thresh = otsu_threshold_eman(volume_lp)
    nmaxseed = 1000
    flat_idx = np.argpartition(volume_lp.ravel(), -nmaxseed)[-nmaxseed:]
    above_thresh = volume_lp > thresh
    labeled, _ = label(above_thresh, structure=np.ones((3, 3, 3), dtype=bool))
    seed_labels = labeled.ravel()[flat_idx]
    seed_labels = seed_labels[seed_labels > 0]
    mask = np.isin(labeled, np.unique(seed_labels))
    if not np.any(mask):
        mask = above_thresh.copy()
    return mask.astype(np.float64)


def soft_mask(mask, soft_width):
    """trueFSC.py:738-781: a cosine edge of ``soft_width`` pixels outside a binary mask; the distance is SciPy's exact
    transform of the mask taken at every ``max(1, int(soft_width / 4))``-th voxel, times that step, ``zoom``ed (order 1) back."""
    if soft_width <= 0:
        return np.asarray(mask).astype(np.float64)
    from scipy.ndimage import distance_transform_edt, zoom

    mask = np.asarray(mask)
    nz, ny, nx = mask.shape
    step = max(1, int(soft_width / 4))
    mask_ds = mask[::step, ::step, ::step].astype(bool)
    dist_ds = distance_transform_edt(~mask_ds) * step
    dist = zoom(dist_ds, (nz / dist_ds.shape[0], ny / dist_ds.shape[1], nx / dist_ds.shape[2]), order=1)
    dist = dist[:nz, :ny, :nx]
    soft = np.ones(mask.shape, dtype=np.float64)
    outside = ~mask.astype(bool)
    near_edge = outside & (dist > 0) & (dist <= soft_width)
    soft[near_edge] = (np.cos(dist[near_edge] / soft_width * np.pi / 2) + 1) / 2
    soft[outside & (dist > soft_width)] = 0.0
    return soft


# ------------------------------------------------------------------------------------------
# masks (device)
# ------------------------------------------------------------------------------------------
def soft_step(soft_width):
    """``soft_mask``'s decimation step ``max(1, int(soft_width / 4))``."""
    return max(1, int(soft_width / 4))


def zoom_taps(n, m):
    """The per-axis tables of ``scipy.ndimage.zoom(order=1)`` (``mode="constant"``) from ``m`` samples to ``n``:
    ``(i0, i1, w0, w1, outside)``, ``[n]`` each.  Coordinate ``c = i (m - 1) / (n - 1)`` in float64, taps ``floor(c)`` and
    ``floor(c) + 1`` clamped to the line with weights ``1 - f`` and ``f``; ``outside`` marks ``c > m - 1``, where ``zoom``
    returns 0 (for some ``(n, m)`` the last index lands one ulp beyond the last sample).  The library's host function
    (``hh_soft_mask_taps``): the tables the device kernel reads; no device is needed."""
    n, m = int(n), int(m)
    if not 1 <= m <= n <= _MAX_BOX:
        raise ValueError(f"zoom_taps: 1 <= m <= n <= {_MAX_BOX} is needed; got n = {n}, m = {m}")
    i0, i1, out = np.empty(n, np.int32), np.empty(n, np.int32), np.empty(n, np.int32)
    w0, w1 = np.empty(n, np.float64), np.empty(n, np.float64)
    _lib.check(_lib.lib().hh_soft_mask_taps(n, m, i0.ctypes.data_as(_i32p), i1.ctypes.data_as(_i32p), w0.ctypes.data_as(_f64p),
                                            w1.ctypes.data_as(_f64p), out.ctypes.data_as(_i32p)), None)
    return i0, i1, w0, w1, out.astype(bool)


def _width(w, name):
    w = float(w)
    if not math.isfinite(w):
        raise ValueError(f"{name}: the width of the soft edge is NaN or infinite")
    return w


def _support(mask, name, shape=None):
    """uint8 0 / 1 of a 3-D mask (nonzero = inside)."""
    m = np.asarray(mask)
    if m.ndim != 3 or min(m.shape, default=0) < 1 or max(m.shape) > _MAX_BOX:
        raise ValueError(f"{name}: a 3-D support with sides in [1, {_MAX_BOX}] is needed; got {m.shape}")
    if shape is not None and m.shape != shape:
        raise ValueError(f"{name}: a support must have the maps' shape {shape}; got {m.shape}")
    if m.dtype.kind == "f" and not np.isfinite(m).all():
        raise ValueError(f"{name}: the support holds NaN or infinite values")
    return np.ascontiguousarray(m != 0, dtype=np.uint8)


def _not_empty(sup, step, name):
    if not sup[::step, ::step, ::step].any():
        raise ValueError(f"{name}: the support has no inside voxel left at every {step}-th voxel (step {step}): there is no distance to take")


def distance_transform_edt_sq(support, stride=1, *, device=0):
    """``np.rint(scipy.ndimage.distance_transform_edt(~S[::stride, ::stride, ::stride]) ** 2)`` exactly, as int32, on the
    device: the squared Euclidean distance of every (decimated) voxel to the nearest inside one.  Sides 1 ... 1024."""
    sup = _support(support, "distance_transform_edt_sq")
    stride = int(stride)
    if stride < 1:
        raise ValueError(f"distance_transform_edt_sq: stride must be >= 1; got {stride}")
    _not_empty(sup, stride, "distance_transform_edt_sq")
    out = np.empty(tuple(-(-v // stride) for v in sup.shape), dtype=np.int32)
    nz, ny, nx = sup.shape
    ms = C.c_double(0.0)
    _lib.check(_lib.lib().hh_edt_3d(int(device), sup.ctypes.data_as(_u8p), nz, ny, nx, stride, out.ctypes.data_as(_i32p), C.byref(ms)), None)
    distance_transform_edt_sq.kernel_ms = ms.value
    return out


def soft_mask_device(mask, soft_width, *, device=0):
    """``soft_mask(mask, soft_width)`` on the device, float32: the same step, exact distances, ``zoom``'s taps and edge rule,
    evaluated in float64 and rounded once.  ``soft_width <= 0``: the support as 0 / 1, no device call.  A support with no
    inside voxel at the step, a NaN or an infinite width raise ``ValueError``."""
    sup = _support(mask, "soft_mask_device")
    w = _width(soft_width, "soft_mask_device")
    if w <= 0:
        return sup.astype(np.float32)
    _not_empty(sup, soft_step(w), "soft_mask_device")
    out = np.empty(sup.shape, dtype=np.float32)
    nz, ny, nx = sup.shape
    ms = C.c_double(0.0)
    _lib.check(_lib.lib().hh_soft_mask_3d(int(device), sup.ctypes.data_as(_u8p), nz, ny, nx, w, out.ctypes.data_as(_f32p), C.byref(ms)), None)
    soft_mask_device.kernel_ms = ms.value
    return out


# ------------------------------------------------------------------------------------------
# adaptive masks (device)
# ------------------------------------------------------------------------------------------
def gaussian_taps(sigma):
    """``w[0 ... r]``, ``r = int(4 sigma + 0.5)``: the half of ``scipy.ndimage``'s Gaussian kernel from its centre, computed by
    SciPy's own NumPy expression (``exp(-0.5 / sigma^2 x^2)`` over ``x = -r ... r``, divided by its sum), in float64."""
    sigma = float(sigma)
    if not (math.isfinite(sigma) and sigma > 0):
        raise ValueError(f"gaussian_taps: sigma must be positive and finite; got {sigma}")
    if 4.0 * sigma + 0.5 >= _MAX_RADIUS + 1:
        raise ValueError(f"gaussian_taps: int(4 sigma + 0.5) must not exceed {_MAX_RADIUS}; got sigma = {sigma}")
    r = int(4.0 * sigma + 0.5)
    x = np.arange(-r, r + 1)
    phi = np.exp(-0.5 / (sigma * sigma) * x ** 2)
    phi = phi / phi.sum()
    return np.ascontiguousarray(phi[r:])


def _volume(volume, name, min_voxels=1):
    """(contiguous float32 or float64 array, is_f64) of a finite 3-D volume within the library's limits."""
    v = np.asarray(volume)
    if v.ndim != 3 or min(v.shape, default=0) < 1 or max(v.shape) > _MAX_BOX:
        raise ValueError(f"{name}: a 3-D volume with sides in [1, {_MAX_BOX}] is needed; got {v.shape}")
    if v.size > _MAX_VOXELS:
        raise ValueError(f"{name}: at most 2^28 voxels; got {v.size}")
    if v.size < min_voxels:
        raise ValueError(f"{name}: at least {min_voxels} voxels are needed (the seeds are the {_N_SEEDS} brightest); got {v.size}")
    v = np.ascontiguousarray(v, dtype=np.float32 if v.dtype == np.float32 else np.float64)
    if not np.isfinite(v).all():
        raise ValueError(f"{name}: the volume holds NaN or infinite values")
    return v, v.dtype == np.float64


def gaussian_filter_device(volume, sigma, *, device=0):
    """``scipy.ndimage.gaussian_filter(volume.astype(float64), sigma)`` (mode ``reflect``, truncate 4) on the device, float64:
    SciPy's taps (``gaussian_taps``), its passes z, y, x and its order of operations, products and sums unfused."""
    v, _ = _volume(volume, "gaussian_filter_device")
    v = np.ascontiguousarray(v, dtype=np.float64)
    taps = gaussian_taps(sigma)
    out = np.empty_like(v)
    nz, ny, nx = v.shape
    _lib.check(_lib.lib().hh_am_gaussian_3d(int(device), v.ctypes.data_as(_f64p), nz, ny, nx, float(sigma), taps.ctypes.data_as(_f64p),
                                            out.ctypes.data_as(_f64p)), None)
    return out


def label_components(binary, *, device=0):
    """``scipy.ndimage.label(binary, structure=np.ones((3, 3, 3)))`` on the device: ``(labels, n)``, int32 labels 1 ... n in the
    order of each component's first voxel (its root, the smallest flat index), 0 on background."""
    sup = _support(binary, "label_components")
    roots = np.empty(sup.shape, dtype=np.int32)
    n = C.c_int64(0)
    nz, ny, nx = sup.shape
    _lib.check(_lib.lib().hh_am_label_3d(int(device), sup.ctypes.data_as(_u8p), nz, ny, nx, roots.ctypes.data_as(_i32p), C.byref(n)), None)
    flat = roots.ravel()
    ids = np.flatnonzero(flat == np.arange(flat.size))      # the roots, ascending
    if len(ids) != n.value:
        raise _lib.HeliconHipError(f"label_components: {len(ids)} roots in the array, {n.value} counted on the device")
    labels = np.zeros(flat.size, dtype=np.int32)
    inside = flat >= 0
    labels[inside] = np.searchsorted(ids, flat[inside]) + 1
    return labels.reshape(sup.shape), int(n.value)


def otsu_from_counts(counts, hmin, hmax):
    """``otsu_threshold_eman`` from its histogram on: the threshold from 256 counts over ``[hmin, hmax]``."""
    hist = np.asarray(counts).astype(np.float64)
    n_bins = len(hist)
    hmin, hmax = float(hmin), float(hmax)
    bin_width = (hmax - hmin) / n_bins
    total = hist.sum()
    if total == 0:
        return hmin
    sum_all = np.dot(np.arange(n_bins, dtype=np.float64), hist)
    cumsum = np.cumsum(hist)
    cumsum_val = np.cumsum(np.arange(n_bins, dtype=np.float64) * hist)
    w_b, w_f = cumsum, total - cumsum
    m_b, m_f = np.zeros(n_bins), np.zeros(n_bins)
    valid = (w_b > 0) & (w_f > 0)
    m_b[valid] = cumsum_val[valid] / w_b[valid]
    m_f[valid] = (sum_all - cumsum_val[valid]) / w_f[valid]
    between = w_b * w_f * (m_b - m_f) ** 2
    max_bi = np.argmax(between[1:]) + 1
    return hmin + (max_bi + 1) * bin_width


_STAGES = ("gauss_z", "gauss_y", "gauss_x", "statistics", "runs", "unions", "flatten", "pick")


def adaptive_stage_ms(reset=True):
    """Device-event milliseconds the mask calls (``adaptive_mask_device``, ``TrueFSC.adaptive_support``) spent per stage since
    the last reset: the three Gaussian passes, the statistics (minimum, maximum, histogram, selections), runs, unions,
    flatten, and the pick of the seeded components."""
    ms = np.zeros(8, dtype=np.float64)
    _lib.check(_lib.lib().hh_am_stage_ms(ms.ctypes.data_as(_f64p), 1 if reset else 0), None)
    return dict(zip(_STAGES, (float(v) for v in ms)))


_INFO_KEYS = ("threshold", "min", "max", "v_star", "above", "kept", "components")


def _mask_mode(n_voxels, apix, cutoff_res, mask_fraction_thresh, mask_thresh, mask_mass, name):
    """(sigma, taps or None, mode, value) of ``adaptive_mask``'s arguments, in its order of precedence."""
    apix, cutoff_res = float(apix), float(cutoff_res)
    if not (math.isfinite(apix) and apix > 0 and math.isfinite(cutoff_res)):
        raise ValueError(f"{name}: apix must be positive and the cutoff finite; got {apix}, {cutoff_res}")
    sigma = cutoff_res / (3.81 * apix) if cutoff_res > 2 * apix else 0.0
    taps = gaussian_taps(sigma) if sigma else None
    if mask_fraction_thresh > 0:
        mode, value = 1, float(mask_fraction_thresh)
    elif mask_thresh and mask_thresh > 0:
        mode, value = 2, float(mask_thresh)
    elif mask_mass > 0:
        mode, value = 3, float(min(int(mask_mass * 1e3 / (0.81 * apix**3)), n_voxels - 1))
    else:
        mode, value = 0, 0.0
    if not math.isfinite(value):
        raise ValueError(f"{name}: the threshold argument is NaN or infinite")
    return sigma, taps, mode, value


def _info(row):
    out = {k: (float(v) if k in ("threshold", "min", "max", "v_star") else int(v)) for k, v in zip(_INFO_KEYS, row)}
    out["fallback"] = bool(int(row[7]) & 1)
    out["ties_at_v_star"] = bool(int(row[7]) & 2)
    return out


def adaptive_mask_device(volume, apix, cutoff_res, mask_fraction_thresh=0, mask_thresh=0, mask_mass=0, *, device=0, info=False):
    """``adaptive_mask(volume.astype(float64), ...)`` on the device, uint8 0 / 1: the float64 Gaussian, the threshold (a
    fraction of the maximum, a value, the mass, or Otsu's on ``np.linspace``'s edges), the 26-connected components of the
    voxels above it that hold a seed; without such a component, every voxel above it.  Seeds: EVERY voxel ``>= v*``, the
    1000th largest value.  ``info=True``: ``(mask, dict)`` with ``threshold``, ``min``, ``max``, ``v_star``, ``above``, ``kept``,
    ``components``, ``fallback``, ``ties_at_v_star``."""
    v, is_f64 = _volume(volume, "adaptive_mask_device", _N_SEEDS)
    sigma, taps, mode, value = _mask_mode(v.size, apix, cutoff_res, mask_fraction_thresh, mask_thresh, mask_mass, "adaptive_mask_device")
    if mode == 0 and v.min() == v.max():
        raise ValueError("adaptive_mask_device: a constant volume has no Otsu threshold")
    out = np.empty(v.shape, dtype=np.uint8)
    row = np.zeros(8, dtype=np.float64)
    nz, ny, nx = v.shape
    _lib.check(_lib.lib().hh_am_mask_3d(int(device), v.ctypes.data_as(C.c_void_p), 1 if is_f64 else 0, nz, ny, nx, sigma,
                                        taps.ctypes.data_as(_f64p) if taps is not None else None, mode, value, out.ctypes.data_as(_u8p),
                                        row.ctypes.data_as(_f64p)), None)
    return (out, _info(row)) if info else out


# ------------------------------------------------------------------------------------------
# the resident context
# ------------------------------------------------------------------------------------------
def _cube(a, name):
    a = np.asarray(a)
    if a.ndim != 3 or len(set(a.shape)) != 1:
        raise ValueError(f"{name}: a cubic map (n x n x n) is needed; got {a.shape}")
    n = a.shape[0]
    if n % 2:
        raise ValueError(f"{name}: the side must be even; got {n} (the reference's irfftn returns n - 1 voxels along x there)")
    if n < _MIN_SIDE or n > _MAX_SIDE:
        raise ValueError(f"{name}: the side must lie in [{_MIN_SIDE}, {_MAX_SIDE}]; got {n}")
    return a


def _angles(p, n, name):
    p = np.ascontiguousarray(p, dtype=np.float64)
    if p.shape != (n, n, n // 2 + 1):
        raise ValueError(f"{name}: the angles must have the half spectrum's shape {(n, n, n // 2 + 1)}; got {p.shape}")
    if not np.isfinite(p).all():
        raise ValueError(f"{name}: the angles hold NaN or infinite values")
    return p


class _Context:
    """``hh_tfsc``: two maps, their randomised versions and the stored half spectra on the device."""

    def __init__(self, map1, map2, m_cut, phases1, phases2, seed, device):
        self.n = int(map1.shape[0])
        self._h = C.c_void_p()
        p1 = phases1.ctypes.data_as(_f64p) if phases1 is not None else None
        p2 = phases2.ctypes.data_as(_f64p) if phases2 is not None else None
        _lib.check(_lib.lib().hh_tfsc_create(C.byref(self._h), int(device), map1.ctypes.data_as(_f32p), map2.ctypes.data_as(_f32p),
                                             self.n, int(m_cut), p1, p2, int(seed) & (2**64 - 1)), None)

    def curves(self):
        sums = np.empty((2, self.n // 2 + 1, 3), dtype=np.float64)
        _lib.check(_lib.lib().hh_tfsc_curves(self._h, sums.ctypes.data_as(_f64p)), None)
        return sums

    def download(self, which, want_map=True, want_spec=False):
        n = self.n
        vol = np.empty((n, n, n), dtype=np.float32) if want_map else None
        spec = np.empty((n, n, n // 2 + 1), dtype=np.complex64) if want_spec else None
        _lib.check(_lib.lib().hh_tfsc_download(self._h, int(which), vol.ctypes.data_as(_f32p) if want_map else None,
                                               spec.ctypes.data_as(_f32p) if want_spec else None), None)
        return vol, spec

    def masked(self, masks1, masks2, full_spectrum):
        batch = masks1.shape[0]
        sums = np.empty((batch, 2, self.n // 2 + 1, 3), dtype=np.float64)
        ms = C.c_double(0.0)
        _lib.check(_lib.lib().hh_tfsc_masked(self._h, masks1.ctypes.data_as(_f32p), masks2.ctypes.data_as(_f32p) if masks2 is not None else None,
                                             batch, 1 if full_spectrum else 0, sums.ctypes.data_as(_f64p), C.byref(ms)), None)
        return sums, ms.value

    def set_support(self, sup1, sup2):
        _lib.check(_lib.lib().hh_tfsm_set_support(self._h, sup1.ctypes.data_as(_u8p), sup2.ctypes.data_as(_u8p) if sup2 is not None else None), None)

    def adaptive_support(self, one_mask, sigma, taps, mode, value):
        info = np.zeros((2, 8), dtype=np.float64)
        _lib.check(_lib.lib().hh_am_context_support(self._h, 1 if one_mask else 0, float(sigma), taps.ctypes.data_as(_f64p) if taps is not None else None,
                                                    int(mode), float(value), info.ctypes.data_as(_f64p)), None)
        return info

    def get_support(self, which):
        out = np.empty((self.n,) * 3, dtype=np.uint8)
        _lib.check(_lib.lib().hh_am_context_get_support(self._h, int(which), out.ctypes.data_as(_u8p)), None)
        return out

    def soft_mask(self, which, width):
        out = np.empty((self.n,) * 3, dtype=np.float32)
        _lib.check(_lib.lib().hh_tfsm_soft_mask(self._h, int(which), float(width), out.ctypes.data_as(_f32p)), None)
        return out

    def soft_masked(self, widths, full_spectrum):
        sums = np.empty((len(widths), 2, self.n // 2 + 1, 3), dtype=np.float64)
        ms = C.c_double(0.0)
        _lib.check(_lib.lib().hh_tfsm_soft_masked(self._h, widths.ctypes.data_as(_f64p), len(widths), 1 if full_spectrum else 0,
                                                  sums.ctypes.data_as(_f64p), C.byref(ms)), None)
        return sums, ms.value

    def close(self):
        if self._h:
            _lib.lib().hh_tfsc_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _draw(n):
    return np.random.uniform(0, 2 * np.pi, size=(n, n, n // 2 + 1))   # filters.py:512: the reference's draw, from the same stream


def randomize_phases_lowpass(data, apix, cutoff_res, return_fft=False, *, phases=None, seed=None, device=0):
    """filters.py:469-520 on the device: the map (float32 ``[n, n, n]``) whose Fourier phases at spatial frequencies
    ``>= apix / cutoff_res`` cycles per pixel are random and whose amplitudes are the input's, or with ``return_fft`` its
    ``rfftn`` half spectrum (complex64 ``[n, n, n // 2 + 1]``).  ``phases``: the angles (radians, the half spectrum's
    shape); ``seed``: the device's counter-based generator; neither: ``np.random.uniform(0, 2 pi, ...)`` drawn here exactly as
    the reference draws it.  Below the cutoff the bins are the transform's own.  Ties (a bin exactly on the cutoff) follow
    ``cutoff_m``, not the reference's float64 rounding; odd sides raise ``ValueError``."""
    a = _f32(_cube(data, "randomize_phases_lowpass"), "randomize_phases_lowpass")
    n = a.shape[0]
    if phases is not None and seed is not None:
        raise ValueError("randomize_phases_lowpass: give phases or seed, not both")
    if seed is None:
        phases = _angles(_draw(n) if phases is None else phases, n, "randomize_phases_lowpass")
    ctx = _Context(a, a, cutoff_m(n, apix, cutoff_res), phases, phases, 0 if seed is None else seed, device)
    try:
        vol, spec = ctx.download(0, want_map=not return_fft, want_spec=bool(return_fft))
    finally:
        ctx.close()
    return spec if return_fft else vol


class TrueFSC:
    """Two half maps and their phase-randomised versions, resident on the device.

    ``cutoff_res > 2`` is taken as it is; otherwise the cutoff follows ``choose_cutoff`` on the unmasked curve (one extra
    ``calc_fsc`` of the two maps).  ``phases=(angles1, angles2)`` or ``seed=`` as in ``randomize_phases_lowpass``; neither:
    two host draws, map 1 first, as the reference makes them.

    Attributes: ``cutoff_res``, ``cutoff_index = int(n apix / cutoff_res)``, ``unmasked`` and ``randomized_unmasked``
    (``[saxis, fsc]`` rows as ``calc_fsc`` returns them; the first equals ``calc_fsc(map1, map2, apix)`` bit for bit)."""

    def __init__(self, map1, map2, apix, cutoff_res=0, *, phases=None, seed=None, device=0):
        a, b = _cube(map1, "TrueFSC"), _cube(map2, "TrueFSC")
        if a.shape != b.shape:
            raise ValueError(f"TrueFSC: the two maps must have one shape; got {a.shape} and {b.shape}")
        a, b = _f32(a, "TrueFSC"), _f32(b, "TrueFSC")
        if phases is not None and seed is not None:
            raise ValueError("TrueFSC: give phases or seed, not both")
        self.n, self.apix, self.device = int(a.shape[0]), float(apix), int(device)
        n = self.n
        if not cutoff_res > 2:
            rows = calc_fsc(a, b, self.apix, device=device)
            cutoff_res = choose_cutoff(rows[:, 0], rows[:, 1], cutoff_res)
        self.cutoff_res = float(cutoff_res)
        self.cutoff_index = int(n * self.apix / self.cutoff_res)
        self.m_cut = cutoff_m(n, self.apix, self.cutoff_res)
        p1 = p2 = None
        if seed is None:
            if phases is None:
                p1 = _draw(n)
                p2 = _draw(n)
            else:
                p1, p2 = phases
            p1, p2 = _angles(p1, n, "TrueFSC"), _angles(p2, n, "TrueFSC")
        self._ctx = _Context(a, b, self.m_cut, p1, p2, 0 if seed is None else seed, device)
        self.sums = self._ctx.curves()
        self.unmasked = _fsc_rows(_ratio(self.sums[0]), n, self.apix)
        self.randomized_unmasked = _fsc_rows(_ratio(self.sums[1]), n, self.apix)
        self.kernel_ms = 0.0

    def close(self):
        self._ctx.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def randomized_map(self, which, return_fft=False):
        """The phase-randomised map 0 / 1 (float32), or its stored half spectrum (complex64)."""
        vol, spec = self._ctx.download(which, want_map=not return_fft, want_spec=bool(return_fft))
        return spec if return_fft else vol

    def _masks(self, m, name):
        m = np.asarray(m)
        want = (self.n,) * 3
        if m.ndim != 4 or m.shape[1:] != want or m.shape[0] < 1:
            raise ValueError(f"{name}: a stack of masks of the maps' shape {want} is needed ([B, n, n, n]); got {m.shape}")
        return _f32(m, name)

    def masked_sums(self, masks1, masks2=None, per_shell=False):
        """``[B, 2, n // 2 + 1, 3]``: ``num, den1, den2`` of ``(map1 m1, map2 m2)`` and of ``(map1r m1, map2r m2)`` for a stack
        of masks (``masks2=None``: one mask for both members)."""
        m1 = self._masks(masks1, "TrueFSC.masked_sums")
        m2 = None if masks2 is None else self._masks(masks2, "TrueFSC.masked_sums")
        if m2 is not None and m2.shape != m1.shape:
            raise ValueError(f"TrueFSC.masked_sums: the two stacks of masks must have one shape; got {m1.shape} and {m2.shape}")
        sums, self.kernel_ms = self._ctx.masked(m1, m2, bool(per_shell))
        return sums

    def _curves(self, sums, per_shell):
        fsc = _ratio(sums)
        if per_shell:
            return fsc
        return np.stack([_fsc_rows(f, self.n, self.apix) for f in fsc])

    def masked_batch(self, masks, per_shell=False):
        """``(fsc_t, fsc_n)`` for a stack of masks ``[B, n, n, n]``, each applied to both members: ``[B, rows, 2]`` each
        (``calc_fsc``'s rows), or ``[B, n // 2 + 1]`` with ``per_shell`` (``calc_fsc_per_shell``'s values).  Every curve is
        bit for bit the one the single call gives."""
        sums = self.masked_sums(masks, None, per_shell)
        return self._curves(sums[:, 0], per_shell), self._curves(sums[:, 1], per_shell)

    def masked(self, mask1, mask2=None, per_shell=False):
        """``(fsc_t, fsc_n)``: the FSC of ``(map1 mask1, map2 mask2)`` and of the phase-randomised maps under the same masks
        (``mask2=None``: ``mask1`` for both)."""
        want = (self.n,) * 3
        for m in (mask1, mask2):
            if m is not None and np.shape(m) != want:
                raise ValueError(f"TrueFSC.masked: a mask must have the maps' shape {want}; got {np.shape(m)}")
        sums = self.masked_sums(np.asarray(mask1)[None], None if mask2 is None else np.asarray(mask2)[None], per_shell)
        return self._curves(sums[:, 0], per_shell)[0], self._curves(sums[:, 1], per_shell)[0]

    # ---- soft masks built on the device from a resident support (csrc/soft_mask.inc)
    def set_support(self, support1, support2=None):
        """Upload the binary support(s) (nonzero = inside) the soft masks are built from: one for both members, or one each."""
        want = (self.n,) * 3
        s1 = _support(support1, "TrueFSC.set_support", want)
        s2 = None if support2 is None else _support(support2, "TrueFSC.set_support", want)
        self._supports = [s1] if s2 is None else [s1, s2]
        self._ctx.set_support(s1, s2)

    # ---- adaptive supports built on the device from the resident maps (csrc/adaptive_mask.inc)
    def adaptive_support(self, one_mask=False, mask_fraction_thresh=0, mask_thresh=0, mask_mass=0):
        """Build the support(s) on the device from the resident maps, as ``adaptive_mask`` defines them at this context's
        ``apix`` and ``cutoff_res`` (every voxel tied at the 1000th largest value is a seed): of the two maps' average for both
        members (``one_mask``), or one of each map.  They stay where ``set_support`` leaves them.  Returns the ``info`` dicts."""
        if self.n**3 < _N_SEEDS:
            raise ValueError(f"TrueFSC.adaptive_support: at least {_N_SEEDS} voxels are needed; the maps have {self.n**3}")
        sigma, taps, mode, value = _mask_mode(self.n**3, self.apix, self.cutoff_res, mask_fraction_thresh, mask_thresh, mask_mass,
                                              "TrueFSC.adaptive_support")
        self._supports = None                                    # a build that fails leaves no support behind
        rows = self._ctx.adaptive_support(bool(one_mask), sigma, taps, mode, value)
        self._supports = [self._ctx.get_support(k) for k in range(1 if one_mask else 2)]
        self.support_info = [_info(r) for r in rows[: len(self._supports)]]
        return self.support_info

    def support(self, which=0):
        """The support of member ``which`` (0 / 1) as it lies on the device: uint8 0 / 1."""
        if which not in (0, 1):
            raise ValueError(f"TrueFSC.support: which must be 0 or 1; got {which}")
        if not getattr(self, "_supports", None):
            raise ValueError("TrueFSC.support: no support is set (TrueFSC.set_support, TrueFSC.adaptive_support)")
        return self._ctx.get_support(which)

    def _widths(self, widths, name):
        if not getattr(self, "_supports", None):
            raise ValueError(f"{name}: no support is set (TrueFSC.set_support)")
        w = np.ascontiguousarray(widths, dtype=np.float64)
        if w.ndim != 1 or len(w) < 1:
            raise ValueError(f"{name}: a list of widths is needed; got an array of shape {w.shape}")
        if not np.isfinite(w).all():
            raise ValueError(f"{name}: the width of the soft edge is NaN or infinite")
        for step in sorted({soft_step(v) for v in w if v > 0}):
            for sup in self._supports:
                _not_empty(sup, step, name)
        return w

    def soft_mask(self, width, which=0):
        """The mask ``soft_masked(width)`` applies to member ``which`` (0 / 1), downloaded: float32 ``[n, n, n]``."""
        if which not in (0, 1):
            raise ValueError(f"TrueFSC.soft_mask: which must be 0 or 1; got {which}")
        w = self._widths([width], "TrueFSC.soft_mask")
        return self._ctx.soft_mask(which, w[0])

    def soft_masked_sums(self, widths, per_shell=False):
        """``masked_sums`` of the soft masks of these widths, built on the device: ``[B, 2, n // 2 + 1, 3]``."""
        w = self._widths(widths, "TrueFSC.soft_masked")
        sums, self.kernel_ms = self._ctx.soft_masked(w, bool(per_shell))
        return sums

    def soft_masked_batch(self, widths, per_shell=False):
        """``masked_batch`` of the supports' soft masks, one per width, none of them uploaded.  Every curve is bit for bit the
        one ``masked(soft_mask(width, 0), soft_mask(width, 1))`` gives, whatever the list and the width's place in it."""
        sums = self.soft_masked_sums(widths, per_shell)
        return self._curves(sums[:, 0], per_shell), self._curves(sums[:, 1], per_shell)

    def soft_masked(self, width, per_shell=False):
        """``(fsc_t, fsc_n)`` under the supports' soft masks of this width, as ``masked`` returns them."""
        sums = self.soft_masked_sums([width], per_shell)
        return self._curves(sums[:, 0], per_shell)[0], self._curves(sums[:, 1], per_shell)[0]

    def true_fsc(self, mask1, mask2=None):
        """trueFSC.py:342-348: ``[saxis, fsc_true]`` rows; ``fsc_t`` up to ``cutoff_index``, ``(fsc_t - fsc_n) / (1 - fsc_n)``
        beyond it, NaN -> 1.0."""
        t, nz = self.masked(mask1, mask2)
        return np.column_stack((t[:, 0], corrected(t[:, 1], nz[:, 1], self.cutoff_index)))


def corrected(fsc_t, fsc_n, cutoff_index):
    out = np.copy(fsc_t)
    i = cutoff_index + 1
    with np.errstate(divide="ignore", invalid="ignore"):
        out[i:] = (fsc_t[i:] - fsc_n[i:]) / (1 - fsc_n[i:])
    out[np.isnan(out)] = 1.0
    return out


def refine_score(fsc_t, fsc_n, cutoff_i):
    """trueFSC.py:223-234: the four-term score of one trial mask, from its two per-shell curves."""
    t, nz = fsc_t[cutoff_i:], fsc_n[cutoff_i:]
    with np.errstate(divide="ignore", invalid="ignore"):
        true = (t - nz) / (1 - nz)
    true[np.isnan(true)] = 1.0
    return (np.mean(1 - np.abs(true)) + np.mean(np.abs(nz)) + np.mean(np.abs(t - true)) + np.mean(1 - np.abs(true - nz)))


# ------------------------------------------------------------------------------------------
# the composition of trueFSC.py:main
# ------------------------------------------------------------------------------------------
def true_fsc(map1, map2, apix, *, mask=None, one_mask=False, cutoff_res=0, mask_soft=0, refine_mask=False, mask_fraction_thresh=0,
             mask_thresh=0, mask_mass=0, seed=None, phases=None, device=0, context=None, device_masks=False, device_support=False):
    """trueFSC.py:102-366.  ``mask``: one mask or a pair, used as given (a pair is averaged with ``one_mask``); without one, the
    adaptive mask of each map (of the maps' average with ``one_mask``) with a soft edge of ``mask_soft`` Angstrom, or of the
    width ``refine_mask`` finds (``minimize_scalar``, bounded to ``(0, n / 3)`` pixels, ``xatol=2``, every evaluation one
    ``.masked(..., per_shell=True)`` call on the resident context), or of ``3 res_unmasked / apix`` pixels.  ``context``
    stands in for ``TrueFSC`` (tests).

    ``device_masks``: the adaptive supports go up once (``set_support``), every trial of ``refine_mask`` is one
    ``.soft_masked(x, per_shell=True)``, the final curves come from ``.soft_masked(soft_px)`` and ``mask1`` / ``mask2`` are
    the device's masks, downloaded (float32); ``host_mask_s`` then counts ``adaptive_mask`` alone.  Refused with ``mask=``:
    a given mask is used as it is, there is no support to soften.

    ``device_support`` (needs ``device_masks``): the adaptive supports are built on the device from the context's resident
    maps (``adaptive_support``) instead of ``adaptive_mask`` + ``set_support``; ``host_mask_s`` is then 0.0.  The maps must be
    exactly representable in float32, because the context holds float32 while the host path filters the caller's float64.

    Returns a dict: ``unmasked``, ``randomized_unmasked``, ``masked``, ``randomized_masked``, ``true`` (``[saxis, fsc]``
    rows), ``true_fit`` (500 rows), ``resolution`` (``unmasked``, ``masked``, ``true``, ``true_fit`` at 0.143),
    ``cutoff_res``, ``cutoff_index``, ``mask_soft_px`` (None with a given mask), ``mask1``, ``mask2``, ``host_mask_s`` (the seconds
    spent in the host's mask helpers)."""
    import time

    if device_masks and mask is not None:
        raise ValueError("true_fsc: device_masks builds the soft edge of the adaptive support; a given mask is used as it is")
    if device_support and not device_masks:
        raise ValueError("true_fsc: device_support needs device_masks=True (the supports stay on the device for the soft masks built there)")
    a64, b64 = np.asarray(map1, dtype=np.float64), np.asarray(map2, dtype=np.float64)
    if device_support and not all(np.array_equal(m.astype(np.float32), m) for m in (a64, b64)):
        raise ValueError("true_fsc: device_support needs maps that float32 represents exactly (the context holds float32; "
                         "the host's adaptive_mask filters the maps in float64)")
    ctx = (context or TrueFSC)(map1, map2, apix, cutoff_res, phases=phases, seed=seed, device=device)
    host_s = 0.0
    try:
        n = a64.shape[0]
        unmasked = ctx.unmasked
        res_unmasked = fsc_resolution(unmasked[:, 0], unmasked[:, 1], 0.143)
        cutoff = ctx.cutoff_res
        soft_px = None
        if mask is not None:
            masks = [np.asarray(m, dtype=np.float64) for m in (mask if isinstance(mask, (list, tuple)) else [mask])]
            if len(masks) not in (1, 2):
                raise ValueError("true_fsc: one mask or two")
            mask1, mask2 = masks[0], masks[-1]
            if len(masks) == 2 and one_mask:
                mask1 = mask2 = (mask1 + mask2) / 2
        else:
            kw = dict(mask_fraction_thresh=mask_fraction_thresh, mask_thresh=mask_thresh, mask_mass=mask_mass)
            if device_support:
                ctx.adaptive_support(one_mask=bool(one_mask), **kw)
                same = bool(one_mask)
            else:
                t0 = time.perf_counter()
                if one_mask:
                    mask1 = mask2 = adaptive_mask((a64 + b64) / 2, apix, cutoff, **kw)
                else:
                    mask1, mask2 = adaptive_mask(a64, apix, cutoff, **kw), adaptive_mask(b64, apix, cutoff, **kw)
                host_s += time.perf_counter() - t0
                same = mask2 is mask1
                if device_masks:
                    ctx.set_support(mask1, None if same else mask2)
            if mask_soft > 0:
                soft_px = mask_soft / apix
            elif refine_mask:
                from scipy.optimize import minimize_scalar

                def score(x):
                    nonlocal host_s
                    if device_masks:
                        fsc_t, fsc_n = ctx.soft_masked(x, per_shell=True)
                        return refine_score(fsc_t, fsc_n, ctx.cutoff_index + 2)
                    t0 = time.perf_counter()
                    trial = soft_mask(mask1, x)
                    host_s += time.perf_counter() - t0
                    fsc_t, fsc_n = ctx.masked(trial, None, per_shell=True)
                    return refine_score(fsc_t, fsc_n, ctx.cutoff_index + 2)

                soft_px = float(minimize_scalar(score, bounds=(0, n / 3), method="bounded", options={"xatol": 2}).x)
            else:
                soft_px = 3 * res_unmasked / apix
            if not device_masks:
                t0 = time.perf_counter()
                mask1 = soft_mask(mask1, soft_px)
                mask2 = mask1 if same else soft_mask(mask2, soft_px)
                host_s += time.perf_counter() - t0
        if device_masks:
            fsc_t, fsc_n = ctx.soft_masked(soft_px)
            mask1 = ctx.soft_mask(soft_px, 0)
            mask2 = mask1 if same else ctx.soft_mask(soft_px, 1)
        else:
            fsc_t, fsc_n = ctx.masked(mask1, None if mask2 is mask1 else mask2)
        true = np.column_stack((fsc_t[:, 0], corrected(fsc_t[:, 1], fsc_n[:, 1], ctx.cutoff_index)))
        s_fit, f_fit, _ = fit_fsc_curve(true[:, 0], true[:, 1])
        return {
            "unmasked": unmasked, "randomized_unmasked": ctx.randomized_unmasked, "masked": fsc_t, "randomized_masked": fsc_n,
            "true": true, "true_fit": np.column_stack((s_fit, f_fit)),
            "resolution": {"unmasked": res_unmasked, "masked": fsc_resolution(fsc_t[:, 0], fsc_t[:, 1], 0.143),
                           "true": fsc_resolution(true[:, 0], true[:, 1], 0.143), "true_fit": fsc_resolution(s_fit, f_fit, 0.143)},
            "cutoff_res": float(cutoff), "cutoff_index": int(ctx.cutoff_index), "mask_soft_px": soft_px,
            "mask1": mask1, "mask2": mask2, "host_mask_s": host_s,
        }
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------
# command line
# ------------------------------------------------------------------------------------------
def add_args(parser: argparse.ArgumentParser) -> argparse.ArgumentParser:
    parser.add_argument("half1", help=".mrc / .map / .npy file with one cubic 3-D map of even side")
    parser.add_argument("half2", help="the second map, of the same shape")
    parser.add_argument("--apix", type=float, default=None, help="voxel size, Angstrom (default: the first map's MRC header)")
    parser.add_argument("--mask", nargs="+", default=None, metavar="M", help="one mask file, or one per map; used as given")
    parser.add_argument("--one-mask", action="store_true", help="one mask for both maps (the average of two given masks, or the adaptive mask of the maps' average)")
    parser.add_argument("--cutoff-res", type=float, default=0.0, help="resolution (Angstrom) beyond which phases are randomised (default: FSC = 0.8 of the unmasked maps)")
    parser.add_argument("--mask-soft", type=float, default=0.0, help="width of the mask's soft edge, Angstrom (default: 3 x the unmasked resolution)")
    parser.add_argument("--refine-mask", action="store_true", help="search the soft edge's width (ignored with --mask-soft)")
    group = parser.add_mutually_exclusive_group()
    group.add_argument("--mask-fraction-thresh", type=float, default=0.0, help="mask threshold as a fraction of the low-passed map's maximum")
    group.add_argument("--mask-thresh", type=float, default=0.0, help="mask threshold, a voxel value")
    group.add_argument("--mask-mass", type=float, default=0.0, help="mask threshold from the structure's mass, kDa")
    parser.add_argument("--seed", type=int, default=None, help="seed of the device's phase generator (default: NumPy's global stream, as the reference)")
    parser.add_argument("--out-prefix", default=None, help="write P.unmasked.txt ... P.true.fit.txt and the mask(s)")
    parser.add_argument("--device", type=int, default=0)
    parser.add_argument("--device-masks", action="store_true", help="build the soft edge of the adaptive mask, and every trial of --refine-mask, on the device (not with --mask)")
    parser.add_argument("--device-support", action="store_true", help="build the adaptive mask itself on the device from the resident maps (needs --device-masks)")
    return parser


def run(args, context=None) -> dict:
    """``context`` stands in for ``TrueFSC`` (tests): everything else, the masks included, runs as it does on a device."""
    if getattr(args, "device_support", False) and not getattr(args, "device_masks", False):
        raise SystemExit("--device-support needs --device-masks")
    m1, apix = _read_map(args.half1, args.apix)
    m2, _ = _read_map(args.half2, args.apix)
    if not apix or apix <= 0:
        raise SystemExit("--apix is required (the maps carry no voxel size)")
    if m1.ndim != 3 or len(set(m1.shape)) != 1 or m1.shape != m2.shape:
        raise SystemExit(f"two cubic maps of one shape are needed; got {tuple(m1.shape)} and {tuple(m2.shape)}")
    n = int(m1.shape[0])
    if n % 2 or n < _MIN_SIDE or n > _MAX_SIDE:
        raise SystemExit(f"the side of the maps must be even and lie in [{_MIN_SIDE}, {_MAX_SIDE}]; got {n}")
    mask = None
    if args.mask:
        if len(args.mask) > 2:
            raise SystemExit("--mask takes one file or two")
        mask = [_read_map(p)[0] for p in args.mask]
        if any(m.shape != m1.shape for m in mask):
            raise SystemExit(f"a mask must have the maps' shape {tuple(m1.shape)}")
    try:
        out = true_fsc(m1, m2, float(apix), mask=mask, one_mask=args.one_mask, cutoff_res=args.cutoff_res, mask_soft=args.mask_soft,
                       refine_mask=args.refine_mask and not args.mask_soft > 0, mask_fraction_thresh=args.mask_fraction_thresh,
                       mask_thresh=args.mask_thresh, mask_mass=args.mask_mass, seed=args.seed, device=args.device, context=context,
                       device_masks=getattr(args, "device_masks", False), device_support=getattr(args, "device_support", False))
    except ValueError as e:
        raise SystemExit(str(e))
    curves = ("unmasked", "randomized_unmasked", "masked", "randomized_masked", "true")
    report = {
        "maps": dict(half1=str(args.half1), half2=str(args.half2), shape=[int(v) for v in m1.shape], apix=float(apix)),
        "cutoff_res": out["cutoff_res"], "cutoff_index": out["cutoff_index"], "mask_soft_px": out["mask_soft_px"],
        "saxis": [float(v) for v in out["unmasked"][:, 0]],
        **{k: [float(v) for v in out[k][:, 1]] for k in curves},
        "resolution": {k: float(v) for k, v in out["resolution"].items()},
    }
    if args.out_prefix:
        p = str(args.out_prefix)
        for k in curves:   # the reference's files: the shells from 1 on
            np.savetxt(f"{p}.{k.replace('_', '-')}.txt", out[k][1:])
        np.savetxt(f"{p}.true.fit.txt", out["true_fit"])
        from .mrc import write_mrc

        if out["mask2"] is out["mask1"]:
            write_mrc(f"{p}.common_mask.mrc", out["mask1"].astype(np.float32), float(apix))
        else:
            write_mrc(f"{p}.mask1.mrc", out["mask1"].astype(np.float32), float(apix))
            write_mrc(f"{p}.mask2.mrc", out["mask2"].astype(np.float32), float(apix))
    return report


def main(argv=None) -> int:
    args = add_args(argparse.ArgumentParser(prog="helicon_amd.true_fsc", description=__doc__.split("\n\n")[0])).parse_args(argv)
    json.dump(run(args), sys.stdout, indent=1)
    sys.stdout.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
