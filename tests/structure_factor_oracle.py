"""NumPy restatement of the reference's structure-factor functions (lib/filters.py:22-208: calculate_structural_factor,
set_structural_factors, match_structural_factors), in float64 whatever the input's dtype: the yardstick of
tests/test_gpu_structure_factor.py, itself pinned to the reference's recorded output by
tests/golden/g24_structure_factor.npz (tests/test_structure_factor_host.py).  Only NumPy and SciPy; the package under test is
not imported.

`rule` switches ONE step to a plausible wrong rule (WRONG_RULES), so that the host tests can show that the GPU tests' probes
notice each of them.  Also here: the case lists of the fixture and of the GPU tests, their input recipe, and the tie census
(voxels whose radius equals a bin edge in exact arithmetic, with the reference's float64 verdict)."""
from fractions import Fraction
from math import isqrt, lcm

import numpy as np

WRONG_RULES = ("left", "fsc_shell", "qstep_width", "closed_last", "exact_ties", "keep_above", "masked_spectrum")

# (shape, apix) of the fixture, in its order
FIXTURE_CASES = [((8, 8, 8), 1.0), ((8, 8, 8), 0.83), ((9, 9, 9), 1.0), ((9, 9, 9), 1.7), ((9, 9, 9), 5.0), ((15, 18, 21), 1.7),
                 ((12, 20, 36), 1.1), ((24, 20), 1.5), ((33, 47), 2.2)]
# what the impulse probe adds to them
IMPULSE_EXTRA = [((16, 16, 16), 1.3), ((16, 16, 16), 0.9), ((4, 4, 4), 1.0), ((2, 2, 8), 1.0), ((8, 8), 1.0), ((66, 70, 130), 1.2)]
VARIANTS = ("plain", "mask", "thresh", "both")
TARGET_APIX_FACTOR = 1.25      # apix_target = 1.25 apix in the fixture: never the data's own
THRESH, THRESH_TARGET = 0.75, 0.5


def radius(shape, apix):
    """qr on the full grid, the reference's expression (filters.py:61-79)."""
    if len(shape) == 2:
        qy, qx = np.meshgrid(np.fft.fftfreq(shape[0]), np.fft.fftfreq(shape[1]), indexing="ij")
        return np.sqrt(qx**2 + qy**2) / apix
    qz, qy, qx = np.meshgrid(np.fft.fftfreq(shape[0]), np.fft.fftfreq(shape[1]), np.fft.fftfreq(shape[2]), indexing="ij")
    return np.sqrt(qx**2 + qy**2 + qz**2) / apix


def bins(shape, apix):
    """(qbins, qstep, qr): filters.py:81-85."""
    qr = radius(shape, apix)
    qmax = np.max(qr)
    qstep = np.min(qr[qr > 0])
    nbins = int(qmax / qstep) // 2 * 2
    return np.linspace(0, nbins * qstep, nbins), qstep, qr


def tie_voxels(shape, apix):
    """[(index, edge, verdict)]: the voxels whose radius equals a bin edge i >= 1 in EXACT arithmetic,
    sum (k_a / n_a)^2 = (i nbins / ((nbins - 1) L))^2 with L the longest side (apix cancels), and what the reference's float64
    comparison makes of them: "at" (qr == qbins[i]), "below" or "above"."""
    qbins, _, qr = bins(shape, apix)
    nbins, L = len(qbins), max(shape)
    m = lcm(*[n * n for n in shape])
    out = []
    for idx in np.ndindex(*shape):
        k = [min(i, n - i) for i, n in zip(idx, shape)]
        lhs = sum(kk * kk * (m // (n * n)) for kk, n in zip(k, shape))       # m sum (k / n)^2, an integer
        # i^2 = lhs (nbins - 1)^2 L^2 / (m nbins^2)
        f = Fraction(lhs * (nbins - 1) ** 2 * L * L, m * nbins * nbins)
        if f.denominator != 1 or f.numerator == 0:
            continue
        i = isqrt(f.numerator)
        if i * i != f.numerator or i > nbins - 1:
            continue
        q, e = qr[idx], qbins[i]
        out.append((idx, i, "at" if q == e else ("below" if q < e else "above")))
    return out


def labels(shape, apix, rule=None):
    """searchsorted(qbins, qr, "right") - 1 (filters.py:86); -1 marks a voxel that a wrong rule leaves out."""
    qbins, qstep, qr = bins(shape, apix)
    nbins = len(qbins)
    if rule == "left":
        return np.searchsorted(qbins, qr, "left") - 1
    if rule == "fsc_shell":
        return np.clip(np.round(qr / qstep).astype(np.int64), 0, nbins - 1)
    if rule == "qstep_width":
        return np.clip(np.searchsorted(np.arange(nbins) * qstep, qr, "right") - 1, 0, nbins - 1)
    lab = np.searchsorted(qbins, qr, "right") - 1
    if rule == "closed_last":
        lab = np.where(qr > qbins[-1], -1, lab)
    if rule == "exact_ties":
        for idx, i, _ in tie_voxels(shape, apix):
            lab[idx] = i
    return lab


def counts(shape, apix, rule=None):
    """voxels per bin: what the profile of a unit impulse must round to."""
    lab = labels(shape, apix, rule)
    return np.bincount(lab[lab >= 0].ravel(), minlength=len(bins(shape, apix)[0]))


def threshold_data(data, thresh):
    return np.clip(data, thresh, None) - thresh


def calculate_structural_factor(data, apix, thresh=None, mask=None, return_fft=False, rule=None):
    work = np.asarray(data, dtype=np.float64)
    if thresh:
        work = threshold_data(work, thresh)
    if mask is not None:
        work = work * np.asarray(mask, dtype=np.float64)
    F = np.fft.fftn(work)
    power = F.real**2 + F.imag**2
    qbins = bins(work.shape, apix)[0]
    lab = labels(work.shape, apix, rule)
    sf = np.bincount(lab[lab >= 0].ravel(), weights=power[lab >= 0].ravel(), minlength=len(qbins))
    return (qbins, sf, F) if return_fft else (qbins, sf)


def ratio_on_grid(qbins, ratio, qr, rule=None):
    """interp1d(qbins, ratio, bounds_error=False, fill_value=0)(qr)"""
    from scipy import interpolate

    if rule == "keep_above":
        return interpolate.interp1d(qbins, ratio, bounds_error=False, fill_value=(0, ratio[-1]))(qr)
    return interpolate.interp1d(qbins, ratio, bounds_error=False, fill_value=0)(qr)


def set_structural_factors(data, apix, target_bins, target_sf, thresh=None, mask=None, rule=None):
    from scipy import interpolate

    data = np.asarray(data, dtype=np.float64)
    qbins, sf, fft = calculate_structural_factor(data, apix, thresh=thresh, mask=mask, return_fft=True, rule=rule)
    if mask is not None and rule != "masked_spectrum":
        fft = np.fft.fftn(data)
    target = interpolate.interp1d(target_bins, target_sf, bounds_error=False, fill_value=0)(qbins)
    ratio = np.zeros_like(sf)
    nz = np.nonzero(sf)
    ratio[nz] = np.sqrt(target[nz] / sf[nz])
    qr = bins(data.shape, apix)[2]
    if rule == "exact_ties":   # a tie that float64 puts above the last edge stays inside
        qr = qr.copy()
        for idx, i, _ in tie_voxels(data.shape, apix):
            qr[idx] = qbins[i]
    return np.real(np.fft.ifftn(fft * ratio_on_grid(qbins, ratio, qr, rule)))


def match_structural_factors(data, apix, data_target, apix_target, thresh=None, thresh_target=None, mask=None, rule=None):
    target_bins, target_sf = calculate_structural_factor(data_target, apix_target, thresh=thresh_target, mask=mask)
    return set_structural_factors(data, apix, target_bins, target_sf, thresh=thresh, mask=mask, rule=rule)


# ---------------------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------------------
def make_inputs(shape, seed, noise=1.0):
    """(data, target, mask): float32 values that float16 holds exactly.  data and target: tests/fsc_oracle.py's recipe (a smooth
    signal plus white noise, dc="auto": the noise floor keeps every bin's power per voxel within 1e-4 of the strongest) with
    the noise scaled by `noise`; mask: a smooth bump in [0, 1], off-centre."""
    from scipy.ndimage import gaussian_filter

    rng = np.random.default_rng(seed)
    shape = tuple(shape)
    offset = 1.0 / np.sqrt(min(shape))
    out = []
    for signal, sigma in ((8.0, 1.5), (5.0, 1.0)):
        v = gaussian_filter(rng.standard_normal(shape), sigma) * signal + noise * rng.standard_normal(shape) + offset
        if len(shape) == 2:
            v = v + offset * (1.0 - 2.0 * ((np.arange(shape[0])[:, None] + np.arange(shape[1])[None, :]) % 2))
        out.append(v.astype(np.float16).astype(np.float32))
    grids = np.meshgrid(*[(np.arange(n) - 0.45 * n) / (0.35 * n) for n in shape], indexing="ij")
    r = np.sqrt(sum(g * g for g in grids))
    mask = np.clip(1.25 - r, 0.0, 1.0).astype(np.float16).astype(np.float32)
    return out[0], out[1], mask


def floor_ratio(shape, apix, sf):
    """min over the bins of (mean power per voxel) / (the strongest bin's)."""
    c = counts(shape, apix)
    per = np.asarray(sf, dtype=np.float64)[c > 0] / c[c > 0]
    return float(per.min() / per.max())


def variant_args(variant, mask):
    """(thresh, thresh_target, mask) of a fixture variant."""
    return (THRESH if variant in ("thresh", "both") else None, THRESH_TARGET if variant in ("thresh", "both") else None,
            mask if variant in ("mask", "both") else None)


def case_key(k, variant):
    return f"c{k}_{variant}"
