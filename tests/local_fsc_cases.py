"""Float64 yardstick of the local resolution map (helicon_amd/local_resolution.py, csrc/local_resolution.inc), the table of
the GPU cases and their generator.  Only NumPy; the package under test is not imported.  The rules, each a restatement of one
of the reference's:

  centres     step // 2 + i step <= N - 1 along every axis
  window      the w^3 clip around a centre, corner c - w // 2, zeros outside the map (lib/transforms.py:516-555)
  taper       one axis of generate_tapering_filter (lib/filters.py:415-466) for a length w, t[z] t[y] t[x]
  curve       fsc_oracle.sums_3d(..., True) and fsc_oracle.ratio: calc_fsc_per_shell (lib/analysis.py:235-290)
  resolution  the first shell k >= 1 below the threshold, linear interpolation with the shell before
              (commands/trueFSC.py:427-462); Nyquist when there is none, w apix when it is shell 1
  map         trilinear between the centres, NaN corners dropped, the other weights renormalised

The keyword arguments of `local_fsc` that default to the rule switch in the WRONG variants whose effect
tests/test_local_fsc_host.py measures."""
import functools

import numpy as np

import fsc_oracle as O

APIX, SEED = 1.5, 7
THRESHOLDS = (0.5, 0.143)
NEAR = 1e-4          # a window with a shell k >= 1 this close to the threshold is left out of the resolution comparison
MAX_EXCLUDED = 0.02  # at most this share of a case's windows
# The curve bound of the GPU tests, per route: the largest |curve - yardstick| measured on an MI355X over the cases of this
# table (profiles/local_fsc.json, "accuracy": 1.453e-7 on the LDS route, at (13, 11, 14) with w = 8; 1.052e-7 on the passes route, at
# (24, 24, 32) with w = 8; the special inputs of tests/test_gpu_local_fsc.py stay below both) times 4.
TOL_CURVE = {"lds": 4 * 1.453e-7, "passes": 4 * 1.052e-7}

# (shape, window, step)
LDS_CASES = tuple(((w + 5, w + 3, w + 6), w, w // 2) for w in range(8, 25, 2))
PASSES_CASES = tuple(((w + 5, w + 3, w + 6), w, w // 2) for w in (8, 24, 26, 32)) + (((66, 64, 70), 64, 32),)
BOTH_CASES = (((24, 24, 32), 8, 4), ((32, 32, 32), 16, 8))
ALL_CASES = tuple(dict.fromkeys(LDS_CASES + PASSES_CASES + BOTH_CASES))


@functools.lru_cache(maxsize=None)
def make_halves(shape, seed=SEED):
    """Two float32 half maps: 40 Gaussian blobs (centres uniform in +-0.4 of each side around the middle, sigma in
    U(0.8, 2.0), amplitude in U(0.5, 1.5)) plus, on each half, independent white noise of standard deviation
    0.02 + 0.6 r^2, r the distance from the z axis over min(ny, nx) / 2: the floor keeps every shell's power within float32's
    reach of the DC shell, the ramp makes the resolution vary across the map."""
    rng = np.random.default_rng(seed)
    shape = tuple(int(v) for v in shape)
    size = np.asarray(shape, dtype=np.float64)
    centres = rng.uniform(-0.4, 0.4, (40, 3)) * size + size / 2.0
    sigma = rng.uniform(0.8, 2.0, 40)
    amp = rng.uniform(0.5, 1.5, 40)
    ax = [np.arange(n, dtype=np.float64) for n in shape]
    signal = np.zeros(shape)
    for c, s, a in zip(centres, sigma, amp):
        gz, gy, gx = (np.exp(-0.5 * ((ax[d] - c[d]) / s) ** 2) for d in range(3))
        signal += a * gz[:, None, None] * gy[None, :, None] * gx[None, None, :]
    r2 = ((ax[1][:, None] - shape[1] / 2.0) ** 2 + (ax[2][None, :] - shape[2] / 2.0) ** 2) / (min(shape[1], shape[2]) / 2.0) ** 2
    sd = (0.02 + 0.6 * r2)[None, :, :]
    h1 = (signal + sd * rng.standard_normal(shape)).astype(np.float32)
    h2 = (signal + sd * rng.standard_normal(shape)).astype(np.float32)
    h1.setflags(write=False)
    h2.setflags(write=False)
    return h1, h2


def window_centres(n, step):
    return np.arange(step // 2, n, step)


def taper_profile(w, fraction_start=0.5, fraction_slope=0.5):
    if not (0 < fraction_start < 1):
        return np.ones(w, dtype=np.float32)
    t = np.abs((np.arange(0, w, dtype=np.float32) - w // 2) / (w // 2))
    inner, outer = t < fraction_start, t > fraction_start + fraction_slope
    t = (1.0 + np.cos((t - fraction_start) / fraction_slope * np.pi)) / 2.0
    t[inner] = 1
    t[outer] = 0
    return t


def clip(data, corner, w, pad="zero"):
    """The w^3 block whose first voxel is `corner`; outside the map zeros (or, the wrong variant, the nearest voxel)."""
    if pad == "edge":
        idx = [np.clip(np.arange(c, c + w), 0, n - 1) for c, n in zip(corner, data.shape)]
        return data[np.ix_(*idx)].astype(np.float64)
    out = np.zeros((w, w, w), dtype=np.float64)
    src, dst = [], []
    for c, n in zip(corner, data.shape):
        lo, hi = max(c, 0), min(c + w, n)
        src.append(slice(lo, hi))
        dst.append(slice(lo - c, hi - c))
    out[tuple(dst)] = data[tuple(src)]
    return out


def resolution_from_curve(fsc, w, apix, threshold, first_shell=1):
    """(resolution, branch, k*): branch "nyquist" (k* = -1), "first" (k* = 1) or "interp"."""
    saxis = np.arange(w // 2 + 1) / (w * apix)
    below = [k for k in range(first_shell, w // 2 + 1) if fsc[k] < threshold]
    if not below:
        return 1.0 / saxis[w // 2], "nyquist", -1
    k = below[0]
    if k <= 1:
        return w * apix, "first", k
    x = saxis[k - 1] + (threshold - fsc[k - 1]) * (saxis[k] - saxis[k - 1]) / (fsc[k] - fsc[k - 1])
    return 1.0 / x, "interp", k


def local_fsc(h1, h2, apix, w, step, threshold=0.5, taper=(0.5, 0.5), mask=None, *, corner_shift=0, full=True, first_shell=1, pad="zero"):
    """dict: centres (three arrays), curves [gz, gy, gx, w // 2 + 1], resolution [gz, gy, gx], branch and kstar of the same grid;
    NaN / "" / 0 where the mask leaves a window out."""
    axes = [window_centres(n, step) for n in h1.shape]
    grid = tuple(len(a) for a in axes)
    t = taper_profile(w, *taper).astype(np.float64)
    t3 = t[:, None, None] * t[None, :, None] * t[None, None, :]
    curves = np.full(grid + (w // 2 + 1,), np.nan)
    res = np.full(grid, np.nan)
    branch = np.full(grid, "", dtype=object)
    kstar = np.zeros(grid, dtype=np.int64)
    for i, cz in enumerate(axes[0]):
        for j, cy in enumerate(axes[1]):
            for k, cx in enumerate(axes[2]):
                if mask is not None and not mask[cz, cy, cx]:
                    continue
                corner = (cz - w // 2 + corner_shift, cy - w // 2 + corner_shift, cx - w // 2 + corner_shift)
                a, b = clip(h1, corner, w, pad) * t3, clip(h2, corner, w, pad) * t3
                f = O.ratio(O.sums_3d(a, b, full))
                curves[i, j, k] = f
                res[i, j, k], branch[i, j, k], kstar[i, j, k] = resolution_from_curve(f, w, apix, threshold, first_shell)
    return dict(centres=axes, curves=curves, resolution=res, branch=branch, kstar=kstar)


@functools.lru_cache(maxsize=None)
def case(shape, w, step, threshold=0.5):
    """The yardstick of one case of the table on make_halves(shape), computed once per session."""
    h1, h2 = make_halves(shape)
    return local_fsc(h1, h2, APIX, w, step, threshold)


def near_threshold(curves, threshold, near=NEAR):
    """Per window: does any shell k >= 1 lie within `near` of the threshold?"""
    return (np.abs(curves[..., 1:] - threshold) < near).any(axis=-1)


def upsample(grid, step, shape):
    """The full-size float64 map of a grid of window values: per axis u = clip((p - step // 2) / step, 0, g - 1),
    i0 = min(floor(u), g - 2) (g == 1: that one corner with weight 1); NaN corners dropped, the other weights renormalised,
    NaN where the remaining weights sum to 0."""
    grid = np.asarray(grid, dtype=np.float64)
    idx, frac = [], []
    for n, g in zip(shape, grid.shape):
        if g == 1:
            idx.append(np.zeros(n, dtype=np.int64))
            frac.append(np.zeros(n))
            continue
        u = np.clip((np.arange(n, dtype=np.float64) - step // 2) / step, 0, g - 1)
        i0 = np.minimum(np.floor(u).astype(np.int64), g - 2)
        idx.append(i0)
        frac.append(u - i0)
    acc, wsum = np.zeros(shape), np.zeros(shape)
    for dz in range(1 if grid.shape[0] == 1 else 2):
        for dy in range(1 if grid.shape[1] == 1 else 2):
            for dx in range(1 if grid.shape[2] == 1 else 2):
                v = grid[np.ix_(idx[0] + dz, idx[1] + dy, idx[2] + dx)]
                wz, wy, wx = (f if d else 1.0 - f for f, d in zip(frac, (dz, dy, dx)))
                wt = wz[:, None, None] * wy[None, :, None] * wx[None, None, :]
                ok = ~np.isnan(v)
                acc += np.where(ok, wt * v, 0.0)
                wsum += np.where(ok, wt, 0.0)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(wsum > 0, acc / wsum, np.nan)
