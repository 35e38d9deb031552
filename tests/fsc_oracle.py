"""NumPy restatement of the reference's Fourier shell / ring correlation (lib/analysis.py:116-484), in float64 whatever the
input's dtype: the yardstick of tests/test_gpu_fsc.py, itself pinned to the reference's recorded output by
tests/golden/g19_fsc.npz (tests/test_fsc_host.py).  Only NumPy and SciPy; the package under test is not imported."""
import numpy as np


def shell_3d_half(n):
    """clip(round(|k| n), 0, n // 2) on the rfftn half spectrum [n, n, n // 2 + 1] (analysis.py:146-151)."""
    k2, kr2 = np.fft.fftfreq(n) ** 2, np.fft.rfftfreq(n) ** 2
    s = np.round(np.sqrt(k2[:, None, None] + k2[None, :, None] + kr2[None, None, :]) * n).astype(np.int32)
    return np.clip(s, 0, n // 2)


def shell_3d_full(n):
    """the same on the full spectrum (analysis.py:264-270)."""
    k = np.fft.fftfreq(n)
    kx, ky, kz = np.meshgrid(k, k, k, indexing="ij")
    s = np.round(np.sqrt(kx**2 + ky**2 + kz**2) * n).astype(np.int32)
    return np.clip(s, 0, n // 2)


def shell_2d(h, w):
    """analysis.py:322-335."""
    n_shells = min(h, w) // 2
    kr = np.sqrt((np.fft.fftfreq(h) ** 2)[:, None] + (np.fft.fftfreq(w) ** 2)[None, :])
    return np.clip(np.round(kr * n_shells).astype(np.int32), 0, n_shells), n_shells


def shell_sums(f1, f2, shell, n_bins):
    """[n_bins, 3] float64: num, den1, den2."""
    s = shell.ravel()
    return np.stack([np.bincount(s, weights=np.real(f1 * np.conj(f2)).ravel(), minlength=n_bins),
                     np.bincount(s, weights=(np.abs(f1) ** 2).ravel(), minlength=n_bins),
                     np.bincount(s, weights=(np.abs(f2) ** 2).ravel(), minlength=n_bins)], axis=1)


def ratio(sums):
    denom = np.sqrt(sums[:, 1] * sums[:, 2])
    fsc = np.ones(len(sums))
    ok = denom > 0
    fsc[ok] = sums[ok, 0] / denom[ok]
    return fsc


def sums_3d(map1, map2, full=False):
    a, b = np.asarray(map1, dtype=np.float64), np.asarray(map2, dtype=np.float64)
    n = a.shape[0]
    if full:
        return shell_sums(np.fft.fftn(a), np.fft.fftn(b), shell_3d_full(n), n // 2 + 1)
    return shell_sums(np.fft.rfftn(a), np.fft.rfftn(b), shell_3d_half(n), n // 2 + 1)


def calc_fsc(map1, map2, apix):
    n = np.asarray(map1).shape[0]
    fsc = ratio(sums_3d(map1, map2, False))
    saxis = np.arange(n // 2 + 1) * (1.0 / (apix * n))
    keep = np.where(saxis <= np.fft.rfftfreq(n).max())
    return np.vstack((saxis[keep], fsc[keep])).T


def calc_fsc_per_shell(map1, map2, apix):
    return ratio(sums_3d(map1, map2, True))


def sums_2d(img1, img2):
    a, b = np.asarray(img1, dtype=np.float64), np.asarray(img2, dtype=np.float64)
    shell, n_shells = shell_2d(*a.shape)
    return shell_sums(np.fft.fft2(a), np.fft.fft2(b), shell, n_shells + 1)


def calc_frc_2d(img1, img2, apix):
    h, w = np.asarray(img1).shape
    return np.arange(min(h, w) // 2 + 1) / (min(h, w) * apix), ratio(sums_2d(img1, img2))


def frc_score(img1, img2, apix):
    _, fsc = calc_frc_2d(img1, img2, apix)
    ok = np.isfinite(fsc) & (fsc >= -1) & (fsc <= 1)
    return float(np.mean(fsc[ok])) if ok.any() else 0.0


def make_map_pair(n, seed, signal=8.0, sigma=1.5, dims=3, shape=None, quantum=None, dc=None):
    """The recipe of the fixture: one smooth signal (Gaussian-filtered normal noise times `signal`) shared by both members,
    plus independent unit white noise on each (the noise floor that keeps every shell's power above 1e-4 of the strongest);
    rounded to float16 so that it stores exactly, returned as float32.  `quantum`: the values are first rounded to multiples
    of it (the fixture's 1/8: fewer distinct values, a smaller file; the rounding error is one more white term).  `dc`: a constant added to both members, and in 2-D the same amplitude times
    the checkerboard (-1)^(y + x).  The DC shell is a single bin, |sum x|^2, and so is the last ring of an image with even sides
    (the Nyquist corner); by chance a single bin can be far below its mean.  `dc="auto"` uses 1 / sqrt(shortest side), which
    puts those bins near the power of the strongest shells whatever the draw (the GPU tests' inputs; the fixture's have none)."""
    from scipy.ndimage import gaussian_filter

    rng = np.random.default_rng(seed)
    shape = tuple(shape) if shape is not None else (n,) * dims
    sig = gaussian_filter(rng.standard_normal(shape), sigma) * signal
    a, b = sig + rng.standard_normal(shape), sig + rng.standard_normal(shape)
    if dc is not None:
        offset = 1.0 / np.sqrt(min(shape)) if dc == "auto" else float(dc)
        a, b = a + offset, b + offset
        if len(shape) == 2:
            board = offset * (1.0 - 2.0 * ((np.arange(shape[0])[:, None] + np.arange(shape[1])[None, :]) % 2))
            a, b = a + board, b + board
    if quantum:
        a, b = np.round(a / quantum) * quantum, np.round(b / quantum) * quantum
    return a.astype(np.float16).astype(np.float32), b.astype(np.float16).astype(np.float32)


def floor_ratio(sums):
    """min over shells that hold a bin of den / (the strongest shell's den), the smaller of the two members'."""
    out = 1.0
    for q in (1, 2):
        d = sums[:, q]
        out = min(out, float(d[d > 0].min() / d.max()))
    return out
