"""Float64 yardstick of the pixel-size calibration (helicon_amd/pixel_size.py, csrc/nudft.inc), the table of the GPU cases and
their generators.  NumPy only; the package under test is imported by the callers, never here.

The transform is ``finufft.nufft2d2(x, y, f)`` as the direct sum it approximates (type 2, isign = -1, centred modes, ``x``
with the FIRST image axis), in two stages::

    F[p] = sum_a ( sum_c f[a, c] e^{-i y[p] (c - nx // 2)} ) e^{-i x[p] (a - ny // 2)}
         = (exp(-i y (x) c) @ f.T * exp(-i x (x) a)).sum(1)

finufft is not installed where the fixtures are made, so the sum is PINNED BY DERIVATION, as oracle/path_b.py's zoomed spectrum
is: at x = 2 pi u / ny, y = 2 pi v / nx it equals (-1)^(u + v) np.fft.fft2(f)[u, v] (tests/test_pixel_size_host.py checks that
on non-square images, which also pins which axis x belongs to).

The one bound of the GPU tests, per image:  max_p |F_device[p] - F_yardstick[p]| <= B * sum |f - mean(f)|."""
import numpy as np

SEED = 5
TARGET = 2.13                      # graphene, Angstrom
POINT_SHAPES = [(1, 1), (2, 3), (37, 50), (64, 64), (65, 63), (128, 130)]
POINT_COUNTS = [1, 63, 64, 65]     # and hh_nudft_chunk() + 1, which the GPU test adds
LONG_SHAPES = [(4, 4096), (4096, 4), (3, 8191)]
RATE = np.pi * np.sqrt(2.0)        # the reference's band reaches the corner of the spectrum: pi sqrt 2 radians per pixel

# The largest device-versus-yardstick difference over sum |f - mean| measured on an MI355X by tools/pixel_size_bench.py over
# exactly the shapes, counts and stacks of the GPU tests (profiles/pixel_size.json, "accuracy"); B is four times it, rounded
# up to one significant digit (the factor covers other seeds).  The f32 unit round-off is 6e-8.  The largest value is the
# offset image's, at a point 0.08 radians off an axis where the mean's leakage makes |F| = 87 490: it is exactly what rounding
# the YARDSTICK to complex64 gives there (|F| 2^-24 up to sqrt 2), so it measures the output format; every other case stays
# below 1.9e-7 (the 2 x 3 image, again the output's rounding), and the images of 37 x 50 and larger below 2e-8.
MEASURED = 7.419e-7      # "offset 64x64"
B = 3e-6


def yardstick(x, y, f, block=16384):
    """complex128 [P] or [B, P]: the direct sum in float64, ``block`` points at a time."""
    f = np.asarray(f, dtype=np.float64)
    x = np.asarray(x, dtype=np.float64).reshape(-1)
    y = np.asarray(y, dtype=np.float64).reshape(-1)
    stack = f if f.ndim == 3 else f[None]
    ny, nx = stack.shape[-2:]
    a = np.arange(ny) - ny // 2
    c = np.arange(nx) - nx // 2
    out = np.empty((len(stack), x.size), np.complex128)
    for p0 in range(0, x.size, block):
        ey = np.exp(-1j * np.outer(y[p0:p0 + block], c))
        ex = np.exp(-1j * np.outer(x[p0:p0 + block], a))
        for b, img in enumerate(stack):
            out[b, p0:p0 + block] = (ey @ img.T * ex).sum(1)
    return out if f.ndim == 3 else out[0]


def ring_maximum(x, y, f, group):
    """float64 [group]: max over images and over the points p with p % group == r of |F| (calibratepixelsize.py:147-148)."""
    mag = np.abs(yardstick(x, y, np.asarray(f) if np.asarray(f).ndim == 3 else np.asarray(f)[None]))
    return mag.reshape(mag.shape[0], -1, group).max(axis=(0, 1))


def scale(f):
    """[B] (or scalar): sum |f - mean(f)| per image, float64."""
    f = np.asarray(f, dtype=np.float64)
    return np.abs(f - f.mean(axis=(-2, -1), keepdims=True)).sum(axis=(-2, -1))


def images(shape, n_img, seed=SEED, offset=0.0):
    """float32 [n_img, ny, nx]: unit noise (+ offset)."""
    rng = np.random.default_rng([seed, shape[0], shape[1], n_img])
    return (offset + rng.standard_normal((n_img,) + tuple(shape))).astype(np.float32)


def points(n, seed=SEED, origin=True):
    """(x, y) float64 [n], uniform in +-pi sqrt 2.  With ``origin``: point 0 is (0, 0), whose value is the plain sum of the
    image, and (n >= 3) point 2 is point 1 shifted by 2 pi on both axes, whose value is point 1's."""
    rng = np.random.default_rng([seed, n])
    x, y = rng.uniform(-RATE, RATE, n), rng.uniform(-RATE, RATE, n)
    if origin:
        x[0] = y[0] = 0.0
        if n >= 3:
            x[1], y[1] = rng.uniform(1.9, 4.4), -rng.uniform(1.9, 4.4)   # so that the shifted copy stays in the band too
            x[2], y[2] = x[1] - 2 * np.pi, y[1] + 2 * np.pi
    return x, y


def band(apix=1.0, target=TARGET, search_range=0.05, r_samples=100):
    """(X, Y, R, theta_samples): the calibration's polar band (calibratepixelsize.py:68-78, 100-110), points flattened [theta][r]."""
    corner_res = 2 * apix / np.sqrt(2)
    res_low = target * (1 + search_range)
    res_high = max(corner_res, target * (1 - search_range))
    theta_samples = int(np.pi / ((1 / res_high - 1 / res_low) / (r_samples - 1) / (1 / target))) + 1
    R = np.linspace(1 / res_low, 1 / res_high, r_samples)
    th, rg = np.meshgrid(np.linspace(0, np.pi, theta_samples, endpoint=False), R, indexing="ij")
    return (2 * np.pi * apix * rg * np.cos(th)).ravel(), (2 * np.pi * apix * rg * np.sin(th)).ravel(), R, theta_samples


RING_SHAPE, RING_STACK = (48, 40), 3
OFFSET_SHAPE, OFFSET = (64, 64), 1000.0


def offset_points(n=65):
    """The offset case's points: no origin.  There the mean's term is 4.1e6 and complex64 cannot hold it to better than 0.25,
    which is 7.6e-5 of sum |f - mean|: a limit of the output format, not of the transform."""
    return points(n, origin=False)


def accuracy_cases(chunk):
    """(label, images [B, ny, nx], x, y) of every comparison the GPU tests hold to the bound B: the measuring tool walks this
    same list."""
    for shape in POINT_SHAPES:
        for n_img in (1, 3):
            for n in POINT_COUNTS + [chunk + 1]:
                yield f"points {shape[0]}x{shape[1]} stack {n_img} n {n}", images(shape, n_img), *points(n)
    for shape in LONG_SHAPES:
        yield f"long {shape[0]}x{shape[1]}", images(shape, 1), *points(65)
    yield "offset 64x64", images(OFFSET_SHAPE, 1, offset=OFFSET), *offset_points()
    X, Y, _, _ = band()
    yield "band 48x40 stack 3", images(RING_SHAPE, RING_STACK), X, Y


def planted(shape, apix_true, n_img, noise_seed=1, target=TARGET, amplitude=0.3):
    """float32 [n_img, ny, nx]: unit noise (default_rng(noise_seed)) plus three cosines of ``amplitude`` at
    apix_true / target cycles per pixel along 17 + 60 k + 7 b degrees (k = 0, 1, 2; b the image), the angle measured as the
    calibration's Theta is: its cosine goes with the rows."""
    ny, nx = shape
    rng = np.random.default_rng(noise_seed)
    out = rng.standard_normal((n_img, ny, nx))
    a, c = np.meshgrid(np.arange(ny) - ny // 2, np.arange(nx) - nx // 2, indexing="ij")
    q = apix_true / target
    for b in range(n_img):
        for k in range(3):
            th = np.deg2rad(17.0 + 60.0 * k + 7.0 * b)
            out[b] += amplitude * np.cos(2 * np.pi * q * (a * np.cos(th) + c * np.sin(th)))
    return out.astype(np.float32)


def lead(curve):
    """(top - runner-up) / |top| of a curve: how far its arg-max is from changing."""
    s = np.sort(np.asarray(curve, dtype=np.float64))
    return float((s[-1] - s[-2]) / abs(s[-1]))
