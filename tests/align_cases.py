"""Float64 yardstick of the batched image alignment (helicon_amd/align.py, csrc/align.inc): one evaluation of the reference's
objective (lib/alignment.py:107-154) and ``align_images`` itself, the table of the GPU cases and their generator.  NumPy and
SciPy's optimisers only, plus ``oracle.prep`` for the constant-mode warp; the package under test is not imported.  The rules:

  prepare     alignment.py:84-100: generate_tapering_filter(shape, [0.8, 0.8]) (lib/filters.py:415-466), pad_to_size,
              threshold_data(taper ref, 0.0) for the reference, the no-op thresh_fraction = -1 for the moving image; float32
  warp        transform_image(mode="constant"): oracle.prep.warp_affine on the float64 planes
  shift       skimage.registration.phase_cross_correlation(upsample_factor=1, normalization="phase", disambiguate=False) of
              unmasked float32 images: P = F_ref conj(F_mov); P /= max(|P|, 100 eps_float32); c = ifft2(P); the arg-max of |c|
              (first in C order), minus the side where an index is strictly above fix(side / 2)
  wrap warp   transform_image(post_translation=shift, mode="wrap"): _warp_fast with bilinear_interpolation whose four
              neighbours (floor / ceil of the coordinate) each go through coord_map: an index < 0 maps to
              (dim - 1) - ((-i - 1) % dim), an index > dim - 1 to i % dim; clipped to the input's range.  The inverse matrix
              is the unshifted one with its translation column moved: h2 - (h0 sx + h1 sy), h5 likewise
  score       cross_correlation_coefficient (lib/analysis.py:793-799) of (ref, warped image)[warped taper > 0]

scikit-image is not installed beside the reference, so the shift and the wrap rule are PINNED BY DERIVATION from its source
(registration/_phase_cross_correlation.py, transform/_warps_cy.pyx, _shared/interpolation.pxd of 0.25), as oracle/prep.py's
constant-mode warp is.

Two diagnostics per candidate decide what the device is compared on: ``gap = 1 - runner_up / peak`` of |c| (a shift whose peak
leads by less than the surface bound can legitimately differ) and ``borderline``, the pixels whose mask decision hangs on a
bilinear weight below 1e-5 along an axis (a neighbour that float32 and float64 coordinates weigh as 0 or not)."""
import functools

import numpy as np
from scipy.optimize import minimize, minimize_scalar

from oracle import prep as P

SEED = 11
CLAMP = 100 * float(np.finfo(np.float32).eps)
WEIGHT_EPS = 1e-5
MAX_EXCLUDED = 0.05
# The two bounds of the GPU tests: the largest device-versus-yardstick difference measured on an MI355X over the cases of this
# table by tools/align_bench.py (profiles/align.json, "accuracy"), times 4 (the margin of local_fsc_cases.TOL_CURVE):
#   surface  max |c_device - c_yardstick| / peak over every pixel of every candidate
#   score    max |score_device - score_yardstick| over the candidates whose shift agrees and that have no borderline pixel
MEASURED_SURFACE = 8.611e-5     # at (33, 47)
MEASURED_SCORE = 5.948e-7       # at (24, 130)
TOL_SURFACE = None if MEASURED_SURFACE is None else 4 * MEASURED_SURFACE
TOL_SCORE = None if MEASURED_SCORE is None else 4 * MEASURED_SCORE

# (reference shape, moving shape): no side's taper has a vanishing positive value (tests/test_align_host.py checks each)
CASES = (((33, 47), (33, 47)),      # odd sides, no padding
         ((48, 64), (41, 57)),      # odd, asymmetric padding on both axes
         ((64, 64), (64, 64)),      # exactly one tile
         ((65, 82), (65, 82)),      # just past a tile seam on both axes, half width 42
         ((24, 130), (24, 130)))    # past two tiles in x
ANGLES = tuple(-31.0 + 5.0 * k for k in range(13))
SCALES = (0.97, 1.0, 1.03, 1.06)
PLANTED = dict(flip=True, angle=187.0, scale=1.03, shift=(3, -5))   # test (j)


# ------------------------------------------------------------------------------------------ preparation
def taper_profile(w, fraction_start=0.8, fraction_slope=0.1):
    y = np.arange(0, w, dtype=np.float32) - w // 2
    y = np.abs(y / (w // 2))
    inner, outer = y < fraction_start, y > fraction_start + fraction_slope
    y = (1.0 + np.cos((y - fraction_start) / fraction_slope * np.pi)) / 2.0
    y[inner] = 1
    y[outer] = 0
    return y.astype(np.float32)


def tapering_filter(shape):
    ny, nx = shape
    f = np.ones((ny, nx), dtype=np.float32)
    f *= taper_profile(ny)[:, None]
    f *= taper_profile(nx)[None, :]
    return f


def prepare(image_ref, image_moving):
    """``(ref_work, moving_work, taper, padded)``, float32, of one reference and one moving image."""
    ref, mov = np.asarray(image_ref, dtype=np.float32), np.asarray(image_moving, dtype=np.float32)
    taper = P.pad_to_size(tapering_filter(mov.shape), ref.shape)
    padded = P.pad_to_size(mov, ref.shape)
    work = taper * padded
    r = tapering_filter(ref.shape) * ref
    thresh = r.max() * 0.0
    return (np.clip(r, thresh, None) - thresh).astype(np.float32), work.astype(np.float32), taper.astype(np.float32), padded


# ------------------------------------------------------------------------------------------ one evaluation
def inverse_matrix(shape, scale, angle):
    return np.linalg.inv(P.transform_image_matrix(shape, scale=float(scale), rotation=float(angle)))


def shifted(inv, shift):
    sy, sx = float(shift[0]), float(shift[1])
    h = np.array(inv, dtype=np.float64)
    h[0, 2] = inv[0, 2] - (inv[0, 0] * sx + inv[0, 1] * sy)
    h[1, 2] = inv[1, 2] - (inv[1, 0] * sx + inv[1, 1] * sy)
    return h


def coord_map(i, dim):
    i = np.asarray(i, dtype=np.int64)
    return np.where(i < 0, (dim - 1) - ((-i - 1) % dim), np.where(i > dim - 1, i % dim, i))


def _coords(shape, h):
    rows, cols = shape
    y, x = np.meshgrid(np.arange(rows, dtype=np.float64), np.arange(cols, dtype=np.float64), indexing="ij")
    return h[1, 0] * x + h[1, 1] * y + h[1, 2], h[0, 0] * x + h[0, 1] * y + h[0, 2]     # r, c


def warp_wrap(image, h):
    """``skimage.transform.warp(image, h, mode="wrap", order=1)`` of a 2-D image, float64."""
    img = np.asarray(image, dtype=np.float64)
    rows, cols = img.shape
    r, c = _coords(img.shape, h)
    minr, minc, maxr, maxc = np.floor(r), np.floor(c), np.ceil(r), np.ceil(c)
    dr, dc = r - minr, c - minc
    px = lambda rr, cc: img[coord_map(rr, rows), coord_map(cc, cols)]
    top = (1 - dc) * px(minr, minc) + dc * px(minr, maxc)
    bottom = (1 - dc) * px(maxr, minc) + dc * px(maxr, maxc)
    return np.clip((1 - dr) * top + dr * bottom, img.min(), img.max())


def borderline_pixels(taper, h):
    """Pixels whose ``warped taper > 0`` hangs on an axis weight below WEIGHT_EPS: the decision from the neighbours that
    carry at least that weight differs from the decision with every neighbour within WEIGHT_EPS of the coordinate."""
    t = np.asarray(taper) > 0
    rows, cols = t.shape
    r, c = _coords(t.shape, h)

    def sets(v):
        f = np.floor(v)
        strong = [(f, (1 - (v - f)) >= WEIGHT_EPS), (np.ceil(v), (v - f) >= WEIGHT_EPS)]
        possible = [(np.floor(v - WEIGHT_EPS), None), (f, None), (np.ceil(v), None), (np.ceil(v + WEIGHT_EPS), None)]
        return strong, possible

    sr, pr = sets(r)
    sc, pc = sets(c)
    strong = np.zeros(t.shape, dtype=bool)
    for ir, wr in sr:
        for ic, wc in sc:
            strong |= wr & wc & t[coord_map(ir, rows), coord_map(ic, cols)]
    possible = np.zeros(t.shape, dtype=bool)
    for ir, _ in pr:
        for ic, _ in pc:
            possible |= t[coord_map(ir, rows), coord_map(ic, cols)]
    return int(np.count_nonzero(possible != strong))


def cross_power(ref, mov):
    """``(|P| before the division, c)`` of phase_cross_correlation's unmasked route."""
    p = np.fft.fft2(np.asarray(ref, dtype=np.float64)) * np.conj(np.fft.fft2(np.asarray(mov, dtype=np.float64)))
    mag = np.abs(p)
    return mag, np.fft.ifft2(p / np.maximum(mag, CLAMP))


def shift_of(surface):
    a = np.abs(surface)
    idx = np.unravel_index(int(np.argmax(a)), a.shape)
    return tuple(int(i - n) if i > n // 2 else int(i) for i, n in zip(idx, a.shape))


def pearson(a, b):
    mean_a, mean_b = np.mean(a), np.mean(b)
    norm = np.sqrt(np.sum((a - mean_a) ** 2) * np.sum((b - mean_b) ** 2))
    return 0.0 if norm == 0 else float(np.sum((a - mean_a) * (b - mean_b)) / norm)


def evaluate(ref_work, moving_work, taper, scale, angle, keep_surface=False):
    """One evaluation: dict(shift, score, peak, nmask, gap, borderline, min_power[, surface])."""
    ref, mov, tap = (np.asarray(v, dtype=np.float64) for v in (ref_work, moving_work, taper))
    inv = inverse_matrix(ref.shape, scale, angle)
    mag, c = cross_power(ref, P.warp_affine(mov, inv, order=1))
    a = np.abs(c).ravel()
    top = np.partition(a, a.size - 2)[-2:]
    shift = shift_of(c)
    h = shifted(inv, shift)
    mask = warp_wrap(tap, h) > 0
    with np.errstate(all="ignore"):
        score = pearson(ref[mask], warp_wrap(mov, h)[mask]) if mask.any() else float("nan")
    out = dict(shift=shift, score=score, peak=float(top[1]), nmask=int(mask.sum()), gap=float(1 - top[0] / top[1]) if top[1] > 0 else 0.0,
               borderline=borderline_pixels(tap, h), min_power=float(mag.min()))
    if keep_surface:
        out["surface"] = c.real
    return out


def aligned(image, scale, angle, shift):
    img = np.asarray(image, dtype=np.float64)
    return warp_wrap(img, shifted(inverse_matrix(img.shape, scale, angle), shift))


# ------------------------------------------------------------------------------------------ align_images
def align_images(image_moving, image_ref, scale_range, angle_range, check_polarity=True, check_flip=True):
    """alignment.py:8-239 on this module's objective.  ``(result tuple, trace)``: the trace lists every evaluation as
    ``(scale, angle, flipped, evaluate(...))`` in the order the optimiser asked for them."""
    trace = []
    results = []
    for flipped in ((False, True) if check_flip else (False,)):
        mov = np.asarray(image_moving)[::-1, :] if flipped else np.asarray(image_moving)
        ref_work, work, taper, _ = prepare(image_ref, mov)
        best = [1e10, 1, 0, 0]

        def objective(x, angle0):
            if isinstance(x, np.ndarray):
                scale, angle = np.exp(x[0]), x[1]
            else:
                scale, angle = 1.0, x
            angle = angle + angle0
            e = evaluate(ref_work, work, taper, scale, angle)
            trace.append((float(scale), float(angle), flipped, e))
            if -e["score"] < best[0]:
                best[:] = [-e["score"], scale, angle, np.array(e["shift"], dtype=np.float64)]
            return -e["score"]

        angle0s = (0, 180) if check_polarity else (0,)
        if scale_range > 0:
            for angle0 in angle0s:
                minimize(objective, x0=[0, 0], args=(angle0,), method="Nelder-Mead", options=dict(xatol=0.01),
                         bounds=[(-np.log(1 + scale_range), np.log(1 + scale_range)), (-angle_range, angle_range)])
        elif angle_range > 0:
            for angle0 in angle0s:
                minimize_scalar(objective, args=(angle0,), bounds=(-angle_range, angle_range), method="bounded")
        if best[0] == 1e10:
            mask = taper > 0        # the unshifted wrap warp at scale 1, angle 0 is the identity
            score = pearson(ref_work[mask].astype(np.float64), work[mask].astype(np.float64))
        else:
            score = -best[0]
        results.append((best[1], best[2], best[3], score))
    if not check_flip:
        return results[0], trace
    return ((True, *results[1]) if results[1][3] > results[0][3] else (False, *results[0])), trace


# ------------------------------------------------------------------------------------------ generators
def blob_scene(shape, rng, blobs=14, noise=2.5):
    """Gaussian blobs (centres uniform in the middle 60 % of each side, sigma in U(1.2, 3.5), amplitude in U(1, 3)) plus white
    noise: the noise keeps every bin of the cross-power spectrum far above the clamp."""
    ny, nx = shape
    y, x = np.meshgrid(np.arange(ny, dtype=np.float64), np.arange(nx, dtype=np.float64), indexing="ij")
    img = np.zeros(shape)
    for _ in range(blobs):
        cy, cx = ny * rng.uniform(0.2, 0.8), nx * rng.uniform(0.2, 0.8)
        s, a = rng.uniform(1.2, 3.5), rng.uniform(1.0, 3.0)
        img += a * np.exp(-0.5 * ((y - cy) ** 2 + (x - cx) ** 2) / s ** 2)
    return img + noise * rng.standard_normal(shape)


def crop_centre(img, shape):
    y0, x0 = (img.shape[0] - shape[0]) // 2, (img.shape[1] - shape[1]) // 2
    return img[y0:y0 + shape[0], x0:x0 + shape[1]]


@functools.lru_cache(maxsize=None)
def make_pair(ref_shape, mov_shape, seed=SEED, planted=False):
    """A float32 reference and a float32 moving image of the same scene.  ``planted``: the moving image is the scene moved by
    the inverse of PLANTED (so that PLANTED aligns it), else by a fixed small rotation, scale and shift; then cropped to
    ``mov_shape`` and given a little noise of its own."""
    rng = np.random.default_rng(seed + 1000 * ref_shape[0] + ref_shape[1])
    scene = blob_scene(ref_shape, rng)
    if planted:
        q = PLANTED
        # aligned = warp(moving, inverse of (rotate / scale about the centre, then shift)); the moving image is therefore the
        # scene pushed through that transform's FORWARD resampling, i.e. warped with the forward matrix as the "inverse"
        fwd = P.transform_image_matrix(ref_shape, scale=q["scale"], rotation=q["angle"], post_translation=q["shift"])
        moved = warp_wrap(scene, fwd)
        moved = moved[::-1, :] if q["flip"] else moved
    else:
        moved = aligned(scene, 1.0 / 1.02, -9.0, (0, 0))
        moved = np.roll(moved, (-2, 3), axis=(0, 1))
    mov = crop_centre(moved, mov_shape) + 0.5 * rng.standard_normal(mov_shape)
    ref, mov = scene.astype(np.float32), mov.astype(np.float32)
    ref.setflags(write=False)
    mov.setflags(write=False)
    return ref, mov


def candidates():
    """``(scale, angle, plane)`` of a case: 13 angles x 4 scales x 2 polarities on two planes (the image and its flip)."""
    return [(s, a + pol, pl) for pl in (0, 1) for pol in (0.0, 180.0) for s in SCALES for a in ANGLES]


@functools.lru_cache(maxsize=None)
def case_planes(case):
    """``(ref_work, moving_work [2], taper [2], padded [2])`` of a case: the image and its vertical flip."""
    ref, mov = make_pair(*CASES[case])
    a, b = prepare(ref, mov), prepare(ref, mov[::-1, :])
    out = (a[0], np.stack([a[1], b[1]]), np.stack([a[2], b[2]]), np.stack([a[3], b[3]]))
    for v in out:
        v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def case_yardstick(case):
    """The yardstick's evaluation (with its surface) of every candidate of a case, computed once."""
    ref_work, work, taper, _ = case_planes(case)
    return tuple(evaluate(ref_work, work[pl], taper[pl], s, a, keep_surface=True) for s, a, pl in candidates())
