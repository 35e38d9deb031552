"""Shared by tests/test_image_prep_probes_host.py and tests/test_gpu_image_prep_probes.py: the probe table of the pre-sweep
image preparation and the non-cosine scores (csrc/image_prep.inc, k_affine_bilinear / k_spline_prefilter / spline_mirror in
helicon_hip.hip), each probe's reference, the comparison both tests apply, and the wrong-rule variants the host test uses to
show that a comparison would notice a defect.  CPU only: nothing here imports the device package.

A probe names the kernel and rule it aims at (``rule``), its input (``inputs()``), the call (``kind`` + ``args``: the Python
wrapper, or the C entry point where the wrapper cannot reach the path) and its reference (``reference(probe)``: oracle/prep.py;
np.histogramdd for raw counts; float64 NumPy on oracle.prep.closing_cross for raw moments).

kind                 call on the device                                              reference
warp                 hh_warp_affine_2d(image, inverse matrix, order, cval, clip)     P.warp_affine, the same matrix
transform_image      helicon_amd.transform_image(image, **args)                      P.transform_image
rotate               helicon_amd.rotate_shift_image(image, angle, pre, post, order)  P.rotate_shift_image (SciPy)
rescale              helicon_amd.denovo3D.rescale(image, scale, order, aa, clip)     P.rescale (SciPy)
moments              hh_helix_moments(image, threshold) -> 8 numbers                 moments_numpy on P.closing_cross
ssim / ms_ssim / mi  helicon_amd.solver.ssim_score / ms_ssim_score / mutual_...      P.ssim_score / ms_ssim_score / mutual_...
hist                 hh_joint_histogram(a, b, edges, bins) -> counts                 np.histogramdd (its own edges go to the device)
"""
import zlib
from dataclasses import dataclass, field

import numpy as np
from scipy import ndimage as ndi

from oracle import prep as P

CAP = 2e-4          # the project's cap: on a bound, and on the share of float32 warp pixels that may take the neighbouring cell
F32, F64 = np.float32, np.float64
DTYPES = (F32, F64)


@dataclass(frozen=True)
class Probe:
    name: str
    kind: str
    rule: str                      # "kernel: the rule the probe reaches"
    make: object                   # () -> dict of input arrays
    args: dict = field(default_factory=dict)

    def inputs(self):
        return self.make()


def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def _tname(dtype):
    return "f32" if dtype == F32 else "f64"


def _sname(shape):
    return "x".join(str(int(v)) for v in shape)


# ------------------------------------------------------------------------------------------------------------------- warp
WARP_SHAPES = ((1, 1), (1, 9), (9, 1), (2, 3), (5, 255), (5, 256), (5, 257), (3, 513))


def _translation(tx, ty):
    return np.array([[1.0, 0.0, tx], [0.0, 1.0, ty], [0.0, 0.0, 1.0]])


PROJECTIVE = np.array([[1.01, 0.02, 0.3], [-0.03, 0.98, -0.2], [1e-3, -2e-3, 1.0]])


def _quarter(shape, sign):
    """An exact quarter turn as entries 0 / +-1 with integer offsets that keep some samples inside a rectangle."""
    side = min(shape) - 1
    return np.array([[0.0, -1.0, side], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]]) if sign > 0 else np.array([[0.0, 1.0, 0.0], [-1.0, 0.0, side + 1.0], [0.0, 0.0, 1.0]])


def _warp_probes():
    out = []
    # (tag, rule, matrix(shape), order, cval, clip, image kind)
    table = [
        ("projective_o0", "k_warp_affine: the projective branch (division by z), order 0", lambda s: PROJECTIVE, 0, 0.0, 1, "wide"),
        ("projective_o1", "k_warp_affine: the projective branch (division by z), order 1", lambda s: PROJECTIVE, 1, 0.0, 1, "wide"),
        ("cval7_noclip", "k_warp_affine: cval != 0, clip = 0", lambda s: _translation(1.25, -0.75), 1, 7.0, 0, "wide"),
        ("cval7_clip", "k_warp_affine / k_prep_clip: cval != 0 kept by the preserve-cval rule", lambda s: _translation(1.25, -0.75), 1, 7.0, 1, "wide"),
        ("mixed_border_clip", "k_prep_clip: border pixels mixing cval with the image are clipped up to its minimum, exact zeros stay",
         lambda s: _translation(2.5, 2.5), 1, 0.0, 1, "high"),
        ("nan_no_clip", "k_prep_minmax / k_prep_clip: a NaN in the image switches the clip off", lambda s: _translation(2.5, 2.5), 1, 0.0, 1, "high_nan"),
        ("nan_identity", "k_warp_affine: corners at floor and CEIL (a NaN neighbour must not leak at integer coordinates)",
         lambda s: np.eye(3), 1, 0.0, 1, "wide_nan"),
        ("tie_pp", "k_warp_affine: order 0 rounds a .5 tie away from zero", lambda s: _translation(0.5, 0.5), 0, 0.0, 1, "wide"),
        ("tie_mm", "k_warp_affine: order 0 rounds a -.5 tie away from zero", lambda s: _translation(-0.5, -0.5), 0, 0.0, 1, "wide"),
        ("tie_pm", "k_warp_affine: order 0 ties of both signs", lambda s: _translation(0.5, -0.5), 0, 0.0, 1, "wide"),
        ("identity", "k_warp_affine: the identity returns the image", lambda s: np.eye(3), 1, 0.0, 1, "wide"),
        ("quarter_p", "k_warp_affine: exact quarter turn (0 / +-1 entries, integer offsets)", lambda s: _quarter(s, +1), 1, 0.0, 1, "wide"),
        ("quarter_m", "k_warp_affine: exact quarter turn the other way", lambda s: _quarter(s, -1), 1, 0.0, 1, "wide"),
    ]
    for tag, rule, mat, order, cval, clip, kind in table:
        for shape in WARP_SHAPES:
            for dtype in DTYPES:
                name = f"warp/{tag}/{_sname(shape)}/{_tname(dtype)}"

                def make(name=name, shape=shape, dtype=dtype, kind=kind):
                    r = _rng(name).random(shape)
                    img = (5.0 + r if kind.startswith("high") else 3.0 * r - 1.0).astype(dtype)
                    if kind.endswith("nan"):
                        img[shape[0] // 2, shape[1] // 2] = np.nan
                    return dict(image=img)

                out.append(Probe(name, "warp", rule, make, dict(matrix=mat(shape), order=order, cval=cval, clip=clip)))
    return out


def _smooth(shape):
    y, x = np.meshgrid(np.arange(shape[0]), np.arange(shape[1]), indexing="ij")
    taper = np.sin(np.pi * (y + 0.5) / shape[0]) * np.sin(np.pi * (x + 0.5) / shape[1])     # small where cval = 0 takes over
    return ((1.0 + 0.5 * np.sin(x / 23.0) * np.cos(y / 17.0)) * taper).astype(F32)


def _transform_probes():
    """The one float32 warp whose matrix the wrapper and the oracle compose each on their own: a general angle."""
    return [Probe("transform_image/general_angle/33x47/f32", "transform_image",
                  "k_warp_affine through transform_image: float32 coordinates of a general angle",
                  lambda: dict(image=_smooth((33, 47))), dict(rotation=7.0, post_translation=(1.5, -0.75)))]


# ---------------------------------------------------------------------------------------------------- rotate_shift_image
ROTATE_SHAPES = ((64, 64), (48, 80), (33, 47), (7, 9))
ROTATE_SHIFTS = ((0, 0), (1, 0), (0.5, 0), (2.5, -1), (-3, 2))
ROTATE_THIN = ((1, 9), (9, 1), (2, 3), (3, 513), (257, 5), (4, 255), (4, 256), (4, 257))


def _positive(name, shape):
    return (0.5 + 1.5 * _rng(name).random(shape)).astype(F32)


def _rotate_probes():
    out = []

    def add(tag, rule, shape, angle, post, order):
        name = f"rotate/{tag}/{_sname(shape)}/o{order}"
        out.append(Probe(name, "rotate", rule, lambda: dict(image=_positive(name, shape)), dict(angle=angle, pre=(0, 0), post=post, order=order)))

    for order in (1, 3):
        kern = "k_affine_bilinear" if order == 1 else "k_affine_cubic"
        for shape in ROTATE_SHAPES:
            for angle in (0, 90, -90, 180, 270):
                for post in ROTATE_SHIFTS:
                    add(f"a{angle}_s{post[0]}_{post[1]}", f"{kern}: inside/outside verdict 0 <= c <= n - 1 at right angles, float64 sum (m y + m x) + o",
                        shape, angle, post, order)
        for shape in ROTATE_THIN:
            add("a31.5_s0.25_-0.5", f"{kern}: sides 1, 2, 3 (mirrored taps, y1 = min(y0 + 1, ny - 1)) and width seams", shape, 31.5, (0.25, -0.5), order)
            for post in ((0, 0), (0, 0.5), (0, -1)):
                add(f"a0_s{post[0]}_{post[1]}", f"{kern}: sides 1, 2, 3 with samples inside, c = n - 1 exactly", shape, 0, post, order)
    return out


def rotate_matrix(shape, angle, pre_shift, post_shift):
    """The float32 matrix and offset of rotate_shift_image (lib/transforms.py:315-369), formed as oracle/prep.py forms them."""
    ny, nx = shape
    centre = np.array((ny // 2, nx // 2), dtype=F32)
    ang = np.deg2rad(angle)
    m = np.array([[np.cos(ang), np.sin(ang)], [-np.sin(ang), np.cos(ang)]], dtype=F32)
    offset = -np.dot(m, np.array(post_shift, dtype=F32).T)
    offset += centre.T - np.dot(m, centre.T)
    offset += -np.array(pre_shift, dtype=F32).T
    return m, offset


def affine_numpy(image, m, offset, *, offset_first=False, strict_upper=False):
    """scipy.ndimage.affine_transform(order=1, mode="constant", cval=0) restated: the coordinate (m00 y + m01 x) + o in float64,
    inside iff 0 <= c <= n - 1 on both axes, the 2 x 2 support summed in (y, x) order with weights w_y w_x."""
    img = np.asarray(image)
    ny, nx = img.shape
    m = np.asarray(m, dtype=F64)
    o = np.asarray(offset, dtype=F64)
    y, x = np.meshgrid(np.arange(ny, dtype=F64), np.arange(nx, dtype=F64), indexing="ij")
    if offset_first:
        cy, cx = (o[0] + m[0, 0] * y) + m[0, 1] * x, (o[1] + m[1, 0] * y) + m[1, 1] * x
    else:
        cy, cx = (m[0, 0] * y + m[0, 1] * x) + o[0], (m[1, 0] * y + m[1, 1] * x) + o[1]
    if strict_upper:
        inside = (cy >= 0) & (cy < ny - 1) & (cx >= 0) & (cx < nx - 1)
    else:
        inside = (cy >= 0) & (cy <= ny - 1) & (cx >= 0) & (cx <= nx - 1)
    cy, cx = np.where(inside, cy, 0.0), np.where(inside, cx, 0.0)
    fy, fx = np.floor(cy), np.floor(cx)
    y0, x0 = fy.astype(int), fx.astype(int)
    wy, wx = cy - fy, cx - fx
    y1, x1 = np.minimum(y0 + 1, ny - 1), np.minimum(x0 + 1, nx - 1)
    d = img.astype(F64)
    acc = d[y0, x0] * ((1 - wy) * (1 - wx))
    acc = acc + d[y0, x1] * ((1 - wy) * wx)
    acc = acc + d[y1, x0] * (wy * (1 - wx))
    acc = acc + d[y1, x1] * (wy * wx)
    return np.where(inside, acc, 0.0).astype(img.dtype)


# ------------------------------------------------------------------------------------------------------- rescale / resize
RESCALE_PAIRS = (((1, 40), 0.5), ((40, 1), 0.5), ((2, 2), 0.5), ((2, 2), 2.0), ((3, 300), 0.3), ((300, 3), 0.3), ((7, 7), 1 / 7), ((4, 4), 0.1),
                 ((9, 1030), 0.25), ((256, 257), 0.5), ((257, 513), 0.5), ((16, 520), 2.0),
                 ((5, 255), 0.5), ((5, 256), 0.5))     # (the last two: the remaining width seams)


def _wide(name, shape, dtype):
    return (3.0 * _rng(name).random(shape) - 1.0).astype(dtype)


def _step(shape, dtype):
    img = np.zeros(shape, dtype=dtype)
    img[:, shape[1] // 2:] = 1.0
    img[shape[0] // 2:, :] += 0.5
    return img


def _rescale_probes():
    out = []

    def add(tag, rule, shape, scale, dtype, order, aa=True, clip=True, step=False):
        name = f"rescale/{tag}/{_sname(shape)}/o{order}/{_tname(dtype)}"
        make = (lambda: dict(image=_step(shape, dtype))) if step else (lambda: dict(image=_wide(name, shape, dtype)))
        out.append(Probe(name, "rescale", rule, make, dict(scale=scale, order=order, anti_aliasing=aa, clip=clip)))

    for dtype in DTYPES:
        for order in (1, 3):
            for shape, scale in RESCALE_PAIRS:
                add(f"s{scale:.3g}", "k_gauss_axis / k_zoom_grid / k_spline_prefilter: sides of 1, radius beyond the line, folds on up-scaling, width seams",
                    shape, scale, dtype, order)
            add("axis1_only", "prep_rescale: only axis 1 is filtered (pass / dst[pass])", (16, 520), (1.0, 0.5), dtype, order)
            add("axis0_only", "prep_rescale: only axis 0 is filtered (pass / dst[pass])", (520, 16), (0.5, 1.0), dtype, order)
            add("no_aa", "k_zoom_grid: anti_aliasing=False at a seam width", (9, 514), 0.5, dtype, order, aa=False)
        add("step_clip", "k_prep_clip after rescale: the cubic overshoot of a step edge clipped to the input's range", (12, 34), 1.5, dtype, 3, step=True)
        add("step_noclip", "k_zoom_grid: the cubic overshoot of a step edge kept with clip off", (12, 34), 1.5, dtype, 3, clip=False, step=True)
        add("step_down_clip", "k_prep_clip after rescale: a filtered step edge, clip on", (12, 34), 0.5, dtype, 3, step=True)
    return out


def resize_scipy(image, output_shape, order=3, anti_aliasing=True, clip=True, *, zoom_mode="mirror", grid_mode=True, clip_from="input",
                 gauss_mode="mirror", radius_rule="round", axis1_from_input=False):
    """P.resize with every SciPy argument and step exposed; the defaults ARE P.resize (asserted bit for bit by the host test).
    gaussian_filter is made as SciPy makes it: gaussian_filter1d per axis with sigma > 1e-15, in axis order, each from the last."""
    img = np.asarray(image)
    output_shape = tuple(int(v) for v in output_shape)
    factors = np.divide(img.shape, output_shape)
    filtered = img
    if anti_aliasing:
        first = True
        for axis in (0, 1):
            sigma = max(0.0, (factors[axis] - 1) / 2)
            if not sigma > 1e-15:
                continue
            truncate = 4.0 if radius_rule == "round" else int(4.0 * sigma) / sigma   # SciPy: radius = int(truncate sigma + 0.5)
            src = img if (axis1_from_input and not first) else filtered
            filtered = ndi.gaussian_filter1d(src, sigma, axis=axis, mode=gauss_mode, cval=0, truncate=truncate)
            first = False
    out = ndi.zoom(filtered, [1 / f for f in factors], order=order, mode=zoom_mode, cval=0, grid_mode=grid_mode)
    src = img if clip_from == "input" else filtered
    lo, hi = src.min(), src.max()
    if clip and not (np.isnan(lo) or np.isnan(hi)):
        out = np.clip(out, lo, hi)
    return out


def rescale_shape(shape, scale):
    return tuple(int(v) for v in np.maximum(np.round(np.atleast_1d(scale) * np.asarray(shape)), 1))


# ------------------------------------------------------------------------------------------------------ closing + moments
MOMENT_SHAPES = ((1, 9), (9, 1), (2, 2), (5, 257), (300, 420), (4, 255), (4, 256), (3, 513))
MOMENT_PATTERNS = ("bar_top", "bar_bottom", "bar_left", "bar_right", "frame", "lone", "holes", "checker", "equal", "equal_inexact", "nan_hole",
                   "nan_alone", "empty")
MOMENT_RULES = {
    "bar_top": "k_closing_cross: ignore-outside rule at the top border", "bar_bottom": "k_closing_cross: ignore-outside rule at the bottom border",
    "bar_left": "k_closing_cross: ignore-outside rule at the left border", "bar_right": "k_closing_cross: ignore-outside rule at the right border",
    "frame": "k_closing_cross: a mask on all four borders", "lone": "k_closing_cross / k_helix_moments: a lone pixel survives, one-term sums",
    "holes": "k_closing_cross: one-pixel holes are closed", "checker": "k_closing_cross: a checkerboard closes to the full image",
    "equal": "k_closing_cross: data == threshold is outside (>, not >=)",
    "equal_inexact": "k_closing_cross: data == float32(threshold) for a threshold float32 does not hold",
    "nan_hole": "k_helix_moments: a NaN pixel inside the closed mask", "nan_alone": "k_closing_cross: a NaN pixel is below any threshold",
    "empty": "k_helix_moments: an all-false mask reports 0 pixels",
}


def _moment_image(name, pattern, shape, dtype):
    ny, nx = shape
    rng = _rng(name)
    thr = 0.3 if pattern == "equal_inexact" else 0.25
    mask = np.zeros(shape, bool)
    t = max(1, min(3, ny // 3)), max(1, min(3, nx // 3))
    if pattern == "bar_top":
        mask[: t[0], :] = True
    elif pattern == "bar_bottom":
        mask[ny - t[0]:, :] = True
    elif pattern == "bar_left":
        mask[:, : t[1]] = True
    elif pattern == "bar_right":
        mask[:, nx - t[1]:] = True
    elif pattern == "frame":
        mask[0, :] = mask[-1, :] = mask[:, 0] = mask[:, -1] = True
    elif pattern == "lone":
        mask[ny // 2, nx // 3] = True
    elif pattern in ("holes", "nan_hole", "nan_alone"):
        mask[ny // 4: ny - ny // 4, nx // 5: nx - nx // 5] = True
        mask[ny // 2:: 7, nx // 2:: 5] = False
    elif pattern == "checker":
        mask[0::2, 0::2] = True
        mask[1::2, 1::2] = True
    elif pattern in ("equal", "equal_inexact"):
        mask[ny // 3: ny - ny // 3, :] = True
    img = np.where(mask, thr + 0.05 + 1.7 * rng.random(shape), thr - 0.05 - 1.2 * rng.random(shape)).astype(dtype)
    if pattern in ("equal", "equal_inexact"):
        # a band of pixels exactly on the threshold AS THE IMAGE TYPE HOLDS IT, beside the mask and inside it
        img[max(ny // 3 - 1, 0), :] = dtype(thr)
        img[ny // 2, ::2] = dtype(thr)
    if pattern == "nan_hole":
        img[ny // 2, nx // 2] = np.nan
    if pattern == "nan_alone":
        img[0, 0] = np.nan
    return img, thr


def _moment_probes():
    out = []
    for pattern in MOMENT_PATTERNS:
        for shape in MOMENT_SHAPES:
            for dtype in DTYPES:
                name = f"moments/{pattern}/{_sname(shape)}/{_tname(dtype)}"
                thr = 0.3 if pattern == "equal_inexact" else 0.25
                out.append(Probe(name, "moments", MOMENT_RULES[pattern], lambda name=name, pattern=pattern, shape=shape, dtype=dtype:
                                 dict(image=_moment_image(name, pattern, shape, dtype)[0]), dict(threshold=thr)))
    return out


def closing_variant(erosion_border=1, dilation_border=0):
    return lambda mask: ndi.binary_erosion(ndi.binary_dilation(mask, P._CROSS, border_value=dilation_border), P._CROSS, border_value=erosion_border)


def moments_numpy(data, threshold, *, closing=P.closing_cross, ge=False):
    """The eight outputs of hh_helix_moments in float64 NumPy — {pixels, cy, cx, i_yy, i_xx, i_xy, first row, last row} of the
    closed mask ``data > threshold`` (the comparison as NumPy makes it for a Python-scalar threshold: in the image's type) —
    and, for each, the cost of forming its sums in another order: 4 n 2^-53 of the sum of the absolute terms, carried through
    the quotients and the centroid's own error (no measured figure enters)."""
    d = np.asarray(data)
    mask = closing((d >= threshold) if ge else (d > threshold))
    ys, xs = np.nonzero(mask)
    n = len(ys)
    out, bound = np.full(8, np.nan), np.zeros(8)
    out[0] = n
    if n == 0:
        out[6], out[7] = np.inf, -np.inf
        return out, bound
    out[6], out[7] = ys.min(), ys.max()
    w = d[ys, xs].astype(F64)
    with np.errstate(invalid="ignore"):
        w = w - w.min() + 1e-8
        tw = w.sum()
        e = 4.0 * n * 2.0**-53
        cy, cx = (ys * w).sum() / tw, (xs * w).sum() / tw
        b_cy, b_cx = e * (np.abs(ys * w).sum() + abs(cy) * tw) / tw, e * (np.abs(xs * w).sum() + abs(cx) * tw) / tw
        uy, ux = ys - cy, xs - cx
        i_yy, i_xx, i_xy = (uy * uy * w).sum() / tw, (ux * ux * w).sum() / tw, (uy * ux * w).sum() / tw
        ay, ax = (np.abs(uy) * w).sum() / tw, (np.abs(ux) * w).sum() / tw
        out[1:6] = cy, cx, i_yy, i_xx, i_xy
        bound[1:6] = (b_cy, b_cx,
                      e * 2 * i_yy + 2 * b_cy * ay + b_cy * b_cy,
                      e * 2 * i_xx + 2 * b_cx * ax + b_cx * b_cx,
                      e * ((np.abs(uy * ux) * w).sum() / tw + abs(i_xy)) + b_cy * ax + b_cx * ay + b_cy * b_cx)
    return out, bound


# -------------------------------------------------------------------------------------------------------------- SSIM
SSIM_SHAPES = ((7, 7), (7, 300), (300, 7), (8, 262), (8, 263), (13, 519), (7, 255), (7, 256), (7, 257))
MS_SSIM_SHAPES = ((13, 262), (64, 520))


def _ssim_pair(name, shape):
    # a ramp along the longer side under a little texture: window variances of the size of C2 = (0.03 R)^2, where the
    # covariance normalisation and the window decide the score
    rng = _rng(name)
    ramp = np.linspace(0.0, 1.0, max(shape)).reshape((-1, 1) if shape[0] >= shape[1] else (1, -1))
    a = (ramp + 0.02 * ndi.gaussian_filter(rng.standard_normal(shape), 1.0)).astype(F32)
    b = (a + 0.02 * rng.standard_normal(shape)).astype(F32)
    return dict(a=a, b=b)


def _ssim_probes():
    out = []
    for shape in SSIM_SHAPES:
        name = f"ssim/{_sname(shape)}"
        out.append(Probe(name, "ssim", "k_ssim_axis0 / k_ssim_map: one-pixel map, cols - 6 either side of the 256-thread block, dead tail threads add 0",
                         lambda name=name, shape=shape: _ssim_pair(name, shape)))
    for shape in MS_SSIM_SHAPES:
        name = f"ms_ssim/{_sname(shape)}"
        out.append(Probe(name, "ms_ssim", "k_ssim_map / k_zoom_grid order 1: the scales of ms_ssim_score across the block seam",
                         lambda name=name, shape=shape: _ssim_pair(name, shape)))
    return out


def ssim_numpy(im1, im2, *, win=7, cov_norm=None, crop=True):
    """P.ssim_score restated with the window, the covariance normalisation and the crop of the mean exposed."""
    im1, im2 = np.asarray(im1, dtype=F32), np.asarray(im2, dtype=F32)
    R = max(im1.max() - im1.min(), im2.max() - im2.min())
    npx = win * win
    cov_norm = npx / (npx - 1) if cov_norm is None else cov_norm
    ux, uy = ndi.uniform_filter(im1, size=win), ndi.uniform_filter(im2, size=win)
    uxx, uyy, uxy = ndi.uniform_filter(im1 * im1, size=win), ndi.uniform_filter(im2 * im2, size=win), ndi.uniform_filter(im1 * im2, size=win)
    vx, vy, vxy = cov_norm * (uxx - ux * ux), cov_norm * (uyy - uy * uy), cov_norm * (uxy - ux * uy)
    C1, C2 = (0.01 * R) ** 2, (0.03 * R) ** 2
    S = ((2 * ux * uy + C1) * (2 * vxy + C2)) / ((ux ** 2 + uy ** 2 + C1) * (vx + vy + C2))
    pad = (win - 1) // 2
    return float(S[pad:-pad, pad:-pad].mean(dtype=F64) if crop else S.mean(dtype=F64))


# -------------------------------------------------------------------------------------------------------- joint histogram
def _hist_probes():
    out = []

    def add(tag, rule, make, bins):
        out.append(Probe(f"hist/{tag}/b{bins}", "hist", rule, make, dict(bins=bins)))

    def random_pair(name, n):
        def make():
            rng = _rng(name)
            a = (3.0 * rng.random(n) - 1.0).astype(F32)
            return dict(a=a, b=(0.6 * a + 1.2 * rng.random(n)).astype(F32))
        return make

    def edge_pair(bins):
        def make():
            e = np.linspace(F32(-1.0), F32(2.0), bins + 1).astype(F32)       # the values np.histogramdd's own edges take
            a = np.tile(e, 3)
            return dict(a=a, b=np.ascontiguousarray(a[::-1]))
        return make

    for bins in (1, 2, 64, 257):
        add("n360000", "k_joint_hist: the grid-stride loop (n > 262144, grid capped at 1024 blocks)", random_pair(f"hist/n360000/{bins}", 360000), bins)
        add("n257", "k_joint_hist: one block and one thread of the next", random_pair(f"hist/n257/{bins}", 257), bins)
        add("n1", "k_joint_hist: a single value (widened edges)", random_pair(f"hist/n1/{bins}", 1), bins)
        add("edges", "k_joint_hist: values exactly on inner edges and on the outermost edges", edge_pair(bins), bins)
        add("constant", "k_joint_hist: a constant image (edges widened by one half either side)",
            lambda: dict(a=np.full(300, 0.75, F32), b=np.linspace(0, 1, 300).astype(F32)), bins)
    out.append(Probe("mi/600x600", "mi", "k_joint_hist through mutual_information_score: the grid-stride loop", lambda: {
        k: v.reshape(600, 600) for k, v in random_pair("hist/n360000/64", 360000)().items()}))
    return out


def hist_numpy(a, b, ea, eb, *, side="right", last_edge=True, limit=None):
    """np.histogramdd's counting rule restated: bin = searchsorted(edges, v, "right") - 1, the outermost edge in the last bin."""
    bins = len(ea) - 1
    a, b = np.asarray(a).ravel()[:limit].astype(F64), np.asarray(b).ravel()[:limit].astype(F64)
    ka, kb = np.searchsorted(ea, a, side) - 1, np.searchsorted(eb, b, side) - 1
    if last_edge:
        ka[a == ea[-1]] = bins - 1
        kb[b == eb[-1]] = bins - 1
    ok = (ka >= 0) & (ka < bins) & (kb >= 0) & (kb < bins)
    return np.bincount(ka[ok] * bins + kb[ok], minlength=bins * bins).reshape(bins, bins).astype(np.int64)


def hist_edges(probe, inp):
    """np.histogramdd's own edges for the probe — what the device is handed, as the float64 values they are."""
    _, (ea, eb) = np.histogramdd([inp["a"].ravel(), inp["b"].ravel()], bins=probe.args["bins"])
    return np.ascontiguousarray(ea, dtype=F64), np.ascontiguousarray(eb, dtype=F64)


# ------------------------------------------------------------------------------------------------------------------ warp, restated
def warp_numpy(image, inverse_matrix, order=1, cval=0.0, clip=True, *, ceil_rule="ceil", round_rule="away", force_affine=False,
               preserve_cval=True, clip_despite_nan=False, nudge=(0, 0)):
    """P.warp_affine restated with its rules exposed (the defaults are P.warp_affine bit for bit: asserted by the host test).
    ``nudge`` = (k_r, k_c) moves every row / column coordinate k float-ulps (np.nextafter) before it is used."""
    img = np.asarray(image)
    T = img.dtype.type
    H = np.asarray(inverse_matrix, dtype=F64).astype(img.dtype)
    rows, cols = img.shape
    tfr, tfc = np.meshgrid(np.arange(rows), np.arange(cols), indexing="ij")
    x, y = tfc.astype(img.dtype), tfr.astype(img.dtype)
    with np.errstate(all="ignore"):
        c = H[0, 0] * x + H[0, 1] * y + H[0, 2]
        r = H[1, 0] * x + H[1, 1] * y + H[1, 2]
        if not force_affine and not (H[2, 0] == 0 and H[2, 1] == 0 and H[2, 2] == 1):
            z = H[2, 0] * x + H[2, 1] * y + H[2, 2]
            c, r = c / z, r / z
        for _ in range(abs(nudge[0])):
            r = np.nextafter(r, T(np.sign(nudge[0]) * np.inf))
        for _ in range(abs(nudge[1])):
            c = np.nextafter(c, T(np.sign(nudge[1]) * np.inf))

        def pixel(rr, cc):
            inside = (rr >= 0) & (rr < rows) & (cc >= 0) & (cc < cols)
            out = np.full(rr.shape, T(cval), dtype=img.dtype)
            out[inside] = img[rr[inside], cc[inside]]
            return out

        if order == 0:
            if round_rule == "away":
                rnd = lambda v: np.where(v >= 0, np.floor(v.astype(F64) + 0.5), np.ceil(v.astype(F64) - 0.5)).astype(np.int64)
            else:
                rnd = lambda v: np.rint(v.astype(F64)).astype(np.int64)
            out = pixel(rnd(r), rnd(c))
        else:
            minr, minc = np.floor(r).astype(np.int64), np.floor(c).astype(np.int64)
            maxr, maxc = (np.ceil(r).astype(np.int64), np.ceil(c).astype(np.int64)) if ceil_rule == "ceil" else (minr + 1, minc + 1)
            dr, dc = r - minr.astype(img.dtype), c - minc.astype(img.dtype)
            one = T(1)
            top = ((one - dc) * pixel(minr, minc) + dc * pixel(minr, maxc)).astype(F64)
            bottom = ((one - dc) * pixel(maxr, minc) + dc * pixel(maxr, maxc)).astype(F64)
            out = ((one - dr).astype(F64) * top + dr.astype(F64) * bottom).astype(img.dtype)
        if clip:
            lo, hi = (img.min(), img.max()) if not clip_despite_nan or np.isnan(img).all() else (np.nanmin(img), np.nanmax(img))
            if not (np.isnan(lo) or np.isnan(hi)):
                preserve = preserve_cval and not (lo <= cval <= hi)
                keep = out == T(cval)
                out = np.clip(out, lo, hi)
                if preserve:
                    out[keep] = T(cval)
    return out


# ------------------------------------------------------------------------------------------------------------ the table
PROBES = tuple(_warp_probes() + _transform_probes() + _rotate_probes() + _rescale_probes() + _moment_probes() + _ssim_probes() + _hist_probes())
BY_NAME = {p.name: p for p in PROBES}
assert len(BY_NAME) == len(PROBES)


def reference(probe, inp=None):
    inp = probe.inputs() if inp is None else inp
    a = probe.args
    if probe.kind == "warp":
        return P.warp_affine(inp["image"], a["matrix"], order=a["order"], cval=a["cval"], clip=bool(a["clip"]))
    if probe.kind == "transform_image":
        return P.transform_image(inp["image"], **a)
    if probe.kind == "rotate":
        return P.rotate_shift_image(inp["image"], a["angle"], a["pre"], a["post"], order=a["order"])
    if probe.kind == "rescale":
        return P.rescale(inp["image"], a["scale"], order=a["order"], anti_aliasing=a["anti_aliasing"], clip=a["clip"])
    if probe.kind == "moments":
        return moments_numpy(inp["image"], a["threshold"])
    if probe.kind == "ssim":
        return P.ssim_score(inp["a"], inp["b"])
    if probe.kind == "ms_ssim":
        return P.ms_ssim_score(inp["a"], inp["b"])
    if probe.kind == "mi":
        return P.mutual_information_score(inp["a"], inp["b"])
    if probe.kind == "hist":
        return np.histogramdd([inp["a"].ravel(), inp["b"].ravel()], bins=a["bins"])[0].astype(np.int64)
    raise KeyError(probe.kind)


# ---------------------------------------------------------------------------------------------------------- the comparison
@dataclass
class Verdict:
    figure: float          # the largest difference of a compared number (0 for a purely exact comparison)
    bound: float           # what the figure is held to (0: exact)
    mismatches: int        # exactly compared items that differ (counts, verdicts, NaN positions, order-0 pixels)
    ok: bool
    note: str = ""

    def bitten(self):
        """What the host test asks of a wrong-rule variant: an exact item changed, or a number moved by 100 bounds."""
        return self.mismatches > 0 or (self.bound > 0 and self.figure >= 100.0 * self.bound)


def _scale(*arrays):
    m = 1.0
    for v in arrays:
        v = np.asarray(v, dtype=F64)
        v = v[np.isfinite(v)]
        if v.size:
            m = max(m, float(np.abs(v).max()))
    return m


def _values(got, want, bound):
    g, w = np.asarray(got, dtype=F64), np.asarray(want, dtype=F64)
    if g.shape != w.shape:
        return Verdict(np.inf, bound, 1, False, f"shape {g.shape} != {w.shape}")
    nan = int((np.isnan(g) != np.isnan(w)).sum())
    both = ~(np.isnan(g) | np.isnan(w))
    with np.errstate(invalid="ignore"):
        diff = np.abs(g[both] - w[both])
    diff = np.where(np.isnan(diff), np.inf, diff)       # inf against a finite number, or inf - inf of opposite signs
    same_inf = (g[both] == w[both])
    diff = np.where(same_inf, 0.0, diff)
    fig = float(diff.max()) if diff.size else 0.0
    return Verdict(fig, bound, nan, nan == 0 and fig <= bound)


def compare(probe, got, want, inp=None):
    """The comparison of a probe: bounds are those of the existing tests of the same function (test_gpu_prep.py,
    test_gpu_scores.py, test_gpu_round2.py), times max |input| where the input is not of order 1."""
    inp = probe.inputs() if inp is None else inp
    a = probe.args
    k = probe.kind
    if k == "warp":
        f32 = inp["image"].dtype == F32
        if np.asarray(got).dtype != np.asarray(want).dtype:
            return Verdict(np.inf, 0.0, 1, False, "dtype")
        if a["order"] == 0:
            v = _values(got, want, 0.0)
            g, w = np.asarray(got), np.asarray(want)
            v.mismatches += int(((g != w) & ~(np.isnan(g) & np.isnan(w))).sum())
            v.figure, v.ok = 0.0, v.mismatches == 0
            return v
        return _values(got, want, (2e-6 if f32 else 1e-12) * _scale(inp["image"], a["cval"]))      # no pixel left out
    if k == "transform_image":
        bound = 2e-6 * _scale(inp["image"])
        bad = np.abs(np.asarray(got, dtype=F64) - np.asarray(want, dtype=F64)) > bound
        return Verdict(float(bad.mean()), CAP, 0, bool(bad.mean() <= CAP), "share of pixels outside 2e-6")
    if k == "rotate":
        v = _values(got, want, (1e-6 if a["order"] == 1 else 2e-6) * _scale(inp["image"]))
        v.mismatches += int(((np.asarray(got) == 0) != (np.asarray(want) == 0)).sum())
        v.ok = v.ok and v.mismatches == 0
        return v
    if k == "rescale":
        if np.asarray(got).dtype != np.asarray(want).dtype:
            return Verdict(np.inf, 0.0, 1, False, "dtype")
        return _values(got, want, (3e-6 if inp["image"].dtype == F32 else 1e-11) * _scale(inp["image"]))
    if k == "moments":
        g, (w, bound) = np.asarray(got, dtype=F64), want
        exact = int(g[0] != w[0])
        if w[0] > 0:
            exact += int(g[6] != w[6]) + int(g[7] != w[7])
            exact += int((np.isnan(g[1:6]) != np.isnan(w[1:6])).sum())
        fig, rel = 0.0, 0.0
        if w[0] > 0 and not np.isnan(w[1:6]).any() and not np.isnan(g[1:6]).any():
            d = np.abs(g[1:6] - w[1:6])
            fig = float(d.max())
            with np.errstate(divide="ignore", invalid="ignore"):
                rel = float(np.nanmax(np.where(d > 0, d / bound[1:6], 0.0)))
        # the five sums each have their own bound: the figure reported is the largest difference in units of its bound
        return Verdict(rel, 1.0, exact, exact == 0 and rel <= 1.0, f"largest |difference| {fig:.3g}")
    if k in ("ssim", "ms_ssim", "mi"):
        bound = {"ssim": 2e-6, "ms_ssim": 5e-6, "mi": 1e-12}[k]
        return _values(np.array([got]), np.array([want]), bound)
    if k == "hist":
        g, w = np.asarray(got), np.asarray(want)
        n = int((g != w).sum()) if g.shape == w.shape else 1
        return Verdict(0.0, 0.0, n, n == 0)
    raise KeyError(k)


# ------------------------------------------------------------------------------------------------- the wrong-rule variants
def _resize_variant(**kw):
    def run(probe, inp):
        a = probe.args
        return resize_scipy(inp["image"], rescale_shape(inp["image"].shape, a["scale"]), order=a["order"], anti_aliasing=a["anti_aliasing"],
                            clip=a["clip"], **kw)
    return run


def _warp_variant(**kw):
    def run(probe, inp):
        a = probe.args
        return warp_numpy(inp["image"], a["matrix"], order=a["order"], cval=a["cval"], clip=bool(a["clip"]), **kw)
    return run


def _affine_variant(**kw):
    def run(probe, inp):
        a = probe.args
        m, off = rotate_matrix(inp["image"].shape, a["angle"], a["pre"], a["post"])
        return affine_numpy(inp["image"], m, off, **kw)
    return run


def _moments_variant(**kw):
    return lambda probe, inp: moments_numpy(inp["image"], probe.args["threshold"], **kw)[0]


def _ssim_variant(**kw):
    return lambda probe, inp: ssim_numpy(inp["a"], inp["b"], **kw)


def _hist_variant(**kw):
    def run(probe, inp):
        ea, eb = hist_edges(probe, inp)
        return hist_numpy(inp["a"], inp["b"], ea, eb, **kw)
    return run


def _names(prefix, *contains):
    return tuple(p.name for p in PROBES if p.name.startswith(prefix) and all(c in p.name for c in contains))


@dataclass(frozen=True)
class Variant:
    rule: str          # the one rule changed
    run: object        # (probe, inputs) -> what the device would return under the wrong rule
    probes: tuple      # the probes listed for it: at least one must be bitten


VARIANTS = {
    "zoom: mode reflect for mirror": Variant("k_zoom_grid / spline_mirror fold", _resize_variant(zoom_mode="reflect"), _names("rescale/s", "/f64")),
    "zoom: grid_mode False": Variant("k_zoom_grid coordinate (k + 0.5) zoom - 0.5", _resize_variant(grid_mode=False), _names("rescale/s", "/f64")),
    "zoom: clip from the filtered image's range": Variant("prep_rescale: k_prep_minmax reads d_in", _resize_variant(clip_from="filtered"),
                                                          _names("rescale/s0.5/25", "/f64")),
    "gauss: radius int(4 sigma)": Variant("prep_rescale: lw = int(4 sigma + 0.5)", _resize_variant(radius_rule="floor"),
                                          _names("rescale/s0.3/", "/f64") + _names("rescale/s0.25/", "/f64")),
    "gauss: mode reflect": Variant("k_gauss_axis fold", _resize_variant(gauss_mode="reflect"), _names("rescale/s", "/f64")),
    "gauss: axis 1 filtered from the input": Variant("prep_rescale: cur / dst[pass]", _resize_variant(axis1_from_input=True),
                                                     _names("rescale/s0.5/25", "/f64")),
    "warp: floor + 1 for ceil": Variant("k_warp_affine corners", _warp_variant(ceil_rule="floor+1"), _names("warp/nan_identity/")),
    "warp: round half to even": Variant("k_warp_affine order 0", _warp_variant(round_rule="even"), _names("warp/tie_")),
    "warp: affine arithmetic on a projective matrix": Variant("k_warp_affine !a.affine", _warp_variant(force_affine=True), _names("warp/projective_")),
    "warp: clip without the preserve-cval rule": Variant("k_prep_clip preserve", _warp_variant(preserve_cval=False),
                                                         _names("warp/mixed_border_clip/") + _names("warp/cval7_clip/")),
    "warp: clip despite NaN": Variant("k_prep_minmax NaN / k_prep_clip lo != lo", _warp_variant(clip_despite_nan=True), _names("warp/nan_no_clip/")),
    "affine: < for <= at n - 1": Variant("k_affine_bilinear / k_affine_cubic verdict", _affine_variant(strict_upper=True), _names("rotate/a0_", "/o1")),
    "affine: the offset added first": Variant("k_affine_bilinear / k_affine_cubic coordinate sum", _affine_variant(offset_first=True),
                                              _names("rotate/a270_", "/o1") + _names("rotate/a-90_", "/o1") + _names("rotate/a90_", "/o1")),
    "closing: erosion with border_value 0": Variant("k_closing_cross STEP 1 outside = 1", _moments_variant(closing=closing_variant(erosion_border=0)),
                                                    _names("moments/bar_") + _names("moments/frame/")),
    "closing: dilation with border_value 1": Variant("k_closing_cross STEP 0 outside = 0", _moments_variant(closing=closing_variant(dilation_border=1)),
                                                     _names("moments/lone/") + _names("moments/holes/")),
    "closing: >= for >": Variant("k_closing_cross threshold", _moments_variant(ge=True), _names("moments/equal")),
    "ssim: cov_norm 1": Variant("hh_ssim_2d cov_norm = 49 / 48", _ssim_variant(cov_norm=1.0), _names("ssim/")),
    "ssim: the mean over the whole map": Variant("k_ssim_map: the 3-pixel rim is left out", _ssim_variant(crop=False), _names("ssim/")),
    "ssim: window 5": Variant("k_ssim_axis0 / k_ssim_map: 7 taps", _ssim_variant(win=5), _names("ssim/")),
    "hist: side left": Variant("k_joint_hist: count of edges <= v", _hist_variant(side="left"), _names("hist/edges/")),
    "hist: the last edge dropped": Variant("k_joint_hist: v == e[bins]", _hist_variant(last_edge=False), _names("hist/edges/") + _names("hist/n257/")),
    "hist: a stride loop that stops at 262144": Variant("k_joint_hist grid-stride loop", _hist_variant(limit=262144), _names("hist/n360000/")),
}
