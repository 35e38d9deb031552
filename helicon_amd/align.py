"""Batched 2-D image alignment on the device: ``helicon.align_images`` (lib/alignment.py:8-239) and its whole candidate grid.

One evaluation of the reference's objective at (scale, angle) is: warp the prepared moving image (``transform_image``,
``mode="constant"``), find the integer shift by phase cross-correlation (scikit-image's ``phase_cross_correlation`` with
``normalization="phase"``, ``upsample_factor=1``, ``disambiguate=False``), warp the image and its taper again with that shift
in ``mode="wrap"``, and take ``cross_correlation_coefficient`` of the reference and the warped image under ``taper > 0``.
``AlignContext`` keeps the prepared reference (and its half spectrum), the prepared moving planes and their tapers on the
device (``hh_align_*``, csrc/align.inc) and evaluates any list of (moving plane, scale, angle) in one call: only the 2 x 3
inverse matrices go up, only (shift, score, peak, mask count) come back.  A candidate's result is bit-identical from run to run
and independent of the rest of the list.  Precision: float32 planes, coordinates and transforms (as the reference's float32
images get from scikit-image), float64 moments and score.

``align_images`` keeps the reference's signature, return tuples and optimiser calls (SciPy's Nelder-Mead / bounded scalar
search drive the device objective); the flipped image is a second plane of the same context.  The objective jumps wherever the
integer shift does, so a local search from 0 is fragile: ``align_images_grid`` evaluates every (image, flip, polarity, scale,
angle) in one call and can start the reference's optimiser from the grid's best (``refine=True``).

    python -m helicon_amd.align moving.mrc ref.mrc --angle-range 180 --angle-step 1 --scale-range 0.05 --scale-step 0.01
                                [--no-flip] [--no-polarity] [--refine] [--out aligned.mrc] [--device 0]

reads two 2-D images (``.mrc`` / ``.npy``; the moving image no larger than the reference), prints a JSON report (best flip,
scale, angle, shift, score; candidates, seconds) and writes the aligned, untapered moving image with ``--out``.
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import sys
import time
from collections import namedtuple

import numpy as np

from . import _lib
from .fsc import _f32, _read_map
from .local_resolution import taper_profile

__all__ = ["AlignContext", "AlignEval", "AlignBest", "align_images", "align_images_grid", "generate_tapering_filter",
           "inverse_matrices", "chunk", "main"]

_f32p, _f64p, _i32p = C.POINTER(C.c_float), C.POINTER(C.c_double), C.POINTER(C.c_int32)
_MIN_SIDE, _MAX_SIDE = 2, 1024

AlignEval = namedtuple("AlignEval", "shifts scores peaks nmask")           # [n, 2] int32 (y, x), [n] f64, [n] f32, [n] int32
AlignBest = namedtuple("AlignBest", "flip scale angle shift score")


def chunk():
    """Candidates of one launch group (compiled in)."""
    return int(_lib.lib().hh_align_chunk())


def generate_tapering_filter(image_size, fraction_start=(0.8, 0.8), fraction_slope=0.1):
    """``helicon.generate_tapering_filter`` (lib/filters.py:415-466): float32 ``[ny, nx]``, the product of the two one-axis
    profiles (an axis whose fraction is outside (0, 1) is all ones)."""
    ny, nx = (int(v) for v in image_size)
    fy, fx = fraction_start
    if not (0 < fy < 1 or 0 < fx < 1):
        return np.ones((ny, nx))
    return (np.ones((ny, nx), dtype=np.float32) * taper_profile(ny, fy, fraction_slope)[:, None]) * taper_profile(nx, fx, fraction_slope)[None, :]


def _pad_to_size(d, shape):
    from .denovo3D import pad_to_size

    if d.shape[0] > shape[0] or d.shape[1] > shape[1]:
        raise ValueError(f"align: a moving image {d.shape} larger than the reference {tuple(shape)} is not provided")
    return pad_to_size(d, tuple(shape))


def _affine(scale, rotation, t):
    return np.array([[scale * np.cos(rotation), -scale * np.sin(rotation), t[0]],
                     [scale * np.sin(rotation), scale * np.cos(rotation), t[1]],
                     [0.0, 0.0, 1.0]])


def inverse_matrices(shape, scales, angles):
    """``[n, 6]`` float64: the first two rows of ``xform.inverse`` of ``transform_image(image of this shape, scale, rotation)``,
    composed as ``transform_image`` composes it (to the centre ``shape / 2``, rotate / scale, back), angles in degrees."""
    scales, angles = np.broadcast_arrays(np.asarray(scales, dtype=np.float64), np.asarray(angles, dtype=np.float64))
    s, r = scales.ravel(), np.deg2rad(angles.ravel())
    cy, cx = shape[0] / 2.0, shape[1] / 2.0
    centre = np.zeros((s.size, 3, 3))
    centre[:, 0, 0], centre[:, 0, 1] = s * np.cos(r), -s * np.sin(r)
    centre[:, 1, 0], centre[:, 1, 1] = s * np.sin(r), s * np.cos(r)
    centre[:, 2, 2] = 1.0
    m = _affine(1.0, 0.0, (cx, cy)) @ (centre @ _affine(1.0, 0.0, (-cx, -cy)))   # a + b applies a first; the translations are (0, 0)
    return np.ascontiguousarray(np.linalg.inv(m)[:, :2, :].reshape(-1, 6))


class AlignContext:
    """One reference image and any number of moving images (each no larger than the reference), prepared as the reference
    prepares them (alignment.py:84-100) and resident on the device; a context manager."""

    def __init__(self, image_ref, images_moving, *, device=0):
        from .denovo3D import threshold_data

        ref = _f32(image_ref, "AlignContext")
        single = np.asarray(images_moving[0]).ndim == 1 if len(images_moving) else False
        movs = [images_moving] if single else list(images_moving)
        if ref.ndim != 2 or not movs:
            raise ValueError("AlignContext: a 2-D reference and at least one 2-D moving image are needed")
        work, tapers, padded = [], [], []
        for m in movs:
            m = _f32(m, "AlignContext")
            if m.ndim != 2:
                raise ValueError(f"AlignContext: 2-D moving images are needed; got {m.shape}")
            t = _pad_to_size(generate_tapering_filter(m.shape, [0.8, 0.8]), ref.shape)
            p = _pad_to_size(m, ref.shape)
            tapers.append(t)
            padded.append(p)
            work.append(t * p)                    # threshold_data(..., thresh_fraction=-1) is the identity
        ref_work = np.asarray(threshold_data(generate_tapering_filter(ref.shape, [0.8, 0.8]) * ref, 0.0, device=device), dtype=np.float32)
        self._init_planes(ref_work, np.stack(work), np.stack(tapers), device)
        self.padded = np.stack(padded)

    @classmethod
    def from_planes(cls, ref_work, moving_work, taper, *, device=0):
        """A context of prepared planes: ``ref_work [ny, nx]``, ``moving_work`` and ``taper`` ``[M, ny, nx]`` (or one plane each)."""
        self = cls.__new__(cls)
        mw, tp = np.asarray(moving_work), np.asarray(taper)
        self._init_planes(ref_work, mw[None] if mw.ndim == 2 else mw, tp[None] if tp.ndim == 2 else tp, device)
        self.padded = None
        return self

    def _init_planes(self, ref_work, moving_work, taper, device):
        self._ctx = None
        ref, mw, tp = _f32(ref_work, "AlignContext"), _f32(moving_work, "AlignContext"), _f32(taper, "AlignContext")
        if ref.ndim != 2 or mw.ndim != 3 or mw.shape[1:] != ref.shape or tp.shape != mw.shape or mw.shape[0] < 1:
            raise ValueError(f"AlignContext: planes of the reference's shape are needed; got {ref.shape}, {mw.shape}, {tp.shape}")
        if min(ref.shape) < _MIN_SIDE or max(ref.shape) > _MAX_SIDE:
            raise ValueError(f"AlignContext: every side must lie in [{_MIN_SIDE}, {_MAX_SIDE}]; got {ref.shape}")
        self.shape, self.n_moving, self.device = tuple(int(v) for v in ref.shape), int(mw.shape[0]), int(device)
        self.ref_work, self.moving_work, self.taper = ref, mw, tp
        ctx = C.c_void_p()
        _lib.check(_lib.lib().hh_align_create(self.device, self.shape[0], self.shape[1], ref.ctypes.data_as(_f32p), self.n_moving,
                                              mw.ctypes.data_as(_f32p), tp.ctypes.data_as(_f32p), C.byref(ctx)), None)
        self._ctx = ctx

    def close(self):
        if getattr(self, "_ctx", None):
            _lib.lib().hh_align_destroy(self._ctx)
            self._ctx = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _open(self):
        if not self._ctx:
            raise _lib.HeliconHipError("AlignContext: the context is closed")
        return self._ctx

    def _plane_index(self, moving):
        m = int(moving)
        if m != moving or not 0 <= m < self.n_moving:
            raise ValueError(f"AlignContext: moving must be a plane index in [0, {self.n_moving}); got {moving!r}")
        return m

    def evaluate(self, scales, angles, moving=0):
        """The objective at every (scale, angle in degrees, moving plane); the three broadcast together.  ``AlignEval``."""
        scales, angles, moving = np.broadcast_arrays(np.asarray(scales, dtype=np.float64), np.asarray(angles, dtype=np.float64),
                                                     np.asarray(moving))
        return self.evaluate_matrices(inverse_matrices(self.shape, scales, angles), moving.ravel())

    def evaluate_matrices(self, inv, moving):
        inv = np.ascontiguousarray(inv, dtype=np.float64).reshape(-1, 6)
        idx = np.ascontiguousarray(np.broadcast_to(np.asarray(moving), (len(inv),)), dtype=np.int32)
        n = len(inv)
        if n < 1 or (idx < 0).any() or (idx >= self.n_moving).any() or not np.isfinite(inv).all():
            raise ValueError("AlignContext: at least one candidate, finite matrices and plane indices inside the context are needed")
        shifts, scores = np.empty((n, 2), dtype=np.int32), np.empty(n, dtype=np.float64)
        peaks, nmask = np.empty(n, dtype=np.float32), np.empty(n, dtype=np.int32)
        _lib.check(_lib.lib().hh_align_eval(self._open(), n, idx.ctypes.data_as(_i32p), inv.ctypes.data_as(_f64p), shifts.ctypes.data_as(_i32p),
                                            scores.ctypes.data_as(_f64p), peaks.ctypes.data_as(_f32p), nmask.ctypes.data_as(_i32p)), None)
        return AlignEval(shifts, scores, peaks, nmask)

    def correlation(self, scale, angle, moving=0):
        """The correlation surface ``c`` (float32 ``[ny, nx]``) of one candidate; its shift is the arg-max of ``|c|``."""
        inv = inverse_matrices(self.shape, scale, angle)
        out = np.empty(self.shape, dtype=np.float32)
        _lib.check(_lib.lib().hh_align_correlation(self._open(), self._plane_index(moving), inv.ctypes.data_as(_f64p), out.ctypes.data_as(_f32p)), None)
        return out

    def aligned(self, scale, angle, shift, moving=0, which="image"):
        """The second warp (``mode="wrap"``, post-translation ``shift`` = (y, x), integers) of ``which``: ``"image"`` the
        untapered padded moving image (what ``return_aligned_moving_image`` gives), ``"work"`` the prepared plane, ``"taper"``
        its taper, or a caller's plane of the reference's shape."""
        m = self._plane_index(moving)
        sh = np.asarray(shift)
        if sh.shape != (2,) or (sh != np.round(sh)).any():
            raise ValueError(f"AlignContext.aligned: an integer shift (y, x) is needed; got {shift!r}")
        sh = np.ascontiguousarray(sh, dtype=np.int32)
        inv = inverse_matrices(self.shape, scale, angle)
        plane = None
        if isinstance(which, str):
            if which not in ("image", "work", "taper"):
                raise ValueError(f"AlignContext.aligned: which must be 'image', 'work', 'taper' or a plane; got {which!r}")
            if which == "image":
                if self.padded is None:
                    raise ValueError("AlignContext.aligned: a context made from prepared planes holds no untapered image")
                plane = self.padded[m]
        else:
            plane = _f32(which, "AlignContext.aligned")
            if plane.shape != self.shape:
                raise ValueError(f"AlignContext.aligned: a plane of shape {self.shape} is needed; got {plane.shape}")
        out = np.empty(self.shape, dtype=np.float32)
        _lib.check(_lib.lib().hh_align_warp_wrap(self._open(), None if plane is None else np.ascontiguousarray(plane).ctypes.data_as(_f32p), m,
                                                 int(which == "taper") if isinstance(which, str) else 0, inv.ctypes.data_as(_f64p),
                                                 sh.ctypes.data_as(_i32p), out.ctypes.data_as(_f32p)), None)
        return out

    def profile(self, enable=None):
        """Device-event milliseconds of ``evaluate`` per phase since the last switch; ``enable`` switches the timing and resets."""
        ms = (C.c_double * 5)()
        _lib.check(_lib.lib().hh_align_profile(self._open(), -1 if enable is None else int(bool(enable)), ms), None)
        return dict(zip(("warp", "forward", "inverse_y", "c2r_argmax", "score"), (float(v) for v in ms)))


def _pearson(a, b):
    # cross_correlation_coefficient (lib/analysis.py:793-799) in float64 on the host: the degenerate call only
    a, b = a.astype(np.float64), b.astype(np.float64)
    da, db = a - np.mean(a), b - np.mean(b)
    norm = np.sqrt(np.sum(da ** 2) * np.sum(db ** 2))
    return 0 if norm == 0 else np.sum(da * db) / norm


def _search(ctx, plane, log_bounds, angle_bounds, angle0s, x0=None, trace=None):
    """The reference's optimiser calls (alignment.py:107-197) on the device objective of one plane: ``best`` as it keeps it
    (``[-score, scale, angle, shift]``; the start values when nothing was evaluated)."""
    best = [1e10, 1, 0, 0]

    def objective(x, angle0):
        if isinstance(x, np.ndarray):
            scale_log, angle = x
            scale = np.exp(scale_log)
        else:
            scale, angle = 1.0, x
        angle = angle + angle0
        r = ctx.evaluate(scale, angle, plane)
        score = -float(r.scores[0])
        if trace is not None:
            trace.append((float(scale), float(angle), int(plane)))
        if score < best[0]:
            best[:] = [score, scale, angle, r.shifts[0].astype(np.float64)]
        return score

    if log_bounds is not None:
        from scipy.optimize import minimize

        for angle0 in angle0s:
            minimize(objective, x0=[0, 0] if x0 is None else list(x0), args=(angle0,), bounds=[tuple(log_bounds), tuple(angle_bounds)],
                     method="Nelder-Mead", options=dict(xatol=0.01))
    elif angle_bounds is not None:
        from scipy.optimize import minimize_scalar

        for angle0 in angle0s:
            minimize_scalar(objective, args=(angle0,), bounds=tuple(angle_bounds), method="bounded")
    return best


def _align_plane(ctx, plane, scale_range, angle_range, check_polarity, return_image, trace=None):
    angle0s = (0, 180) if check_polarity else (0,)
    if scale_range > 0:
        best = _search(ctx, plane, (-np.log(1 + scale_range), np.log(1 + scale_range)), (-angle_range, angle_range), angle0s, trace=trace)
    elif angle_range > 0:
        best = _search(ctx, plane, None, (-angle_range, angle_range), angle0s, trace=trace)
    else:
        best = [1e10, 1, 0, 0]
    neg, scale, angle, shift = best
    if neg == 1e10:   # nothing evaluated: the reference scores the prepared image itself under the unshifted taper
        mask = ctx.aligned(1, 0, (0, 0), plane, "taper") > 0
        score = _pearson(ctx.ref_work[mask], ctx.moving_work[plane][mask])
        shift_yx = (0, 0)
    else:
        score, shift_yx = -neg, shift
    if return_image:
        return scale, angle, shift, score, ctx.aligned(scale, angle, shift_yx, plane, "image")
    return scale, angle, shift, score


def align_images(image_moving, image_ref, scale_range, angle_range, check_polarity=True, check_flip=True,
                 return_aligned_moving_image=False, *, device=0, _trace=None):
    """``helicon.align_images`` (lib/alignment.py:8-239) with its return tuples: ``(scale, rotation_angle_degree,
    shift_cartesian, similarity_score[, aligned_image])``, led by the flip flag when ``check_flip`` is on; the start values
    ``(1, 0, 0, score of the unmoved image)`` when both ranges are 0."""
    assert 0 <= scale_range < 1, f"align_images(): {scale_range=} is out of valid range [0, 1)"
    mov = np.asarray(image_moving)
    planes = [mov, mov[::-1, :]] if check_flip else [mov]
    with AlignContext(image_ref, planes, device=device) as ctx:
        result = _align_plane(ctx, 0, scale_range, angle_range, check_polarity, return_aligned_moving_image, _trace)
        if not check_flip:
            return result
        result_flip = _align_plane(ctx, 1, scale_range, angle_range, check_polarity, return_aligned_moving_image, _trace)
    if result_flip[3] > result[3]:
        return (True, *result_flip)
    return (False, *result)


def align_images_grid(images_moving, image_ref, scales, angles, check_polarity=True, check_flip=True, refine=False, *, device=0):
    """Every (image, flip, polarity, scale, angle) through one ``evaluate`` call.  Returns ``(best, scores)``: ``scores`` is
    ``[n_images, n_flip, n_polarity, n_scales, n_angles]`` float64 and ``best`` one ``AlignBest(flip, scale, angle, shift,
    score)`` per image (the angle includes the polarity's 180 degrees; NaN scores never win); a single 2-D image gives a single
    ``AlignBest`` and ``scores`` without the leading axis.  ``refine=True`` then runs the reference's optimiser from each
    image's best, inside the grid's extent."""
    single = np.asarray(images_moving[0]).ndim == 1
    imgs = [np.asarray(images_moving)] if single else [np.asarray(m) for m in images_moving]
    scales, angles = np.atleast_1d(np.asarray(scales, dtype=np.float64)), np.atleast_1d(np.asarray(angles, dtype=np.float64))
    if scales.ndim != 1 or angles.ndim != 1 or not scales.size or not angles.size or (scales <= 0).any():
        raise ValueError("align_images_grid: 1-D lists of positive scales and of angles are needed")
    nf, npol = (2 if check_flip else 1), (2 if check_polarity else 1)
    planes = [p for m in imgs for p in ([m, m[::-1, :]] if check_flip else [m])]
    shape = (len(imgs), nf, npol, scales.size, angles.size)
    plane_ix = np.arange(len(planes)).reshape(len(imgs), nf, 1, 1, 1)
    cand_angle = angles.reshape(1, 1, 1, 1, -1) + 180.0 * np.arange(npol).reshape(1, 1, -1, 1, 1)
    pl, sc, an = (np.broadcast_to(v, shape).ravel() for v in (plane_ix, scales.reshape(1, 1, 1, -1, 1), cand_angle))
    best = []
    with AlignContext(image_ref, planes, device=device) as ctx:
        r = ctx.evaluate(sc, an, pl)
        scores = r.scores.reshape(shape)
        per = int(np.prod(shape[1:]))
        for i in range(len(imgs)):
            s = r.scores[i * per:(i + 1) * per]
            if np.isnan(s).all():
                best.append(AlignBest(False, 1.0, 0.0, np.zeros(2), float("nan")))
                continue
            k = i * per + int(np.nanargmax(s))
            b = AlignBest(bool(pl[k] % nf) if check_flip else False, float(sc[k]), float(an[k]), r.shifts[k].astype(np.float64), float(r.scores[k]))
            if refine:
                angle0 = 180.0 * np.unravel_index(k - i * per, shape[1:])[1]
                lo, hi = np.log(scales.min()), np.log(scales.max())
                x0 = [np.log(b.scale), b.angle - angle0]
                if hi > lo:
                    found = _search(ctx, int(pl[k]), (lo, hi), (angles.min(), angles.max()), (angle0,), x0=x0)
                elif angles.max() > angles.min():
                    found = _search(ctx, int(pl[k]), None, (angles.min(), angles.max()), (angle0,))
                else:
                    found = [1e10]
                if -found[0] > b.score:
                    b = AlignBest(b.flip, float(found[1]), float(found[2]), found[3], -found[0])
            best.append(b)
    return (best[0], scores[0]) if single else (best, scores)


# ------------------------------------------------------------------------------------------
# command line
# ------------------------------------------------------------------------------------------
def add_args(parser: argparse.ArgumentParser) -> argparse.ArgumentParser:
    parser.add_argument("moving", help=".mrc / .npy file with one 2-D image")
    parser.add_argument("ref", help="the reference image, no smaller than the moving one")
    parser.add_argument("--angle-range", type=float, default=180.0, help="angles -range ... +range, degrees")
    parser.add_argument("--angle-step", type=float, default=1.0)
    parser.add_argument("--scale-range", type=float, default=0.0, help="scales 1 - range ... 1 + range")
    parser.add_argument("--scale-step", type=float, default=0.01)
    parser.add_argument("--no-flip", action="store_true")
    parser.add_argument("--no-polarity", action="store_true")
    parser.add_argument("--refine", action="store_true", help="run the reference's optimiser from the grid's best")
    parser.add_argument("--out", default=None, help=".mrc file for the aligned, untapered moving image")
    parser.add_argument("--device", type=int, default=0)
    return parser


def _image(path):
    d = np.squeeze(np.asarray(_read_map(path)[0]))
    if d.ndim != 2:
        raise SystemExit(f"{path}: one 2-D image is needed; got shape {d.shape}")
    return d


def _axis(rng, step):
    if rng < 0 or step <= 0:
        raise SystemExit("ranges must be >= 0 and steps > 0")
    k = int(np.floor(rng / step + 1e-9))
    return np.arange(-k, k + 1, dtype=np.float64) * step


def run(args, grid_fn=None) -> dict:
    """``grid_fn`` stands in for ``align_images_grid`` (tests)."""
    mov, ref = _image(args.moving), _image(args.ref)
    angles, scales = _axis(args.angle_range, args.angle_step), 1.0 + _axis(args.scale_range, args.scale_step)
    if (scales <= 0).any():
        raise SystemExit("--scale-range must be below 1")
    t0 = time.perf_counter()
    try:
        best, scores = (grid_fn or align_images_grid)(mov, ref, scales, angles, check_polarity=not args.no_polarity, check_flip=not args.no_flip,
                                                     refine=args.refine, device=args.device)
    except ValueError as e:
        raise SystemExit(str(e))
    report = {
        "images": dict(moving=str(args.moving), ref=str(args.ref), moving_shape=list(mov.shape), ref_shape=list(ref.shape)),
        "candidates": int(np.asarray(scores).size), "angles": int(angles.size), "scales": int(scales.size),
        "best": dict(flip=bool(best.flip), scale=float(best.scale), angle=float(best.angle), shift=[float(v) for v in best.shift],
                     score=float(best.score)),
        "seconds": time.perf_counter() - t0,
    }
    if args.out:
        from .mrc import write_mrc

        with AlignContext(ref, [mov[::-1, :] if best.flip else mov], device=args.device) as ctx:
            write_mrc(args.out, ctx.aligned(best.scale, best.angle, best.shift, 0, "image"), 1.0)
    return report


def main(argv=None) -> int:
    args = add_args(argparse.ArgumentParser(prog="helicon_amd.align", description=__doc__.split("\n\n")[0])).parse_args(argv)
    json.dump(run(args), sys.stdout, indent=1)
    sys.stdout.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
