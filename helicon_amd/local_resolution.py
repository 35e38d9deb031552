"""Local resolution of two half maps: the Fourier shell correlation of overlapping windows, on the device.

The reference has no local-resolution function; this one is a composition of its rules.  For an even ``window = w`` and a
``step = s`` the centres along an axis of length N are ``s // 2 + i s <= N - 1`` (``window_centres``); the window at centre
``c`` is ``get_clip3d(map, c - w // 2, ..., w, w, w)`` (lib/transforms.py:516-555: zeros outside the map) times
``t[z] t[y] t[x]`` with ``t`` the one-axis profile of ``generate_tapering_filter`` (lib/filters.py:415-466,
``taper_profile``); its curve ``fsc[0 .. w / 2]`` is ``calc_fsc_per_shell``'s (lib/analysis.py:235-290); its resolution is the
first crossing of ``threshold`` from shell 1 on, linearly interpolated as commands/trueFSC.py:427-462 does
(``resolution_from_curve``): Nyquist, ``2 apix``, when no shell is below, ``w apix`` when shell 1 already is.  There is no 999.

``LocalFSC`` keeps both maps on the device (``hh_lres_*``, csrc/local_resolution.inc); only the centres and the taper go up
and only the results come back.  Two routes give the curves: ``"lds"`` (w <= 24: one workgroup per window pair, both half
spectra in LDS; what ``"auto"`` takes there) and ``"passes"`` (any w in [8, 64]: gathered windows through ``calc_fsc``'s
passes).  Each route is bit-identical from run to run and independent of the order of the centres; the two routes round
differently.  Precision: float32 transforms, float64 shell sums, ratio and crossing rule.

    python -m helicon_amd.local_resolution half1.mrc half2.mrc --window 24 --step 4 [--threshold 0.5] [--mask m.mrc] [--apix A]
                                           [--out locres.mrc] [--grid-out grid.npy] [--route auto] [--device 0]

reads two maps of one shape (``.mrc`` / ``.map`` / ``.npy``; the header's voxel size unless ``--apix``), prints a JSON report
(grid shape, route, minimum / median / maximum and a ten-bin histogram of the evaluated windows, ``kernel_ms``) and writes the
full-size map (``--out``, with the input's voxel size) and / or the grid of window values (``--grid-out``).
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import sys

import numpy as np

from . import _lib
from .fsc import _f32, _read_map

__all__ = ["LocalFSC", "LocalResolution", "local_resolution", "taper_profile", "window_centres", "resolution_from_curve",
           "lds_bytes", "upsample_grid", "main"]

_MIN_SIDE, _MAX_SIDE = 8, 512
_MIN_W, _MAX_W, _MAX_LDS_W = 8, 64, 24
_ROUTES = {"auto": 0, "lds": 1, "passes": 2}
_ROUTE_NAMES = {1: "lds", 2: "passes"}
_f32p, _f64p, _i32p = C.POINTER(C.c_float), C.POINTER(C.c_double), C.POINTER(C.c_int32)


# ------------------------------------------------------------------------------------------
# the three rules, on the host
# ------------------------------------------------------------------------------------------
def taper_profile(w, fraction_start=0.5, fraction_slope=0.5):
    """One axis of ``generate_tapering_filter`` (lib/filters.py:415-466) for a length ``w``: float32 ``[w]``; all ones when
    ``fraction_start`` is outside (0, 1)."""
    w = int(w)
    if not (0 < fraction_start < 1):
        return np.ones(w, dtype=np.float32)
    y = np.arange(0, w, dtype=np.float32) - w // 2
    y = np.abs(y / (w // 2))
    inner = y < fraction_start
    outer = y > fraction_start + fraction_slope
    y = (y - fraction_start) / fraction_slope
    y = (1.0 + np.cos(y * np.pi)) / 2.0
    y[inner] = 1
    y[outer] = 0
    return np.ascontiguousarray(y, dtype=np.float32)


def window_centres(n, step):
    """``step // 2 + i step`` for every ``i >= 0`` with a centre ``<= n - 1``."""
    n, step = int(n), int(step)
    if step < 1 or n < 1:
        raise ValueError(f"window_centres: n and step must be >= 1; got {n}, {step}")
    return np.arange(step // 2, n, step, dtype=np.int64)


def resolution_from_curve(fsc, w, apix, threshold=0.5):
    """The crossing rule: ``k*`` is the smallest ``k >= 1`` with ``fsc[k] < threshold``; Nyquist when there is none,
    ``w apix`` when ``k* = 1``, else the linear interpolation between shells ``k* - 1`` and ``k*``."""
    f = np.asarray(fsc, dtype=np.float64)
    w = int(w)
    if f.shape != (w // 2 + 1,):
        raise ValueError(f"resolution_from_curve: a curve of {w // 2 + 1} shells is needed; got {f.shape}")
    box = float(w) * float(apix)
    below = np.flatnonzero(f[1:] < threshold)
    if below.size == 0:
        return float(1.0 / (float(w // 2) / box))
    k = int(below[0]) + 1
    if k == 1:
        return box
    s0, s1 = float(k - 1) / box, float(k) / box
    x = s0 + (threshold - f[k - 1]) * (s1 - s0) / (f[k] - f[k - 1])
    return float(1.0 / x)


def lds_bytes(w, route="auto"):
    """LDS bytes of one workgroup of the ``"lds"`` route at window ``w`` (``hh_lres_plan``: host arithmetic, no device)."""
    out = C.c_int64(0)
    _lib.check(_lib.lib().hh_lres_plan(int(w), _route_code(route), 0, 0, None, C.byref(out), None), None)
    return int(out.value)


def upsample_grid(grid, step, shape, *, device=0):
    """The full-size float32 map of a grid of window values (``hh_lres_upsample``): trilinear between the centres, NaN
    corners dropped and the other weights renormalised, NaN where nothing evaluated remains."""
    g = np.ascontiguousarray(grid, dtype=np.float64)
    shape = tuple(int(v) for v in shape)
    if g.ndim != 3 or len(shape) != 3:
        raise ValueError(f"upsample_grid: a 3-D grid and a 3-D shape are needed; got {g.shape} and {shape}")
    out = np.empty(shape, dtype=np.float32)
    _lib.check(_lib.lib().hh_lres_upsample(int(device), g.ctypes.data_as(_f64p), *g.shape, int(step), *shape, out.ctypes.data_as(_f32p)), None)
    return out


def _route_code(route):
    try:
        return _ROUTES[route]
    except (KeyError, TypeError):
        raise ValueError(f"route must be one of {sorted(_ROUTES)}; got {route!r}") from None


# ------------------------------------------------------------------------------------------
# the context
# ------------------------------------------------------------------------------------------
class LocalResolution:
    """What ``LocalFSC.run`` returns: ``centres`` (three int arrays: z, y, x), ``resolution`` (float64 grid, NaN where a window
    was not evaluated), ``curves`` (``[gz, gy, gx, w // 2 + 1]`` float64, NaN rows where not evaluated; or None), ``route``
    (``"lds"`` / ``"passes"``), ``kernel_ms``, and ``resolution_map()``."""

    def __init__(self, centres, resolution, curves, route, kernel_ms, step, shape, device):
        self.centres, self.resolution, self.curves = centres, resolution, curves
        self.route, self.kernel_ms = route, kernel_ms
        self.step, self.shape, self.device = step, shape, device

    def resolution_map(self):
        """The full-size float32 map, computed on the device from the grid."""
        return upsample_grid(self.resolution, self.step, self.shape, device=self.device)


class LocalFSC:
    """Two half maps of one shape (every side in [8, 512]) resident on the device; a context manager."""

    def __init__(self, half1, half2, *, device=0):
        a, b = np.asarray(half1), np.asarray(half2)
        if a.ndim != 3 or a.shape != b.shape:
            raise ValueError(f"LocalFSC: two 3-D maps of one shape are needed; got {a.shape} and {b.shape}")
        if min(a.shape) < _MIN_SIDE or max(a.shape) > _MAX_SIDE:
            raise ValueError(f"LocalFSC: every side must lie in [{_MIN_SIDE}, {_MAX_SIDE}]; got {a.shape}")
        a, b = _f32(a, "LocalFSC"), _f32(b, "LocalFSC")
        self.shape, self.device = tuple(int(v) for v in a.shape), int(device)
        self._ctx = C.c_void_p()
        _lib.check(_lib.lib().hh_lres_create(C.byref(self._ctx), self.device, a.ctypes.data_as(_f32p), b.ctypes.data_as(_f32p), *self.shape), None)

    def close(self):
        if getattr(self, "_ctx", None):
            _lib.lib().hh_lres_destroy(self._ctx)
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

    def set_budget(self, scratch_bytes=0, max_windows_per_launch=0):
        """Caps of the later runs (0: the defaults): tests cross every chunk cut with them at small sizes."""
        _lib.check(_lib.lib().hh_lres_set_budget(self._ctx, int(scratch_bytes), int(max_windows_per_launch)), None)

    def run_centres(self, apix, window, centres, threshold=0.5, taper=(0.5, 0.5), return_curves=False, route="auto"):
        """The windows around a list of centres ``[n, 3]`` (z, y, x): ``(resolution [n], curves [n, w // 2 + 1] or None, route,
        kernel_ms)``."""
        if not self._ctx:
            raise _lib.HeliconHipError("LocalFSC: the context is closed")
        w = int(window)
        if w != window or w < _MIN_W or w > _MAX_W or w % 2:
            raise ValueError(f"LocalFSC: the window must be even and lie in [{_MIN_W}, {_MAX_W}]; got {window}")
        cen = np.ascontiguousarray(centres, dtype=np.int32)
        if cen.ndim != 2 or cen.shape[1] != 3 or cen.shape[0] < 1:
            raise ValueError(f"LocalFSC: centres [n, 3] with n >= 1 are needed; got {cen.shape}")
        t = taper_profile(w, float(taper[0]), float(taper[1]))
        n = cen.shape[0]
        res = np.empty(n, dtype=np.float64)
        curves = np.empty((n, w // 2 + 1), dtype=np.float64) if return_curves else None
        code = _route_code(route)
        taken, ms = C.c_int32(0), C.c_double(0.0)
        lib = _lib.lib()
        _lib.check(lib.hh_lres_plan(w, code, 0, 0, C.byref(taken), None, None), None)
        _lib.check(lib.hh_lres_run(self._ctx, w, t.ctypes.data_as(_f32p), cen.ctypes.data_as(_i32p), n, float(apix), float(threshold), code,
                                   res.ctypes.data_as(_f64p), curves.ctypes.data_as(_f64p) if return_curves else None, C.byref(ms)), None)
        return res, curves, _ROUTE_NAMES[int(taken.value)], float(ms.value)

    def run(self, apix, window, step, threshold=0.5, taper=(0.5, 0.5), mask=None, return_curves=False, route="auto"):
        step = int(step)
        if step < 1:
            raise ValueError(f"LocalFSC: step must be >= 1; got {step}")
        axes = tuple(window_centres(n, step) for n in self.shape)
        grid_shape = tuple(len(a) for a in axes)
        if min(grid_shape) == 0:
            raise ValueError(f"LocalFSC: step {step} leaves an axis of {self.shape} without a centre (step // 2 must be inside the map)")
        zz, yy, xx = np.meshgrid(*axes, indexing="ij")
        cen = np.stack([zz.ravel(), yy.ravel(), xx.ravel()], axis=1)
        keep = np.ones(len(cen), dtype=bool)
        if mask is not None:
            m = np.asarray(mask)
            if m.shape != self.shape:
                raise ValueError(f"LocalFSC: the mask must have the maps' shape {self.shape}; got {m.shape}")
            keep = m[cen[:, 0], cen[:, 1], cen[:, 2]].astype(bool)
        w = int(window)
        resolution = np.full(len(cen), np.nan, dtype=np.float64)
        curves = np.full((len(cen), w // 2 + 1), np.nan, dtype=np.float64) if return_curves else None
        taken, ms = None, 0.0
        if keep.any():
            r, c, taken, ms = self.run_centres(apix, window, cen[keep], threshold, taper, return_curves, route)
            resolution[keep] = r
            if return_curves:
                curves[keep] = c
        else:   # nothing to evaluate: the arguments are still checked, and the route named
            t = C.c_int32(0)
            _lib.check(_lib.lib().hh_lres_plan(w, _route_code(route), 0, 0, C.byref(t), None, None), None)
            taken = _ROUTE_NAMES[int(t.value)]
        return LocalResolution(axes, resolution.reshape(grid_shape), curves.reshape(grid_shape + (w // 2 + 1,)) if return_curves else None,
                               taken, ms, step, self.shape, self.device)


def local_resolution(half1, half2, apix, *, device=0, **kw):
    """``LocalFSC(half1, half2).run(apix, **kw)`` in one call."""
    with LocalFSC(half1, half2, device=device) as ctx:
        return ctx.run(apix, **kw)


# ------------------------------------------------------------------------------------------
# command line
# ------------------------------------------------------------------------------------------
def add_args(parser: argparse.ArgumentParser) -> argparse.ArgumentParser:
    parser.add_argument("half1", help=".mrc / .map / .npy file with one 3-D map")
    parser.add_argument("half2", help="the second map, of the same shape")
    parser.add_argument("--window", type=int, required=True, help="even window side, 8 ... 64")
    parser.add_argument("--step", type=int, required=True, help="distance between window centres, voxels")
    parser.add_argument("--threshold", type=float, default=0.5)
    parser.add_argument("--mask", default=None, help="map of the same shape; windows whose centre voxel is <= 0.5 are skipped")
    parser.add_argument("--apix", type=float, default=None, help="voxel size, Angstrom (default: the first map's MRC header)")
    parser.add_argument("--out", default=None, help=".mrc file for the full-size local resolution map")
    parser.add_argument("--grid-out", default=None, help=".npy file for the grid of window values")
    parser.add_argument("--route", choices=sorted(_ROUTES), default="auto")
    parser.add_argument("--device", type=int, default=0)
    return parser


def run(args, run_fn=None) -> dict:
    """``run_fn(half1, half2, apix, **kw)`` stands in for ``local_resolution`` (tests)."""
    m1, apix = _read_map(args.half1, args.apix)
    m2, _ = _read_map(args.half2, args.apix)
    if not apix or apix <= 0:
        raise SystemExit("--apix is required (the maps carry no voxel size)")
    if m1.ndim != 3 or m1.shape != m2.shape:
        raise SystemExit(f"two 3-D maps of one shape are needed; got {tuple(m1.shape)} and {tuple(m2.shape)}")
    mask = None
    if args.mask:
        mask = np.asarray(_read_map(args.mask)[0]) > 0.5
    try:
        r = (run_fn or local_resolution)(m1, m2, float(apix), window=args.window, step=args.step, threshold=args.threshold, mask=mask,
                                         route=args.route, device=args.device)
    except ValueError as e:
        raise SystemExit(str(e))
    vals = r.resolution[np.isfinite(r.resolution)]
    report = {
        "maps": dict(half1=str(args.half1), half2=str(args.half2), shape=[int(v) for v in m1.shape], apix=float(apix)),
        "window": int(args.window), "step": int(args.step), "threshold": float(args.threshold),
        "grid": [int(v) for v in r.resolution.shape], "route": r.route,
        "windows": int(r.resolution.size), "evaluated": int(vals.size),
        "kernel_ms": float(r.kernel_ms),
    }
    if vals.size:
        counts, edges = np.histogram(vals, bins=10)
        report.update(min=float(vals.min()), median=float(np.median(vals)), max=float(vals.max()),
                      histogram=dict(edges=[float(v) for v in edges], counts=[int(v) for v in counts]))
    if args.grid_out:
        np.save(args.grid_out, r.resolution)
    if args.out:
        from .mrc import write_mrc

        write_mrc(args.out, r.resolution_map(), float(apix))
    return report


def main(argv=None) -> int:
    args = add_args(argparse.ArgumentParser(prog="helicon_amd.local_resolution", description=__doc__.split("\n\n")[0])).parse_args(argv)
    json.dump(run(args), sys.stdout, indent=1)
    sys.stdout.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
