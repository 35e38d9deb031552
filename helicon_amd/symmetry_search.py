"""Helical symmetry search of a 3-D map: which (twist, rise, Csym) does this map have?

For every candidate the map ``V`` is helically symmetrised on its own grid and compared with itself,

    S     = apply_helical_symmetry(V, apix, twist, rise, csym, fraction, new_size=V.shape, new_apix=apix)
    score = cross_correlation_coefficient(V[M], S[M])          # Pearson; 0 where either side has no variance

(the reference's operator, lib/transforms.py:58-165) over a scored region ``M`` given on voxel indices::

    M = {(k, j, i): rmin**2 <= (j - ny//2)**2 + (i - nx//2)**2 < rmax**2  and  -h <= k - nz//2 < h}
    rmax None: no outer limit;   z_fraction >= 1: every plane, else h = max(1, int(nz * z_fraction + 0.5) // 2)

and the true symmetry is the peak over the (Csym x twist x rise) grid.  The map is uploaded once (``SymmetrySearch``), a
candidate costs its gathers over ``M`` and three sums, the symmetrised map is never stored (csrc/symmetry_search.inc).

    python -m helicon_amd.symmetry_search map.mrc [--apix A] --twist MIN MAX STEP --rise MIN MAX STEP [--csym 1 2 3]
           [--fraction F] [--rmin PX] [--rmax PX] [--z-fraction F] [--device 0] [--top 10] [--out scores.npz]
           [--resample NZ NY NX]

reads a ``.mrc`` / ``.map`` / ``.npy`` map (the header's voxel size unless ``--apix``), prints a JSON report in
``denovo3DBatch``'s layout (``n_candidates``, ``n_skipped``, ``best``, ``top``, and the region written out) and, with
``--out``, saves ``scores[C, T, R]``, ``twists``, ``rises``, ``csyms``, ``params``, ``valid``.  The grid and its skipped
pairs are those of the 2-D sweep (``grid.build_grid`` with the map's length nz * apix as the tube length).  With
``--resample`` the map is first Fourier-resampled to those sides on the device (``fft_resample`` with ``output="real"``;
even sides and one ratio for all three axes only); the report's ``map`` entry then shows the new shape and voxel size
and adds ``resampled_from``.  The report's ``best`` is what
``python -m helicon_amd.denovo3DBatch map.mrc --from-map TWIST RISE CSYM`` takes as the map's symmetry.
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import math
import sys

import numpy as np

from . import _lib
from .grid import build_grid, sweep_axis

__all__ = ["SymmetrySearch", "helical_symmetry_search", "default_rmax", "region_spec", "main"]

_MIN_SIDE, _MAX_SIDE = 2, 1024


def default_rmax(shape) -> int:
    """The default outer radius of the scored region, in voxels: ``min(ny, nx) // 2 - 1``."""
    return min(int(shape[1]), int(shape[2])) // 2 - 1


def region_spec(shape, rmin=0, rmax=Ellipsis, z_fraction=0.5):
    """The scored region ``M`` of a map of this shape, as the device is told about it: a dict with ``rmin``, ``rmax``
    (``None``: no outer limit; ``...``: the default ``min(ny, nx) // 2 - 1``), ``z_fraction``, the planes ``k_range`` =
    [k0, k1), ``plane_voxels`` (in-plane voxels of the shell) and ``region_voxels`` = |M|.  ``ValueError`` on an empty
    region or a bad argument."""
    nz, ny, nx = (int(v) for v in shape)
    if rmax is Ellipsis:
        rmax = default_rmax((nz, ny, nx))
    rmin, z_fraction = float(rmin), float(z_fraction)
    if not rmin >= 0 or (rmax is not None and math.isnan(float(rmax))) or not z_fraction > 0:
        raise ValueError(f"region: rmin must be >= 0, rmax a number or None, z_fraction > 0; got {rmin}, {rmax}, {z_fraction}")
    if rmax is not None and float(rmax) < 0:
        raise ValueError(f"region: rmax must be >= 0 (None: no outer limit); got {rmax}")
    jj = (np.arange(ny, dtype=np.int64) - ny // 2)[:, None]
    ii = (np.arange(nx, dtype=np.int64) - nx // 2)[None, :]
    r2 = (jj * jj + ii * ii).astype(np.float64)
    shell = r2 >= rmin * rmin
    if rmax is not None:
        shell &= r2 < float(rmax) * float(rmax)
    if z_fraction >= 1:
        k0, k1 = 0, nz
    else:
        h = max(1, int(nz * z_fraction + 0.5) // 2)
        k0, k1 = max(0, nz // 2 - h), min(nz, nz // 2 + h)
    plane = int(shell.sum())
    if plane == 0 or k1 <= k0:
        raise ValueError(f"region: rmin {rmin}, rmax {rmax}, z_fraction {z_fraction} select no voxel of a {nz} x {ny} x {nx} map")
    return dict(rmin=rmin, rmax=None if rmax is None else float(rmax), z_fraction=z_fraction, k_range=(k0, k1),
                plane_voxels=plane, region_voxels=plane * (k1 - k0))


def _volume(data, name):
    d = np.asarray(data)
    if d.ndim != 3:
        raise ValueError(f"{name}: data must be a 3D map (nz, ny, nx); got {d.ndim} dimension(s)")
    if d.dtype.kind not in "biuf":
        raise ValueError(f"{name}: data must be real; got dtype {d.dtype}")
    if min(d.shape) < _MIN_SIDE or max(d.shape) > _MAX_SIDE:
        raise ValueError(f"{name}: every side must lie in [{_MIN_SIDE}, {_MAX_SIDE}]; got {d.shape}")
    vol = np.ascontiguousarray(d, dtype=np.float32)
    if not np.isfinite(vol).all():
        raise ValueError(f"{name}: the map holds NaN or infinite values")
    return vol


class SymmetrySearch:
    """A map on the device, ready to score lists of (twist, rise, csym) candidates (a context manager around ``hh_hs``).

    ``fraction`` is the operator's (the central part of the map's occupied z range that is read as the source).
    ``partial_bytes`` bounds the device memory one launch may take for its partial sums (default 64 MiB, or the
    environment's ``HELICON_HS_PARTIAL_BYTES``): a longer list is cut into several launches; the scores do not depend on
    it.  The default region (``set_region()``'s defaults) is set when the map allows one."""

    def __init__(self, data, apix, *, fraction=1.0, device=0, partial_bytes=None):
        vol = _volume(data, "SymmetrySearch")
        if not float(apix) > 0 or not float(fraction) > 0:
            raise ValueError(f"SymmetrySearch: apix and fraction must be positive; got {apix}, {fraction}")
        self.shape, self.apix, self.fraction, self.device = tuple(vol.shape), float(apix), float(fraction), int(device)
        self._h = None
        self._L = _lib.lib()
        h = C.c_void_p()
        shape = (C.c_int32 * 3)(*vol.shape)
        self._check(self._L.hh_hs_create(C.byref(h), self.device, vol.ctypes.data_as(C.POINTER(C.c_float)), shape, self.apix,
                                         self.fraction), None)
        self._h = h
        self.region = None
        try:
            self.region = region_spec(self.shape)
        except ValueError:
            pass   # a map too small for the default region: set_region() before search()
        if partial_bytes is not None:
            self._check(self._L.hh_hs_set_budget(self._h, int(partial_bytes)), self._h)

    def _check(self, rc, h):
        if rc == 0:
            return
        msg = self._L.hh_hs_last_error(h)
        kind = ValueError if rc == -1 else _lib.HeliconHipError
        raise kind(f"libhelicon_hip error {rc}: {msg.decode() if msg else '?'}")

    def close(self):
        if self._h is not None:
            self._L.hh_hs_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _handle(self):
        if self._h is None:
            raise _lib.HeliconHipError("SymmetrySearch: the handle is closed")
        return self._h

    def set_region(self, rmin=0, rmax=Ellipsis, z_fraction=0.5):
        """The scored region (module docstring); ``rmax=None``: no outer limit, left out: ``min(ny, nx) // 2 - 1``."""
        spec = region_spec(self.shape, rmin, rmax, z_fraction)
        self._check(self._L.hh_hs_set_region(self._handle(), spec["rmin"], -1.0 if spec["rmax"] is None else spec["rmax"],
                                             spec["z_fraction"]), self._h)
        self.region = spec
        return spec

    def search(self, params) -> np.ndarray:
        """params [G, 3] (twist degrees, rise Angstrom, csym) -> scores [G] float32."""
        p = np.ascontiguousarray(params, dtype=np.float64)
        if p.ndim != 2 or p.shape[1] != 3:
            raise ValueError(f"SymmetrySearch.search: params must be [G, 3] (twist, rise, csym); got {p.shape}")
        scores = np.empty(len(p), dtype=np.float32)
        self._check(self._L.hh_hs_search(self._handle(), p.ctypes.data_as(C.POINTER(C.c_double)), len(p),
                                         scores.ctypes.data_as(C.POINTER(C.c_float))), self._h)
        return scores

    def _info(self):
        z = (C.c_int32 * 2)()
        n, launches = C.c_int64(0), C.c_int64(0)
        self._check(self._L.hh_hs_info(self._handle(), z, C.byref(n), C.byref(launches)), self._h)
        return (int(z[0]), int(z[1])), int(n.value), int(launches.value)

    @property
    def z_range(self):
        """The source planes [z0, z1) the operator reads: the 1 % profile rule and ``fraction`` (transforms.py:92-99)."""
        return self._info()[0]

    @property
    def region_voxels(self) -> int:
        return self._info()[1]

    @property
    def launches(self) -> int:
        """Scoring launches since the handle was created (a list cut by ``partial_bytes`` takes several)."""
        return self._info()[2]

    @property
    def kernel_ms(self) -> float:
        """Device time of the last search's kernels, all launches."""
        ms = C.c_double(0.0)
        self._check(self._L.hh_hs_kernel_ms(self._handle(), C.byref(ms)), self._h)
        return ms.value


def helical_symmetry_search(data, apix, twists, rises, csyms=(1,), *, fraction=1.0, rmin=0, rmax=Ellipsis, z_fraction=0.5,
                            device=0, engine=None):
    """Score every (csym, twist, rise) candidate symmetry of a 3-D map on one GPU; returns the sweep's ``SweepResult``
    with one segment (``scores[1, C, T, R]``, skipped pairs -inf, ``best[0]`` = (twist, rise, csym, score)).

    The grid is ``grid.build_grid(twists, rises, csyms, tube_length=nz * apix)``: the 2-D sweep's order (csym-major,
    then twist, then rise) and its skipped pairs (|twist| < 0.01, |rise| < 0.01, rise >= length / 2), which take a
    harmless rise on the device and -inf in the result.  ``rmax`` left out is ``min(ny, nx) // 2 - 1``, ``None`` no
    outer limit.  ``engine``: a ``SymmetrySearch`` that already holds this map (it keeps the region it is given here)."""
    from .denovo3D import finish_sweep
    from .distributed import harmless_rise

    if engine is None:
        vol = _volume(data, "helical_symmetry_search")
        nz = vol.shape[0]
    else:
        nz = int(engine.shape[0])
    grid = build_grid(twists, rises, csyms, tube_length=nz * float(apix))
    params = grid.params[:, :3].copy()
    params[~grid.valid, 1] = harmless_rise(grid)   # skipped pairs still occupy a slot
    eng =engine if engine is not None else SymmetrySearch(vol, apix, fraction=fraction, device=device)
    try:
        eng.set_region(rmin, rmax, z_fraction)
        scores = eng.search(params)
    finally:
        if engine is None:
            eng.close()
    return finish_sweep(np.asarray(scores, dtype=np.float32)[None, :], grid)


# ------------------------------------------------------------------------------------------
# command line
# ------------------------------------------------------------------------------------------
def add_args(parser: argparse.ArgumentParser) -> argparse.ArgumentParser:
    parser.add_argument("map", help=".mrc / .map / .npy file with one 3-D map [nz, ny, nx], helical axis along z")
    parser.add_argument("--apix", type=float, default=None, help="voxel size, Angstrom (default: the MRC header's)")
    parser.add_argument("--twist", type=float, nargs=3, metavar=("MIN", "MAX", "STEP"), required=True)
    parser.add_argument("--rise", type=float, nargs=3, metavar=("MIN", "MAX", "STEP"), required=True)
    parser.add_argument("--csym", type=int, nargs="+", default=[1])
    parser.add_argument("--fraction", type=float, default=1.0,
                        help="central fraction of the map's length read as the source (apply_helical_symmetry's fraction)")
    parser.add_argument("--rmin", type=float, default=0.0, help="inner radius of the scored region, voxels")
    parser.add_argument("--rmax", type=float, default=None,
                        help="outer radius of the scored region, voxels (default min(ny, nx) // 2 - 1; negative: no limit)")
    parser.add_argument("--z-fraction", type=float, default=0.5, help="central fraction of the planes that is scored (>= 1: all)")
    parser.add_argument("--device", type=int, default=0)
    parser.add_argument("--top", type=int, default=10, help="how many best candidates to print")
    parser.add_argument("--out", default=None, help=".npz with scores[C, T, R], twists, rises, csyms, params, valid")
    parser.add_argument("--resample", type=int, nargs=3, metavar=("NZ", "NY", "NX"), default=None,
                        help="Fourier-resample the map to these sides before the search (even sides, one ratio for all axes)")
    return parser


def read_map(path, apix=None):
    """The map and its voxel size: ``.mrc`` / ``.map`` with the header's voxel size unless ``apix`` is given, else ``.npy``."""
    if str(path).lower().endswith((".mrc", ".mrcs", ".map")):
        from .mrc import read_mrc

        vol, header_apix = read_mrc(path)
        if apix is None:
            apix = header_apix
    else:
        vol = np.load(path)
    if vol.ndim != 3:
        raise SystemExit(f"the symmetry search needs a 3-D map; {path} has shape {tuple(vol.shape)}")
    if not apix or apix <= 0:
        raise SystemExit("--apix is required (the map carries no voxel size)")
    return vol, float(apix)


def resample_map(vol, apix, new_size, device=0, resampler=None):
    """The map at ``new_size`` and its voxel size, for ``--resample``.  Exits with a message on an odd side, old or new
    (the transform keeps a phase factor there, so the result is not a resampled map), and on unequal ratios old / new
    (the search takes one voxel size)."""
    old, new = tuple(int(v) for v in vol.shape), tuple(int(v) for v in new_size)
    if min(new) < 1:
        raise SystemExit(f"--resample: the new sides must be positive; got {new}")
    if any(v % 2 for v in old + new):
        raise SystemExit(f"--resample: every side must be even, old and new (an odd side keeps a phase factor: the result "
                         f"would not be a resampled map); got {old} -> {new}")
    if any(n * new[0] != old[0] * on for n, on in zip(old, new)):
        raise SystemExit(f"--resample: the three ratios old / new differ ({old} -> {new}): the search takes one voxel size")
    if resampler is None:
        from .fft_resample import fft_resample as resampler
    try:
        out, new_apix = resampler(vol, apix, new, output="real", device=device)
    except ValueError as e:
        raise SystemExit(str(e))
    return out, float(new_apix)


def run(args, engine_factory=None, resampler=None) -> dict:
    """``engine_factory(vol, apix, fraction=, device=)`` stands in for ``SymmetrySearch`` and
    ``resampler(vol, apix, new_size, output=, device=)`` for ``fft_resample`` (tests)."""
    vol, apix = read_map(args.map, args.apix)
    resampled_from = None
    if getattr(args, "resample", None):
        resampled_from = dict(shape=[int(v) for v in vol.shape], apix=apix)
        vol, apix = resample_map(np.asarray(vol), apix, args.resample, args.device, resampler)
    if any(c < 1 for c in args.csym):
        raise SystemExit(f"--csym must be >= 1; got {args.csym}")
    twists, rises = sweep_axis(*args.twist), sweep_axis(*args.rise)
    rmax = Ellipsis if args.rmax is None else (None if args.rmax < 0 else args.rmax)
    try:
        spec = region_spec(vol.shape, args.rmin, rmax, args.z_fraction)
        vol = _volume(vol, "symmetry_search")
        eng = (engine_factory or SymmetrySearch)(vol, apix, fraction=args.fraction, device=args.device)
    except ValueError as e:
        raise SystemExit(str(e))
    try:
        res = helical_symmetry_search(vol, apix, twists, rises, tuple(args.csym), fraction=args.fraction, rmin=args.rmin, rmax=rmax,
                                      z_fraction=args.z_fraction, device=args.device, engine=eng)
        z_range, region_voxels = eng.z_range, eng.region_voxels
    finally:
        eng.close()
    flat = res.scores.reshape(-1)
    order = np.argsort(-flat, kind="stable")[: args.top]   # score descending, like denovo3DBatch
    report = {
        "n_candidates": int(len(res.grid)), "n_skipped": int((~res.grid.valid).sum()),
        "map": dict(path=str(args.map), shape=[int(v) for v in vol.shape], apix=apix),
        "fraction": float(args.fraction), "z_range": [int(z_range[0]), int(z_range[1])],
        "region": dict(rmin=spec["rmin"], rmax=spec["rmax"], z_fraction=spec["z_fraction"], k_range=list(spec["k_range"])),
        "region_voxels": int(region_voxels),
        "best": dict(zip(("twist", "rise", "csym", "score"), res.best[0])),
        "top": [dict(twist=float(res.grid.params[g, 0]), rise=float(res.grid.params[g, 1]), csym=int(res.grid.params[g, 2]),
                     score=float(flat[g])) for g in order],
    }
    if resampled_from is not None:
        report["map"]["resampled_from"] = resampled_from
    if args.out:
        np.savez_compressed(args.out, scores=res.scores[0], twists=twists, rises=rises, csyms=np.asarray(args.csym),
                            params=res.grid.params, valid=res.grid.valid)
    return report


def main(argv=None) -> int:
    args = add_args(argparse.ArgumentParser(prog="helicon_amd.symmetry_search", description=__doc__.split("\n\n")[0])).parse_args(argv)
    json.dump(run(args), sys.stdout, indent=1)
    sys.stdout.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
