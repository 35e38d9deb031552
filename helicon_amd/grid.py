"""Host-side logic of the sweep driver: candidate grid, candidate filter, Fourier masks.

Mirrors the headless part of the reference's ``run_denovo3D_reconstruction``
(src/helicon/webApps/denovo3D/app.py:2286-2452): axes are ``np.arange(min, max + step/2, step)``
(app.py:2319-2334), candidates are ``itertools.product(twists, rises)`` (app.py:2336-2338) for one
csym at a time, twist is wrapped to [-180, 180] and rounded to 6 decimals (app.py:2360) and
candidates with a tiny twist / tiny rise / too large rise are skipped (app.py:2389-2403).
"""
from __future__ import annotations

import itertools
import math
from dataclasses import dataclass

import numpy as np

__all__ = [
    "set_to_periodic_range",
    "sweep_axis",
    "CandidateGrid",
    "build_grid",
    "radial_band_mask",
    "layer_line_mask",
    "shard_bounds",
    "zoom_spec",
    "filter_spec",
    "phase_spec",
]


def set_to_periodic_range(v: float, min: float = -180, max: float = 180) -> float:
    """src/helicon/lib/angular.py:84-110."""
    if min <= v <= max:
        return v
    tmp = math.fmod(v - min, max - min)
    if tmp >= 0:
        tmp += min
    else:
        tmp += max
    return tmp


def sweep_axis(vmin: float, vmax: float, step: float) -> np.ndarray:
    if vmin < vmax:
        return np.arange(vmin, vmax + step / 2, step)
    return np.array([vmin], dtype=np.float64)


@dataclass
class CandidateGrid:
    """Flat candidate list, csym-major then twist then rise: g = (c*T + t)*R + r."""

    twists: np.ndarray
    rises: np.ndarray
    csyms: np.ndarray
    params: np.ndarray  # [G, 4] float64: twist (wrapped, rounded), rise, csym, rot
    valid: np.ndarray   # [G] bool — False where the reference's driver skips the pair

    @property
    def shape(self):
        return (len(self.csyms), len(self.twists), len(self.rises))

    def __len__(self):
        return len(self.params)

    def unravel(self, g: int):
        c, t, r = np.unravel_index(int(g), self.shape)
        return int(c), int(t), int(r)


def build_grid(twists, rises, csyms=(1,), *, tube_length: float, rot: float = 0.0) -> CandidateGrid:
    twists = np.atleast_1d(np.asarray(twists, dtype=np.float64))
    rises = np.atleast_1d(np.asarray(rises, dtype=np.float64))
    csyms = np.atleast_1d(np.asarray(csyms, dtype=np.int64))
    if (csyms < 1).any():
        raise ValueError("csym must be >= 1")
    tw = np.array([np.round(set_to_periodic_range(float(t), min=-180, max=180), 6) for t in twists])
    pairs = np.array(list(itertools.product(tw, rises)), dtype=np.float64).reshape(-1, 2)
    ok = ~((np.abs(pairs[:, 0]) < 0.01) | (np.abs(pairs[:, 1]) < 0.01) | (np.abs(pairs[:, 1]) >= tube_length / 2))
    n = len(pairs)
    params = np.empty((len(csyms) * n, 4), dtype=np.float64)
    for k, c in enumerate(csyms):
        params[k * n:(k + 1) * n, 0:2] = pairs
        params[k * n:(k + 1) * n, 2] = float(c)
    params[:, 3] = rot
    return CandidateGrid(twists, rises, csyms, params, np.tile(ok, len(csyms)))


def radial_band_mask(ny: int, nx: int, r_lo: float = 2.0, r_hi: float | None = None) -> np.ndarray:
    """``r_lo < r < r_hi`` on the fftshifted plane, r in pixels from DC at [ny//2, nx//2];
    default ``r_hi = min(ny, nx)//2 - 1``."""
    if r_hi is None:
        r_hi = min(ny, nx) // 2 - 1
    ky = (np.arange(ny) - ny // 2).astype(np.float64)
    kx = (np.arange(nx) - nx // 2).astype(np.float64)
    r2 = ky[:, None] ** 2 + kx[None, :] ** 2
    return (r2 > r_lo * r_lo) & (r2 < r_hi * r_hi)


def layer_line_mask(ny, nx, r_lo=2.0, r_hi=None, axial_bins=None, half_width=1) -> np.ndarray:
    """Radial band intersected with layer lines.  The helical axis is the image column axis, so a
    layer line is a COLUMN of the fftshifted plane at axial frequency ``+-axial_bins[j]`` bins."""
    m = radial_band_mask(ny, nx, r_lo, r_hi)
    if axial_bins is None:
        return m
    kx = np.abs(np.arange(nx) - nx // 2)
    sel = np.zeros(nx, dtype=bool)
    for b in axial_bins:
        sel |= np.abs(kx - int(b)) <= half_width
    return m & sel[None, :]


def shard_bounds(n_items: int, rank: int, world: int, align: int = 1) -> tuple[int, int, int]:
    """Contiguous block partition of the flat candidate index:
    rank k owns [k*per, min(G, (k+1)*per)), per = ceil(G/W) rounded up to a multiple of ``align``
    (the number of rises: shards then start on a twist, which keeps every shard a list of whole
    shared-twist runs for the library's fused pass).  Returns (lo, hi, per_rank)."""
    per = -(-n_items // world)
    if align > 1:
        per = -(-per // align) * align
    lo = min(n_items, rank * per)
    hi = min(n_items, lo + per)
    return lo, hi, per


_ZOOM_MIN_SIDE, _ZOOM_MAX_SIDE = 8, 1024


def zoom_spec(shape, apix, cutoff_res=None, output_size=None):
    """The Fourier sampling that ``compute_power_spectra(img, apix, cutoff_res, output_size)`` asks of the sweep
    (transforms.py:663-713): ``None`` for the default sampling, ``(ony, onx, cutoff_y, cutoff_x)`` for a zoom.

    The default sampling is ``cutoff_res`` ``None`` or ``(2 apix, 2 apix)`` together with ``output_size`` ``None`` or the
    image's own shape (on an odd side the reference's transform differs from the FFT by a phase only, and the sweep reads
    amplitudes): such arguments take the sweep's standard pipelines unchanged.  ``ValueError`` on a spectrum side outside
    [8, 1024] or a cutoff that is not a positive finite number."""
    ny, nx = (int(v) for v in shape)
    if not apix > 0:
        raise ValueError(f"apix must be positive; got {apix}")
    if cutoff_res is None:
        cy = cx = 2.0 * float(apix)
    else:
        if np.size(cutoff_res) != 2:
            raise ValueError(f"cutoff_res must be (cutoff_y, cutoff_x) in Angstrom; got {cutoff_res!r}")
        cy, cx = (float(v) for v in cutoff_res)
    if not (cy > 0 and cx > 0 and math.isfinite(cy) and math.isfinite(cx)):
        raise ValueError(f"cutoff_res must be positive and finite; got ({cy}, {cx})")
    if output_size is None:
        ony, onx = ny, nx
    else:
        if np.size(output_size) != 2:
            raise ValueError(f"output_size must be (ony, onx); got {output_size!r}")
        oy, ox = output_size
        if oy != int(oy) or ox != int(ox):
            raise ValueError(f"output_size must be whole numbers; got {output_size!r}")
        ony, onx = int(oy), int(ox)
    if not (_ZOOM_MIN_SIDE <= ony <= _ZOOM_MAX_SIDE and _ZOOM_MIN_SIDE <= onx <= _ZOOM_MAX_SIDE):
        raise ValueError(f"output_size must lie in [{_ZOOM_MIN_SIDE}, {_ZOOM_MAX_SIDE}] per side; got ({ony}, {onx})")
    if (cy, cx) == (2.0 * float(apix), 2.0 * float(apix)) and (ony, onx) == (ny, nx):
        return None
    return ony, onx, cy, cx


def filter_spec(low_pass_fraction=0, high_pass_fraction=0):
    """The spectrum filter that ``compute_power_spectra(..., low_pass_fraction, high_pass_fraction)`` asks of the sweep
    (transforms.py:811-816): ``None`` when both passes are off, else ``(low_pass_fraction, high_pass_fraction)`` with 0.0
    for a pass that is off.  A fraction outside (0, 1) is off, the reference's own rule (filters.py:363-370); ``None``
    counts as 0.  ``ValueError`` on NaN."""
    out = []
    for name, f in (("low_pass_fraction", low_pass_fraction), ("high_pass_fraction", high_pass_fraction)):
        f = 0.0 if f is None else float(f)
        if math.isnan(f):
            raise ValueError(f"{name} is NaN")
        out.append(f if 0.0 < f < 1.0 else 0.0)
    return None if out == [0.0, 0.0] else (out[0], out[1])


def phase_spec(weight=0):
    """The weight of the phase score across the meridian in the sweep's score, ``(1 - weight) * amplitude Pearson + weight *
    phase score``: ``None`` when it is off (0 or ``None``), else the weight as a float in (0, 1].  ``ValueError`` on NaN or a
    value outside [0, 1]."""
    w = 0.0 if weight is None else float(weight)
    if math.isnan(w) or not 0.0 <= w <= 1.0:
        raise ValueError(f"phase_weight must lie in [0, 1]; got {weight!r}")
    return None if w == 0.0 else w
