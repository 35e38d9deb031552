"""A probe that sees every row and column of the plane the zoomed, the filtered and the phase sweep score, on planes of
several output tiles: tests/spectrum_bands.py's band masks and geometry (``Probe``, ``band_masks``) on the scored plane,
the float64 oracle's band scores of every candidate per mode, and the probe's own sensitivity to a misplaced line.  No GPU
dependency: NumPy and the oracle only.

Why: k_zoom_sweep / k_phase_sweep work one 128 x 128 output tile at a time and the filter's x pass one 64 x 64 tile, each
with a host-built list of active tiles, a tile index decoded as (tile / tiles_v, tile % tiles_v), partial sums laid out
[segment][candidate][tile] and edge guards u < ony, v < onx.  Under oracle.path_b.radial_band_mask (r < min(ony, onx)//2 - 1)
no column with |kx| > 67 of a 136 x 264 plane enters a score, and a wrong line at a tile edge is one among thousands of
bins of one number.  Under the band masks every bin of the plane is in exactly one band per axis, and a band is a few
lines wide.

Modes (``MODES``): the amplitude spectrum as it is ("zoom"), low / high-pass filtered ("filter_lp_hp": 0.3, 0.05;
"filter_hp": 0, 0.05) — O.compute_power_spectra + O.cross_correlation_coefficient — and the phase map M across the meridian
("phase": phase_oracle.phase_map + O.cosine_similarity), every candidate simulated with the probe's own subunits.

Cases (``CASES``): the smallest planes at which each tile mechanism exists.  The zoomed cases take a 96 x 176 image at the
Nyquist cutoff, so the plane oversamples the image by less than 1.5: with the 3.4-fold oversampling of a 40 x 72 image at
cutoff (6, 5) apix neighbouring rows of the second image's candidate are too alike for a swap to show (6e-5 on the phase
map).

Sensitivity: for every band, every two adjacent lines (rows for axis 0, columns for axis 1) of the candidate's plane that
both lie in the band are swapped, and the smallest change of the band's score is kept; it must be at least MARGIN x
SCORE_TOL (tests/test_zoom_bands_host.py), for candidate 0 against ``probe.image`` and for ``probe.cand2`` against
``probe.image2``.
"""
from __future__ import annotations

import functools
from dataclasses import dataclass

import numpy as np

import phase_oracle as P
from oracle import path_b as O
from spectrum_bands import APIX, MARGIN, Probe, band_masks, band_of_frequency

SCORE_TOL = 2e-4             # the project's score bound for these paths
PHASE_WEIGHT = 0.5
MODES = {"zoom": None, "filter_lp_hp": (0.3, 0.05), "filter_hp": (0.0, 0.05), "phase": None}   # mode -> (lp, hp) of a filter

ZOOM_IMAGE = (96, 176)       # the zoomed cases' image: 136 / 96 = 1.42, 264 / 176 = 1.5 at the Nyquist cutoff


@dataclass(frozen=True)
class Case:
    shape: tuple            # the image's (ny, nx)
    size: tuple | None      # output_size, or None: the identity zoom (the image's shape and Nyquist)
    what: str
    cutoff: tuple | None = None   # cutoff_res of a zoomed case

    @property
    def plane(self) -> tuple:
        return self.size or self.shape


NYQUIST = (2 * APIX, 2 * APIX)   # finer sampling only

CASES = {
    "zoom_136x264": Case(ZOOM_IMAGE, (136, 264), "2 x 3 zoom tiles, the last 8 lines wide both ways; 3 x 5 filter tiles; even, even", NYQUIST),
    "zoom_129x130": Case(ZOOM_IMAGE, (129, 130), "2 x 2 zoom tiles, a one-line last row of tiles; 3 x 3 filter tiles; odd, even", NYQUIST),
    "zoom_130x129": Case(ZOOM_IMAGE, (130, 129), "2 x 2 zoom tiles, a one-line last column of tiles; 3 x 3 filter tiles; even, odd", NYQUIST),
    "identity_136x264": Case((136, 264), None, "filter and phase without a zoom; even, even"),
    "identity_129x131": Case((129, 131), None, "odd, odd: four operator terms on several tiles"),
}


@functools.lru_cache(maxsize=None)
def probe_of(shape) -> Probe:
    return Probe(*shape)


def score_of(mode: str):
    return O.cosine_similarity if mode == "phase" else O.cross_correlation_coefficient


def plane(img, case: Case, mode: str, apix: float) -> np.ndarray:
    """The float64 plane a mode scores: the normalised (filtered) amplitude spectrum, or the phase map M."""
    img = np.asarray(img, dtype=np.float64)
    if mode == "phase":
        return P.phase_map(img, apix, case.cutoff, case.size, True)[0]
    lp, hp = MODES[mode] or (0, 0)
    return O.compute_power_spectra(img, apix, case.cutoff, case.size, True, lp, hp)[0]


def band_scores(exp, cands, masks, score) -> np.ndarray:
    """[bands, candidates] float64."""
    return np.array([[float(score(exp[m], c[m])) for c in cands] for m in masks], dtype=np.float64)


def swap_sensitivity(exp, cand, axis: int, score) -> np.ndarray:
    """[bands]: the smallest change of a band's score over all swaps of two adjacent lines of ``cand`` (rows for axis 0,
    columns for axis 1) that both lie in the band."""
    e = exp if axis == 1 else exp.T
    p = cand if axis == 1 else cand.T
    band = band_of_frequency(p.shape[1])
    worst = np.full(int(band.max()) + 1, np.inf)
    for b in range(len(worst)):
        cols = np.flatnonzero(band == b)
        eb, pb = e[:, cols], p[:, cols].copy()
        base = float(score(eb, pb))
        for i in np.flatnonzero(np.diff(cols) == 1):
            pb[:, [i, i + 1]] = pb[:, [i + 1, i]]
            worst[b] = min(worst[b], abs(float(score(eb, pb)) - base))
            pb[:, [i, i + 1]] = pb[:, [i + 1, i]]
    return worst


class Oracle:
    """One (case, mode): the planes of both experimental images and of every candidate, then every band of both axes."""

    def __init__(self, name: str, mode: str):
        self.case, self.mode = CASES[name], mode
        self.probe = probe_of(self.case.shape)
        self.score = score_of(mode)
        pr = self.probe
        self.exp = [plane(pr.image, self.case, mode, pr.apix), plane(pr.image2, self.case, mode, pr.apix)]
        self.cands = [plane(s, self.case, mode, pr.apix) for s in pr.sims()]
        self.masks = [band_masks(*self.case.plane, axis) for axis in (0, 1)]
        # scores[image][axis]: [bands, candidates]
        self.scores = [[band_scores(e, self.cands, m, self.score) for m in self.masks] for e in self.exp]

    def under(self, mask, image: int = 0) -> np.ndarray:
        """[candidates] under any mask of the plane."""
        return np.array([float(self.score(self.exp[image][mask], c[mask])) for c in self.cands])

    def sensitivity(self, image: int, axis: int) -> np.ndarray:
        """[bands] of the candidate the image was made from (candidate 0, or probe.cand2 for the second image)."""
        return swap_sensitivity(self.exp[image], self.cands[self.probe.cand2 if image else 0], axis, self.score)


@functools.lru_cache(maxsize=None)
def oracle(name: str, mode: str) -> Oracle:
    return Oracle(name, mode)


__all__ = ["CASES", "MODES", "MARGIN", "SCORE_TOL", "PHASE_WEIGHT", "Case", "Oracle", "oracle", "probe_of", "plane",
           "band_scores", "swap_sensitivity", "score_of"]
