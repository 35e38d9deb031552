"""The band probe of tests/spectrum_bands.py on the square power-of-two planes of the tuned sweep: `Probe(N, N)` for every
compiled size with a candidate list the run pipelines accept, the four paths of tests/sweep_variants.py, the candidates held
against the float64 oracle, the signed quadrant masks that expose the Hermitian fold, and the tolerances.  No GPU is needed
to import this module: tests/test_square_bands_host.py checks the probe with the reference alone,
tests/test_gpu_square_bands.py runs it.

Why: every other test of `k_fused_pass<N, EPI, LOG, WALK>`, `launch_second<N, EPI, LOG>` and the per-candidate transform
pipeline scores under `radial_band_mask` on a clean one-subunit helix (ball radius 2 apix).  That plane is empty between
its layer lines and beyond |k| ~ N/4: a third to a half of all swaps of two adjacent spectrum lines, and every one at high
|k|, move such a score by less than the 2e-5 those tests hold.  Under the 16 |kx| and 16 |ky| band masks every bin of the
plane is in exactly one band per axis, and the probe's speckle has no empty line out to Nyquist.

List (``SquareProbe.params``): Csym-major, then twist, then rise — Csym (1, 2) x twists (31, 47.5) x 8 rises
linspace(r0, 1.06 r0, 8), r0 the probe's first rise: 4 runs of 8 candidates with one rise column, which the run-table and
fused pipelines take (runs of at least 8, one set of column factors per rise).  Candidate 0 and the last candidate are the
probe's own: ``image`` is made from the first, ``image2`` from the last.

Subunits (``N_UNITS``): the fused pass needs kg = (floor(((3 + 2 rpx) apix + 2 slack) / r0) + 2) x subunits <= 16 factor
rows per group of four columns (rpx = 3 at ball radius 0.5 apix, slack = max |z| + 1e-3 = 0.396 r0 + 1e-3 with the seeded
subunits, so the span is 18 A + 0.79 r0).  Up to N = 128 (r0 = 20, 32, 64) the floor is 1 and five subunits give kg 15; from
N = 256 (r0 = 128, 200, 200) it is 0 and kg is 10: every size keeps five subunits.  The tables are short (36 staged rows, 68
at 1024), so the LDS is no limit below 1024; there the rise walk takes 158,240 B of the 162,816 B a workgroup may have.
``footprint(n)`` restates the library's arithmetic (kg, staged rows, LDS bytes of both walks through its host entry
points); the GPU census holds the device's own report to it.

Fold masks (``quadrant_masks``): a band cut to one open quadrant of the lower half plane (ky < 0 with kx > 0, or ky < 0 with
kx < 0).  The kernels score on the Hermitian half plane 0 <= ky <= N/2 with weights W = mask(k) + mask(-k); under such a mask
the half plane receives its whole weight through mask(-k), so a wrong partner index (one line off along either axis) scores
other bins altogether.

Tolerance: per mask max(2e-5, 4 x floor), the floor as `spectrum_bands.OracleSide` computes it (float32 raster, scipy.fft in
complex64, against float64), never above SCORE_TOL = 2e-4 and never from a device's output.
"""
from __future__ import annotations

import ctypes as C
import functools
import math

import numpy as np

import spectrum_bands as SB
from oracle import path_b as O
from tests import sweep_variants as SV

SIZES = SV.SIZES
PATHS = SV.PATHS
N_RISES = 8
RISE_SPAN = 1.06
ORACLE_TOL = SB.ORACLE_TOL       # 2e-5: DESIGN.md section 2, the three pipelines against the oracle and each other
PATHS_TOL = 2e-5
SEGMENT_TOL = 2e-6               # a row of a several-segment sweep against its single-segment sweep (config C5)
SCORE_TOL = SV.SCORE_TOL         # 2e-4: no band's tolerance goes above it
MARGIN = SB.MARGIN
MIN_OWN_SCORE = 0.9
MIN_FOLD_BINS = 8

# Subunits of the probe per size: the most (five ... two) that leave the list on the fused pass (kg <= 16 and the LDS of
# both walks within a compute unit's); tests/test_square_bands_host.py recomputes the choice.
N_UNITS = {32: 5, 64: 5, 128: 5, 256: 5, 512: 5, 1024: 5}

# Forms that cannot be reached at a size: (N, path) -> reason.  The twist walk is not compiled at 1024 (SPLIT rows): a forced
# "twists" runs the rise walk there, which the census asserts and sweeps; that is a report, not a missing form.
UNREACHABLE: dict = {}

CASES = [(n, log, axis) for n in SIZES for log in (True, False) for axis in (1, 0)]


def case_id(case) -> str:
    n, log, axis = case
    return f"n{n}-{'log' if log else 'abs'}-{'kx' if axis == 1 else 'ky'}"


def expected(n: int, path: str) -> tuple:
    """(last_first_pass, last_fused_walk, last_factor_sets) after a sweep of the list on `path`."""
    if path in ("transform", "run_tables"):
        return path, "none", 0
    return "fused", ("twists" if path == "fused/twists" and SV.twist_walk_built(n) else "rises"), N_RISES


class SquareProbe(SB.Probe):
    """`Probe(N, N)` with the 4 x 8 list; every float64 projection is computed once and kept."""

    def __init__(self, n: int, n_units: int | None = None):
        self._memo = {}
        super().__init__(n, n, N_UNITS[n] if n_units is None else n_units)
        base = self.params
        self.rise_column = np.linspace(self.rises[0], RISE_SPAN * self.rises[0], N_RISES)
        self.params = np.array([(tw, rs, float(cs), 0.0) for cs in SB.CSYMS for tw in SB.TWISTS for rs in self.rise_column],
                               dtype=np.float64)
        self.cand2 = len(self.params) - 1
        # the images were made from the base list's first and last candidates: they are this list's first and last too
        assert np.array_equal(self.params[0], base[0]) and np.array_equal(self.params[-1], base[-1])

    def simulate(self, twist, rise, csym) -> np.ndarray:
        key = (float(twist), float(rise), int(csym))
        if key not in self._memo:
            self._memo[key] = super().simulate(twist, rise, csym)
        return self._memo[key]

    def sim(self, cand: int) -> np.ndarray:
        return self.simulate(*self.params[cand, :3])

    def view(self, picks) -> "View":
        return View(self, picks)


class View:
    """What `spectrum_bands.OracleSide` reads of a probe, restricted to some candidates (in the order given)."""

    def __init__(self, probe: SquareProbe, picks):
        self.probe, self.picks = probe, list(picks)
        self.ny, self.nx, self.image, self.image2 = probe.ny, probe.nx, probe.image, probe.image2

    def sims(self) -> list:
        return [self.probe.sim(g) for g in self.picks]


@functools.lru_cache(maxsize=None)
def probe_of(n: int) -> SquareProbe:
    return SquareProbe(n)


def picks(n: int) -> list:
    """Candidates held against the oracle: all 32 up to 256; at 512 the first, the last and both sides of each of the three
    run boundaries; at 1024 the first, the last and one from inside each of the two middle runs."""
    total = 4 * N_RISES
    if n <= 256:
        return list(range(total))
    if n == 512:
        return sorted({0, total - 1} | {r * N_RISES + d for r in (1, 2, 3) for d in (-1, 0)})
    return [0, N_RISES + 3, 2 * N_RISES + 5, total - 1]


def fold_picks(n: int) -> list:
    """Both images' own candidates and two others (a Csym 1 and a Csym 2 one, off the ends of their runs)."""
    total = 4 * N_RISES
    return [0, N_RISES + 3, 2 * N_RISES + 5, total - 1]


@functools.lru_cache(maxsize=None)
def oracle_side(n: int, log: bool, axis: int, image: int, which: str = "picks") -> SB.OracleSide:
    """`OracleSide` of one image (0: ``image``, 1: ``image2``) over picks(n) ("picks") or over the image's own candidate
    alone ("own": what the host checks need)."""
    probe = probe_of(n)
    sel = picks(n) if which == "picks" else [probe.cand2 if image else 0]
    return SB.OracleSide(probe.view(sel), log, axis, image=probe.image2 if image else probe.image)


# ---- the Hermitian fold -----------------------------------------------------------------------------------------------------
def quadrant_masks(n: int) -> tuple[np.ndarray, list]:
    """([masks, n, n] bool, [(axis, band, kx sign)]): every |kx| band and every |ky| band cut to ky < 0, kx > 0 and to
    ky < 0, kx < 0 on the fftshifted plane (row = ky + n/2, column = kx + n/2); masks with fewer than MIN_FOLD_BINS bins are left
    out (the kx = 0 band of a narrow plane)."""
    k = np.arange(n) - n // 2
    lower = (k < 0)[:, None]
    out, names = [], []
    for axis in (1, 0):
        bands = SB.band_masks(n, n, axis)
        for sign in (+1, -1):
            side = (k * sign > 0)[None, :]
            for b, m in enumerate(bands):
                q = m & lower & side
                if q.sum() >= MIN_FOLD_BINS:
                    out.append(q)
                    names.append((axis, b, sign))
    return np.stack(out), names


def scores_at(pwr_exp, pwrs, bins) -> np.ndarray:
    """`spectrum_bands.band_scores` with every mask given as the flat indices of its bins (a quadrant mask holds a
    hundredth of a plane of a million bins): [masks, candidates] float64."""
    e, ps = pwr_exp.ravel(), [p.ravel() for p in pwrs]
    return np.array([[float(O.cross_correlation_coefficient(e[at], p[at])) for p in ps] for at in bins], dtype=np.float64)


class FoldSide:
    """Oracle scores, float32 floor and one-line-shift sensitivity under the quadrant masks, for fold_picks(n)."""

    def __init__(self, n: int, log: bool = True):
        probe = probe_of(n)
        self.masks, self.names = quadrant_masks(n)
        self.picks = fold_picks(n)
        sims = [probe.sim(g) for g in self.picks]
        self.pwrs = [SB.amplitude(s, log) for s in sims]
        low = [SB.amplitude(s, log, np.float32) for s in sims]
        self.exp = [SB.amplitude(img, log) for img in (probe.image, probe.image2)]
        self.bins = [np.flatnonzero(m) for m in self.masks]
        self.scores = np.stack([scores_at(e, self.pwrs, self.bins) for e in self.exp])              # [images, masks, picks]
        floor = np.stack([np.abs(scores_at(e, low, self.bins) - s) for e, s in zip(self.exp, self.scores)])
        self.floor = floor.max(axis=(0, 2))                                                         # [masks]
        self.tol = np.maximum(ORACLE_TOL, SB.FLOOR_FACTOR * self.floor)

    def shift_sensitivity(self, image: int) -> np.ndarray:
        """[masks]: the smallest change of the own candidate's score when its bins are taken one line off (either way,
        along either axis)."""
        own = len(self.picks) - 1 if image else 0
        e, p = self.exp[image], self.pwrs[own]
        out = np.full(len(self.masks), np.inf)
        for axis in (0, 1):
            for step in (1, -1):
                moved = np.roll(p, step, axis=axis)
                for i, at in enumerate(self.bins):
                    d = abs(float(O.cross_correlation_coefficient(e.ravel()[at], moved.ravel()[at])) - self.scores[image, i, own])
                    out[i] = min(out[i], d)
        return out


@functools.lru_cache(maxsize=None)
def fold_side(n: int) -> FoldSide:
    return FoldSide(n)


# ---- the fused pass's shape, restated from the library's host arithmetic -------------------------------------------------------
def footprint(n: int, n_units: int | None = None) -> dict | None:
    """{"kg", "rows", "lds_rises", "lds_twists"} of the list at size n as `fused_shape` (helicon_hip.hip) computes them, or
    None where the fused pass does not fit (kg above 16 or more LDS than 160 KB - 1 KB)."""
    from helicon_amd import _lib

    L = _lib.lib()
    probe = probe_of(n) if n_units is None else SquareProbe(n, n_units)
    r0 = float(probe.rise_column.min())
    sigma2 = probe.ball_radius ** 2 / math.log(2.0)
    rpx = max(1, math.ceil(math.sqrt(sigma2 * 24 * math.log(2.0)) / probe.apix))
    slack = float(np.float32(np.abs(probe.units[:, 2]).max() + 1e-3))
    kg = (math.floor(((3 + 2 * rpx) * probe.apix + 2 * slack) / float(np.float32(r0))) + 2) * len(probe.units)
    ext = int(L.hh_table_extent(n, C.c_double(probe.apix), rpx, C.c_double(slack), C.c_double(r0)))
    rows = max((2 * ext + 1) * len(probe.units), kg)
    rows += (4 - rows % 8 + 8) % 8
    lds_r = int(L.hh_fused_lds_bytes(n, rows, kg, 1))
    lds_t = int(L.hh_fused_lds_bytes(n, rows, kg, 2))
    if kg > 16 or lds_r > 160 * 1024 - 1024:
        return None
    return dict(kg=kg, rows=rows, lds_rises=lds_r, lds_twists=lds_t)


def host_table(sizes=SIZES, logs=(True, False)) -> list:
    """Rows of DESIGN.md's "Square-plane census" host table: per size the worst of the given spectra —
    (N, subunits, kg, swap kx cand 0, swap kx last, swap ky cand 0, swap ky last, mirror, floor, smallest own score)."""
    rows = []
    for n in sizes:
        swap = {(axis, image): np.inf for axis in (1, 0) for image in (0, 1)}
        mirror, floor, own = np.inf, 0.0, np.inf
        for log in logs:
            for axis in (1, 0):
                for image in (0, 1):
                    o = oracle_side(n, log, axis, image, "own")
                    swap[axis, image] = min(swap[axis, image], float(o.swap_sensitivity(0).min()))
                    floor = max(floor, float(o.floor.max()))
                    own = min(own, float(o.scores[:, 0].min()))
                    if image == 0:
                        mirror = min(mirror, float(o.mirror_sensitivity(0)[paired_bands(n)].min()))
        f = footprint(n)
        rows.append((n, len(probe_of(n).units), f["kg"] if f else None, swap[1, 0], swap[1, 1], swap[0, 0], swap[0, 1], mirror, floor, own))
    return rows


def paired_bands(n: int) -> list:
    """Bands that hold more than the self-mirrored lines (k = 0 and the Nyquist line)."""
    band = SB.band_of_frequency(n)
    k = np.abs(np.arange(n) - n // 2)
    return [b for b in range(SB.n_bands(n)) if np.any((band == b) & (k > 0) & (2 * k != n))]
