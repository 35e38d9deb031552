"""A probe that sees every column (or row) of the spectrum a general-size sweep scores: band masks that partition the
plane, a geometry whose amplitude spectrum has no empty column out to Nyquist, the float64 oracle's scores under every
band, the probe's own sensitivity to a misplaced column, and the per-band tolerance.  No GPU dependency: only the NumPy
oracle (and scipy.fft for the float32 floor).

Why: oracle.path_b.radial_band_mask keeps r < min(ny, nx)//2 - 1, so on a 24 x 960 image about 22 of the 960 columns enter
a score, and a clean one-subunit helix with ball_radius = 2 apix has no amplitude between its layer lines anyway — a row
transform that is wrong only at |kx| >~ ny/2 passes every comparison made under that mask.

Band masks.  |kx| in [0, nx//2] is cut into min(16, nx//2 + 1) contiguous bands over all ky (``axis=1``; ``axis=0`` cuts
|ky| the same way over all kx); every bin of the fftshifted plane lies in exactly one band.

Geometry (``Probe``).  Five irregular subunits from a seeded generator (radii 0.1 ... 0.5 of the diameter, any
angle, z within +-0.4 rise) on a helix of diameter 0.8 ny apix, ball_radius = 0.5 apix (a sub-pixel ball: its envelope is
still 0.4 at Nyquist), rise 200 A at apix = 2 (a quarter of the tube, at least 20 A, on short tubes) — few lattice points:
the spectrum is a speckle, not a set of layer lines; candidates 2 twists x 2 rises x Csym 1, 2.  The experimental image is
the first candidate's clean projection plus a little noise; a second one (``image2``) is made from the last candidate
(Csym 2, the other twist and rise).  Only the candidate an image was made from sees every column of it — a swap in another
candidate's spectrum moves a band by about the tolerance or less — so the row transform is seen through candidate 0 and
what depends on Csym / rise through the last candidate and the second image.

Tolerance of a band against the oracle: max(2e-5, 4 x floor), floor = what float32 costs the reference itself (the
candidate's raster rounded to float32 and transformed by scipy.fft in complex64, against the same pipeline in float64,
under that band).  It never looks at the device's output.
"""
from __future__ import annotations

import math

import numpy as np

from oracle import path_b as O

APIX = 2.0
NY = 24                      # the census's image height
MAX_BANDS = 16
ORACLE_TOL = 2e-5            # the project's level for these kernels against the oracle
PATHS_TOL = 5e-6             # between two device paths (two-step / Stockham / float64 direct)
FLOOR_FACTOR = 4.0           # device summation order and twiddle precision against pocketfft's: a small constant
MARGIN = 10.0                # a misplaced column must move its band's score by at least MARGIN x the band's tolerance
UNIT_SEED = 7
REDUCED_SEED = 1             # of the probes with fewer than five subunits: with seed 7 a two- or three-subunit Csym 2 helix leaves
                             # adjacent columns too alike at seven (length, spectrum) cases (3 ... 9 x tolerance); 1 gives >= 13 x
TWISTS = (31.0, 47.5)
RISE = 200.0                 # of the first candidate on a long tube; a short tube takes a quarter of its length (at least 20 A)
NOISE = 0.1                  # the experimental image: the first candidate's projection + this fraction of its std as white noise
CSYMS = (1, 2)


# ---- band masks ------------------------------------------------------------------------------------------------------
def n_bands(n: int) -> int:
    return min(MAX_BANDS, n // 2 + 1)


def band_of_frequency(n: int) -> np.ndarray:
    """Band index of every position of an fftshifted axis of length n (|k| = |index - n//2| in [0, n//2])."""
    k = np.abs(np.arange(n) - n // 2)
    return (k * n_bands(n)) // (n // 2 + 1)


def band_masks(ny: int, nx: int, axis: int = 1) -> np.ndarray:
    """[bands, ny, nx] bool on the fftshifted plane: bands in |kx| over all ky (axis=1) or in |ky| over all kx (axis=0)."""
    n = nx if axis == 1 else ny
    b = band_of_frequency(n)
    sel = b[None, :] == np.arange(n_bands(n))[:, None]                     # [bands, n]
    shape = (ny, nx)
    return np.stack([np.broadcast_to(s[None, :] if axis == 1 else s[:, None], shape).copy() for s in sel])


# ---- geometry --------------------------------------------------------------------------------------------------------
class Probe:
    """Geometry, candidate list and experimental image of one (ny, nx)."""

    def __init__(self, ny: int, nx: int, n_units: int = 5, seed: int | None = None):
        self.ny, self.nx, self.apix = int(ny), int(nx), APIX
        self.diameter = 0.8 * ny * APIX
        self.ball_radius = 0.5 * APIX
        rise = min(RISE, max(20.0, nx * APIX / 4))
        self.rises = (rise, 1.06 * rise)
        rng = np.random.default_rng((UNIT_SEED if n_units >= 5 else REDUCED_SEED) if seed is None else seed)
        r = rng.uniform(0.1, 0.5, 8) * self.diameter
        a = rng.uniform(-np.pi, np.pi, 8)
        z = rng.uniform(-0.4, 0.4, 8) * rise
        self.units = np.stack([r, a, z], axis=1)[:n_units]                 # (radius, angle, z): SweepEngine.set_geometry(units=)
        u = self.units
        self.units_xyz = np.stack([u[:, 0] * np.cos(u[:, 1]), u[:, 0] * np.sin(u[:, 1]), u[:, 2]], axis=1).astype(np.float32)
        # csym-major, then twist, then rise: runs of candidates that share (twist, csym)
        self.params = np.array([(tw, rs, float(cs), 0.0) for cs in CSYMS for tw in TWISTS for rs in self.rises], dtype=np.float64)
        clean = self.simulate(*self.params[0, :3])
        noise = np.random.default_rng(1000 + nx * 1031 + ny).normal(0, NOISE * clean.std(), clean.shape)
        self.image = (clean + noise).astype(np.float32)
        # a second experimental image, made from the last candidate (second twist, second rise, Csym 2): what depends on
        # Csym or rise (table slices, column factors) is then seen on every column too, not only the row transform
        self.cand2 = len(self.params) - 1
        clean2 = self.simulate(*self.params[self.cand2, :3])
        noise2 = np.random.default_rng(2000 + nx * 1031 + ny).normal(0, NOISE * clean2.std(), clean2.shape)
        self.image2 = (clean2 + noise2).astype(np.float32)
        self._sims = None

    def sims(self) -> list:
        """Every candidate's float64 projection (computed once: both spectrum kinds and both axes share them)."""
        if self._sims is None:
            self._sims = [self.simulate(*p[:3]) for p in self.params]
        return self._sims

    def geometry(self) -> dict:
        return dict(apix=self.apix, helical_diameter=self.diameter, ball_radius=self.ball_radius, units=self.units)

    def simulate(self, twist, rise, csym) -> np.ndarray:
        return O.simulate_helical_projection(len(self.units_xyz), twist, rise, int(csym), self.diameter, self.ball_radius, 0, 0,
                                             self.ny, self.nx, self.apix, units=self.units_xyz)

    def stockham_lds(self) -> int:
        """Dynamic LDS bytes the Stockham kernel needs for this list (the launch's own sizing, restated): 16 row buffers,
        8 table slices, the twiddles, the column factors and their column-group starts.  Above 160 KB the list takes the
        float64 direct path."""
        rows_lds, kg = self.rows_lds_kg()
        nxp = (self.nx + 3) // 4 * 4
        return 16 * nxp * 8 + 8 * rows_lds * 8 + ((self.nx + 1) & ~1) * 8 + kg * nxp * 4 + (nxp // 4 + 4) * 4

    # Table rows a run keeps in LDS and table rows one column group reaches, as the library sizes them for this list.
    # These two methods mirror host arithmetic of the library and change with it: rpx and slack from hh_set_geometry
    # (helicon_hip.hip, "truncation half-window" / d.slack), rows, span4, kg and the LDS sum from gen_sweep
    # (general_host.inc, "---- sizes").  The GPU census holds them to it: it asserts last_row_kernel == (0, 0, stockham_lds()).
    def rows_lds_kg(self) -> tuple[int, int]:
        rise = min(self.rises)
        imax = math.ceil(self.nx * self.apix / rise)
        rows = (2 * imax + 1) * len(self.units)
        sigma2 = self.ball_radius ** 2 / math.log(2.0)
        rpx = max(1, math.ceil(math.sqrt(sigma2 * 24 * math.log(2.0)) / self.apix))
        slack = float(np.abs(self.units[:, 2]).max()) + 1e-3
        kg = (math.floor(((3 + 2 * rpx) * self.apix + 2 * slack) / rise) + 2) * len(self.units)
        return max(rows, kg), kg


# ---- oracle side -----------------------------------------------------------------------------------------------------
def amplitude(image, log: bool, dtype=np.float64) -> np.ndarray:
    """fftshifted log1p|F| or |F| of a real image (the quantity compute_power_spectra normalises affinely, which a
    correlation coefficient does not see).  float64: NumPy's transform, as the oracle; float32: the image rounded to
    float32 and scipy.fft in complex64 — the reference's own float32 floor."""
    if dtype == np.float64:
        f = np.fft.fft2(np.asarray(image, dtype=np.float64))
    else:
        import scipy.fft
        f = scipy.fft.fft2(np.asarray(image, dtype=np.float32).astype(np.complex64))
        assert f.dtype == np.complex64
    a = np.abs(np.fft.fftshift(f))
    return np.log1p(a) if log else a


def band_scores(pwr_exp, pwrs, masks) -> np.ndarray:
    """[bands, candidates] float64: O.cross_correlation_coefficient under every mask."""
    out = np.empty((len(masks), len(pwrs)))
    for b, m in enumerate(masks):
        e = pwr_exp[m]
        for g, p in enumerate(pwrs):
            out[b, g] = O.cross_correlation_coefficient(e, p[m])
    return out


class OracleSide:
    """Experimental spectrum once, every candidate's spectrum once, then every band."""

    def __init__(self, probe: Probe, log: bool = True, axis: int = 1, with_floor: bool = True, image=None):
        self.probe, self.log, self.axis = probe, log, axis
        self.masks = band_masks(probe.ny, probe.nx, axis)
        self.pwr_exp = amplitude(probe.image if image is None else image, log)     # (image: another experimental image)
        sims = probe.sims()
        self.pwrs = [amplitude(s, log) for s in sims]
        self.scores = band_scores(self.pwr_exp, self.pwrs, self.masks)          # [bands, candidates]
        if with_floor:
            low = band_scores(self.pwr_exp, [amplitude(s, log, np.float32) for s in sims], self.masks)
            self.floor = np.abs(low - self.scores).max(axis=1)                  # [bands]
            self.tol = np.maximum(ORACLE_TOL, FLOOR_FACTOR * self.floor)        # [bands]

    # -- how far a misplaced column moves its band's score (reference only) ---------------------------------------------
    def swap_sensitivity(self, cand: int = 0) -> np.ndarray:
        """[bands]: over all swaps of two adjacent columns (rows for axis=0) of the candidate's fftshifted spectrum, the
        smallest change of the score under the band(s) the two columns lie in (a swap across a band border counts for
        both bands with the larger of its two changes: either comparison would catch it)."""
        p = self.pwrs[cand] if self.axis == 1 else self.pwrs[cand].T
        e = self.pwr_exp if self.axis == 1 else self.pwr_exp.T
        n = p.shape[1]
        band = band_of_frequency(n)
        worst = np.full(len(self.masks), np.inf)
        stats = [_BandStats(e[:, band == b], p[:, band == b]) for b in range(len(self.masks))]
        pos = np.cumsum(band[None, :] == np.arange(len(self.masks))[:, None], axis=1) - 1    # column -> index inside its band
        for j in range(n - 1):
            bj, bk = band[j], band[j + 1]
            if bj == bk:
                d = stats[bj].swapped(pos[bj, j], pos[bj, j + 1])
                worst[bj] = min(worst[bj], d)
            else:
                d = max(stats[bj].replaced(pos[bj, j], p[:, j + 1]), stats[bk].replaced(pos[bk, j + 1], p[:, j]))
                worst[bj] = min(worst[bj], d)
                worst[bk] = min(worst[bk], d)
        return worst

    def mirror_sensitivity(self, cand: int = 0) -> np.ndarray:
        """[bands]: change of the band's score when the candidate's columns are mirrored kx <-> -kx inside the band."""
        p = self.pwrs[cand] if self.axis == 1 else self.pwrs[cand].T
        e = self.pwr_exp if self.axis == 1 else self.pwr_exp.T
        n = p.shape[1]
        band = band_of_frequency(n)
        k = np.arange(n) - n // 2
        src = (-k) % n                                   # unshifted index of -k ...
        src = (src + n // 2) % n                         # ... and its place on the shifted axis (the Nyquist column is its own mirror)
        out = np.empty(len(self.masks))
        for b in range(len(self.masks)):
            sel = band == b
            out[b] = abs(O.cross_correlation_coefficient(e[:, sel], p[:, src][:, sel]) - O.cross_correlation_coefficient(e[:, sel], p[:, sel]))
        return out


def device_scores(eng, probe: Probe, masks, log: bool, images=None):
    """([bands, segments, candidates] float32, row kernel): the probe's list swept under every mask by an engine (anything
    with SweepEngine's set_reference / sweep / last_row_kernel; its geometry already set to probe.geometry()), every sweep
    repeated bit for bit; the mask must not decide the kernel."""
    images = probe.image if images is None else images
    out, kernels = [], set()
    for b, mask in enumerate(masks):
        eng.set_reference(images, mask, log=log)
        got = eng.sweep(probe.params)
        kernels.add(eng.last_row_kernel)
        assert np.array_equal(got, eng.sweep(probe.params)), (probe.ny, probe.nx, b, "not bit-reproducible")
        out.append(got)
    assert len(kernels) == 1, (probe.ny, probe.nx, kernels)
    return np.stack(out), kernels.pop()


class _BandStats:
    """The correlation coefficient of one band, recomputed after a change of one or two columns of the candidate."""

    def __init__(self, e, p):
        self.e, self.p = np.ascontiguousarray(e, dtype=np.float64), np.array(p, dtype=np.float64)
        self.base = float(O.cross_correlation_coefficient(self.e, self.p))

    def _with(self, cols, values) -> float:
        keep = self.p[:, cols].copy()
        self.p[:, cols] = values
        d = abs(float(O.cross_correlation_coefficient(self.e, self.p)) - self.base)
        self.p[:, cols] = keep
        return d

    def swapped(self, a, b) -> float:
        return self._with([a, b], self.p[:, [b, a]])

    def replaced(self, a, column) -> float:
        return self._with([a], column[:, None])


# ---- the census of row lengths ----------------------------------------------------------------------------------------
def is_31_smooth(n: int) -> bool:
    """No prime factor above 31: the lengths the row-transform kernels (radices 2 ... 31) can serve."""
    for p in (2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31):
        while n % p == 0:
            n //= p
    return n == 1


def census(lo: int = 8, hi: int = 1024):
    """(two_step {nx: (r1, r2)}, stockham [nx], direct [nx]) from the library's own plan (hh_general_plan, host arithmetic,
    at the shape the existing plan test uses) and the 31-smooth rule."""
    import ctypes as C

    from helicon_amd import _lib

    L = _lib.lib()
    two, stock, direct = {}, [], []
    for nx in range(lo, hi + 1):
        out = (C.c_int64 * 6)()
        assert L.hh_general_plan(nx, 2 * (nx // 8) + 1, 7, out) == 0
        if out[0]:
            two[nx] = (int(out[0]), int(out[1]))
        elif is_31_smooth(nx):
            stock.append(nx)
        else:
            direct.append(nx)
    return two, stock, direct


LDS_LIMIT = 160 * 1024


def probe_for_length(nx: int, ny: int = NY) -> Probe:
    """The census's probe of a row length: five subunits, or the most (four ... two) with which the length's own kernel
    serves the list — its factor pair stays on the two-step kernel (hh_general_plan at the probe's rows_lds, kg), a
    Stockham-only length fits the 160 KB of LDS.  A length with a prime factor above 31 keeps five."""
    import ctypes as C

    from helicon_amd import _lib

    L = _lib.lib()
    out = (C.c_int64 * 6)()
    assert L.hh_general_plan(nx, 2 * (nx // 8) + 1, 7, out) == 0
    has_pair = bool(out[0])
    for n_units in (5, 4, 3, 2):
        probe = Probe(ny, nx, n_units)
        if has_pair:
            rows_lds, kg = probe.rows_lds_kg()
            assert L.hh_general_plan(nx, rows_lds, kg, out) == 0
            if out[0]:
                return probe
        elif not is_31_smooth(nx) or probe.stockham_lds() <= LDS_LIMIT:
            return probe
    raise AssertionError(f"nx = {nx}: no probe keeps the length on its kernel")


DIRECT_SAMPLE = (37, 74, 127, 997, 1021, 11 * 37, 2 * 41, 43, 3 * 47, 53 * 8, 59, 61 * 5, 67 * 9, 71 * 14, 73 * 4, 79 * 12,
                 83, 89 * 11, 97 * 10, 101, 103 * 6, 509, 2 * 509, 1019)
