"""The variant matrix of the tuned sweep's scoring kernels: one case per (N, segments, spectrum), the four paths each case
is swept on, the candidates held against the float64 oracle, the edge masks of the compact q, and the tolerances.  No
GPU is needed to import this module: `tests/test_sweep_variants_host.py` checks the table itself,
`tests/test_gpu_sweep_variants.py` runs it.

`k_fused_pass<N, EPI, LOG, WALK>` is compiled for N in SIZES, EPI_SCORE (one segment) / EPI_QSTORE (several), LOG 0 / 1
and the rise / twist walk (the latter for N <= 512): 44 kernels; `launch_second<N, EPI, LOG>` (run tables) and the
per-candidate transform pipeline are dispatched over the same sizes.  A case's grid is 3 twists x 8 rises, Csym 1,
twist-major as `build_grid` makes it: every run carries the same rise column (one set of column factors per rise), and the
odd run count ends the N = 512 twist walk on a pair whose second run is the table's zeroed one.

Geometry: apix 1, helical diameter 0.4 N, ball radius 2 (rpx = 10, slack 1e-3: four columns span 23.002 A, so
kg = floor(23.002 / rise) + 2 <= 16 needs rise > 1.534).  Twists and rises at 512, 256, 64 and 1024 are those of
tests/test_gpu_twist_walk.py; 128 and 32 had no fused case before, and the GPU test asserts the library's own footprint
report for every size (kg <= 16, as many resident workgroups of the twist walk as of the rise walk, and at least one).
N = 32 takes rises from 6.0 (kg 5).  N = 128 takes them from 2.0 (kg 13, 84 staged table rows): with the small tables of
rises near 5 the LDS is no limit (9 and 10 workgroups per compute unit), and the registers of
`k_fused_pass<128, EPI_QSTORE, *, WALK_TWISTS>` hold 6 where the other N = 128 forms hold 8 — `choose_walk` then gives a
forced twist walk with several segments to the rise walk (6 < 8).  From 2.0 the LDS decides: 27,424 B per rise-walking
workgroup (5 in 160 KB), 26,000 B per twist-walking one (6), so both walks run with one and with several segments.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from helicon_amd.grid import build_grid
from oracle import path_b as O

SIZES = (32, 64, 128, 256, 512, 1024)
TWIST_WALK_SIZES = (32, 64, 128, 256, 512)      # twist_walk_built(N); N = 1024 keeps the rise walk (SPLIT rows)
APIX, BALL_RADIUS = 1.0, 2.0
N_TWISTS, N_RISES = 3, 8

# N: (first twist, twist step, first rise); the rise step is 0.05 everywhere
AXES = {
    32: (20.0, 1.0, 6.0),
    64: (20.0, 1.0, 6.0),
    128: (20.0, 1.0, 2.0),
    256: (20.0, 1.0, 4.0),
    512: (2.0, 0.25, 4.0),
    1024: (2.0, 0.25, 9.0),
}

# path: (set_table_path mode, set_fused_walk mode)
PATHS = {
    "transform": (0, "auto"),
    "run_tables": (1, "auto"),
    "fused/rises": (2, "rises"),
    "fused/twists": (2, "twists"),
}

PIPE_TOL = 2e-5      # log spectra against the oracle: tests/test_gpu_twist_walk.py, tests/test_gpu_shared_factors.py
SCORE_TOL = 2e-4     # linear sweeps against goldens (tests/test_gpu_parity.py): LINEAR_TOL never exceeds it

# Linear spectra: the largest |score - oracle| of the `transform` path (per-candidate raster and two transforms, held to
# goldens by tests/test_gpu_parity.py) over the picks of both linear cases of a size, measured on one MI355X and printed
# by test_matrix; DESIGN.md, "Sweep variants", has the run.  The fused and run-table paths are held to
# max(PIPE_TOL, 4 x this) — the factor covers their different summation order — and never to more than SCORE_TOL.
TRANSFORM_LINEAR_ERR = {32: 1.380e-06, 64: 6.103e-07, 128: 3.351e-07, 256: 1.320e-07, 512: 3.432e-08, 1024: 3.233e-08}
LINEAR_TOL = {n: min(SCORE_TOL, max(PIPE_TOL, 4.0 * e)) for n, e in TRANSFORM_LINEAR_ERR.items()}

# Forms that cannot be reached at a size: (N, path) -> reason ("footprint": fused_walk_footprint reports no resident
# workgroup for the walk).  None: with the rises above every form of the table runs on an MI355X, and test_matrix sweeps them all.
UNREACHABLE: dict = {}


def twist_walk_built(n: int) -> bool:
    return n in TWIST_WALK_SIZES


def segments_of(n: int, several: bool) -> int:
    """Three segments below 512, two at 512 and 1024 (the oracle's CPU time)."""
    return 1 if not several else (3 if n < 512 else 2)


@dataclass(frozen=True)
class Case:
    n: int
    segments: int
    log: bool

    @property
    def id(self) -> str:
        return f"n{self.n}-{self.segments}seg-{'log' if self.log else 'linear'}"

    @property
    def twists(self) -> np.ndarray:
        t0, dt, _ = AXES[self.n]
        return t0 + dt * np.arange(N_TWISTS)

    @property
    def rises(self) -> np.ndarray:
        return AXES[self.n][2] + 0.05 * np.arange(N_RISES)

    @property
    def grid(self) -> np.ndarray:
        """[24, 4] float64, twist-major."""
        return build_grid(self.twists, self.rises, (1,), tube_length=float(self.n) * APIX).params

    @property
    def truth(self) -> tuple:
        """The grid's middle candidate (index 12): the experimental images are made from it."""
        return float(self.twists[N_TWISTS // 2]), float(self.rises[N_RISES // 2]), 1

    @property
    def geometry(self) -> dict:
        return dict(apix=APIX, helical_diameter=0.4 * self.n * APIX, ball_radius=BALL_RADIUS)

    @property
    def picks(self) -> list:
        return picks(self.n)

    @property
    def tol(self) -> float:
        return PIPE_TOL if self.log else LINEAR_TOL[self.n]

    def expected(self, path: str) -> tuple:
        """(last_first_pass, last_fused_walk, last_factor_sets) after a sweep of the grid on `path`."""
        if path == "transform":
            return "transform", "none", 0
        if path == "run_tables":
            return "run_tables", "none", 0
        walk = "twists" if path == "fused/twists" and twist_walk_built(self.n) else "rises"
        return "fused", walk, N_RISES


CASES = [Case(n, segments_of(n, several), log) for n in SIZES for several in (False, True) for log in (True, False)]


def picks(n: int) -> list:
    """Candidates held against the oracle (0.6 s each at 512, four times that at 1024): all 24 up to 128; at 256 and 512
    the first and the last of the list, the second run's second rise (the second half of the first pair at 512) and the
    last run's first rise (the lone first half of the last pair), at 256 also the truth and both sides of the first run
    boundary; at 1024 the first and the last."""
    total = N_TWISTS * N_RISES
    if n <= 128:
        return list(range(total))
    if n == 1024:
        return [0, total - 1]
    four = [0, total - 1, N_RISES + 1, (N_TWISTS - 1) * N_RISES]
    return sorted(four + ([N_RISES - 1, N_RISES, total // 2] if n == 256 else []))


MIN_PICKS = {32: 24, 64: 24, 128: 24, 256: 4, 512: 4, 1024: 2}


def noisy(clean: np.ndarray, seed: int) -> np.ndarray:
    return (clean + np.random.default_rng(seed).normal(0, 0.5 * clean.std(), clean.shape)).astype(np.float32)


def images(case: Case, simulate, segments: int | None = None) -> np.ndarray:
    """[S, n, n] float32: `simulate(twist, rise, csym)` of the truth plus noise, one seed per segment."""
    clean = np.asarray(simulate(*case.truth))
    return np.stack([noisy(clean, seed) for seed in range(case.segments if segments is None else segments)])


def oracle_simulate(case: Case):
    """`simulate` for `images` without a device."""
    g = case.geometry
    return lambda tw, rs, cs: O.simulate_helical_projection(1, tw, rs, cs, g["helical_diameter"], g["ball_radius"], 0, 0,
                                                            case.n, case.n, g["apix"])


def oracle_scores(case: Case, imgs: np.ndarray, pick: list, mask: np.ndarray | None = None) -> np.ndarray:
    """[S, len(pick)] float64: `oracle.path_b.sweep_cpu` per segment."""
    m = O.radial_band_mask(case.n, case.n) if mask is None else mask
    grid = case.grid
    return np.stack([O.sweep_cpu(img, grid[pick, :3], m, log=case.log, **case.geometry) for img in imgs])


# ---- the compact q's edge masks (several segments, N <= 512) --------------------------------------------------------------
# The mask lives on the fftshifted plane; its first axis is ky (tests/spectrum_bands.py: axis 0), |ky| = |row - N/2|.  The
# library folds it into Hermitian half-plane weights W[ky][kx], 0 <= ky <= N/2, and a workgroup of the scoring kernels owns
# a ky block: rows 8 kb ... 8 kb + 7, block 0 also the packed ky = N/2 row.  Blocks without weight are not launched, except
# block 0, which always is.
EDGE_SIZES = (32, 128, 256, 512)
EDGE_MASKS = ("without_ky_block_0", "ky_block_0_only")


def edge_mask(n: int, name: str) -> np.ndarray:
    """without_ky_block_0: the radial band minus every bin with |ky| < 8 — block 0 is launched with no weight at all (its
    rows, and the rows N/2 - 1 and N/2, have no bin in the compact q) and the other blocks come from the block list.
    ky_block_0_only: the band's bins with |ky| < 8 — the launch is one block wide, and every workgroup owns the packed row."""
    band = O.radial_band_mask(n, n)
    block0 = (np.abs(np.arange(n) - n // 2) < 8)[:, None]
    return band & (~block0 if name == "without_ky_block_0" else block0)


def edge_ky_blocks(n: int, name: str) -> int:
    """ky blocks the launch has under the mask (`fused_walk_footprint`'s "ky_blocks")."""
    return n // 16 if name == "without_ky_block_0" else 1


def edge_case(n: int) -> Case:
    return Case(n, segments_of(n, True), True)
