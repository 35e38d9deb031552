"""What tests/test_gpu_pair_handover.py and tests/test_pair_handover_host.py share: the grids, the image and the masks.

All at N = 512, the only size whose twist walk takes the runs two at a time.  The masks are there for the row's live mask
(a 64-bin group kx = 64 m .. 64 m + 63 of a spectrum row is skipped when no bin of it carries weight): between them a
row's groups are all live, live at the ends only, live in the middle only, live by a single bin, live on one side of the
meridian only (after the engine's fold of the plane onto its upper half), all dead in one row of a live ky block, and all dead outside ky block 0.
"""
from functools import lru_cache

import numpy as np

from oracle import path_b as O

N = 512
APIX, DIAMETER, BALL = 1.0, 0.4 * N, 2.0
TRUTH = (1.20, 4.75, 1)
RISES8 = 4.60 + 0.05 * np.arange(8)      # the truth is the fourth
TWISTS5 = 0.80 + 0.20 * np.arange(5)     # whole pairs and an odd tail; the truth is the third
TWISTS4 = 1.00 + 0.20 * np.arange(4)     # two whole pairs; the truth is the second
EMPTIED_ROW = 83                         # ky block 10's fourth row


@lru_cache(maxsize=None)
def oracle_image(seed=0):
    clean = O.simulate_helical_projection(1, TRUTH[0], TRUTH[1], TRUTH[2], DIAMETER, BALL, 0, 0, N, N, APIX)
    return (clean + np.random.default_rng(seed).normal(0, 0.5 * clean.std(), clean.shape)).astype(np.float32)


def _kx_positive():
    m = O.radial_band_mask(N, N)
    m[:, : N // 2 + 1] = False           # shifted plane: columns right of the meridian only (unshifted kx = 1 .. 255)
    return m


def _quadrant():
    """The engine folds the plane onto its upper half, W(k) = mask(k) + mask(-k): kx > 0 alone comes out symmetric but for
    the meridian; kx > 0 and ky > 0 leaves the folded rows without weight at negative kx (groups 4 - 7)."""
    m = _kx_positive()
    m[: N // 2 + 1, :] = False
    return m


def _row_emptied():
    m = O.radial_band_mask(N, N)
    m[N // 2 + EMPTIED_ROW, :] = False   # both shifted rows that fold onto spectrum row ky = EMPTIED_ROW
    m[N // 2 - EMPTIED_ROW, :] = False
    return m


def _block_0_only():
    m = O.radial_band_mask(N, N)
    ky = np.abs(np.arange(N) - N // 2)
    m[ky >= 8, :] = False
    return m


MASKS = {
    "default": lambda: O.radial_band_mask(N, N),
    "low_band": lambda: O.radial_band_mask(N, N, 2, 60),          # most rows keep groups 0 and 7 only
    "high_band": lambda: O.radial_band_mask(N, N, 200, 255),      # only the middle groups carry weight
    "layer_lines": lambda: O.layer_line_mask(N, N, axial_bins=(37, 150), half_width=0),   # single live bins in a group
    "kx_positive": _kx_positive,
    "quadrant": _quadrant,
    "row_emptied": _row_emptied,
    "block_0_only": _block_0_only,
}
