"""The case table of tests/sweep_variants.py against the library's own dispatch and host arithmetic (no GPU), and the
float64 oracle alone on the table's small cases and edge masks: the inputs of tests/test_gpu_sweep_variants.py are legitimate
before any device sees them."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

from helicon_amd import _lib
from oracle import path_b as O
from tests import sweep_variants as SV

SOURCE = Path(__file__).resolve().parent.parent / "helicon_amd" / "csrc" / "helicon_hip.hip"


def switch_sizes():
    """The sizes HH_SWITCH_N dispatches, from the source text."""
    text = SOURCE.read_text()
    body = re.search(r"#define HH_SWITCH_N\(c, CALL\)(.*?)return fail", text, re.S)
    assert body, "HH_SWITCH_N not found"
    return tuple(int(v) for v in re.findall(r"case (\d+):", body.group(1)))


def test_table_is_the_full_product_of_the_dispatched_sizes():
    sizes = switch_sizes()
    assert len(sizes) >= 6 and sizes == SV.SIZES and set(SV.AXES) == set(sizes)
    assert len(SV.CASES) == 4 * len(sizes) == len({c.id for c in SV.CASES})
    for n in sizes:
        rows = [c for c in SV.CASES if c.n == n]
        assert sorted((c.segments > 1, c.log) for c in rows) == [(False, False), (False, True), (True, False), (True, True)]
        assert {c.segments for c in rows} == {1, 3 if n < 512 else 2}


def test_every_row_has_the_four_paths_and_the_walk_the_library_builds():
    L = _lib.lib()
    assert list(SV.PATHS) == ["transform", "run_tables", "fused/rises", "fused/twists"]
    assert [SV.PATHS[p][0] for p in SV.PATHS] == [0, 1, 2, 2]
    for case in SV.CASES:
        built = L.hh_fused_lds_bytes(case.n, 140, 7, 2) > 0           # 0: twist_walk_built(N) says no
        assert built == SV.twist_walk_built(case.n)
        assert case.expected("fused/rises") == ("fused", "rises", 8)
        assert case.expected("fused/twists") == ("fused", "twists" if built else "rises", 8)
        assert case.expected("transform") == ("transform", "none", 0)
        assert case.expected("run_tables") == ("run_tables", "none", 0)
    assert [n for n in SV.SIZES if not SV.twist_walk_built(n)] == [1024]


def test_grids_are_three_runs_of_eight_shared_rises():
    L = _lib.lib()
    for case in SV.CASES:
        g = case.grid
        assert g.shape == (24, 4) and g.flags.c_contiguous and (g[:, 2] == 1).all() and (g[:, 3] == 0).all()
        assert (g[:, 0].reshape(3, 8) == case.twists[:, None]).all()                     # twist-major
        assert len(set(case.twists)) == 3 and len(set(case.rises)) == 8
        assert L.hh_rise_columns_shared(g.ctypes.data_as(C.POINTER(C.c_double)), 24, 8) == 1
        assert tuple(g[12, :3]) == case.truth
        # the fused pass's factor rows: kg = floor(((3 + 2 rpx) apix + 2 slack) / rise) + 2 <= 16 with rpx 10, slack 1e-3
        assert int(np.floor(23.002 / case.rises.min())) + 2 <= 16
        geo = case.geometry
        assert geo["helical_diameter"] + geo["ball_radius"] < case.n * geo["apix"] * 0.99


def test_rises_at_128_leave_the_walks_to_the_lds():
    """tests/sweep_variants.py: from rise 2.0 (table extent 38 -> 77 -> 84 staged rows, kg 13) a compute unit's 160 KB hold 5
    rise-walking and 6 twist-walking workgroups — not more than the 6 the registers of the several-segment twist walk allow,
    so a forced twist walk is not given to the rise walk."""
    L = _lib.lib()
    rise = float(SV.Case(128, 1, True).rises.min())
    ext = int(L.hh_table_extent(128, SV.APIX, 10, 1e-3, rise))
    kg = int(np.floor(23.002 / rise)) + 2
    rows = 2 * ext + 1
    rows += (4 - rows % 8 + 8) % 8
    assert (rise, ext, kg, rows) == (2.0, 38, 13, 84)
    assert (L.hh_fused_lds_bytes(128, rows, kg, 1), L.hh_fused_lds_bytes(128, rows, kg, 2)) == (27424, 26000)
    assert (163840 // 27424, 163840 // 26000) == (5, 6)


def test_unreachable_names_only_forms_of_the_table():
    for (n, path), reason in SV.UNREACHABLE.items():
        assert n in SV.SIZES and path in ("fused/rises", "fused/twists") and reason == "footprint"


def test_picks_meet_the_minimum_counts():
    for n in SV.SIZES:
        p = SV.picks(n)
        assert len(p) == len(set(p)) >= SV.MIN_PICKS[n] and min(p) == 0 and max(p) == 23
        if n <= 128:
            assert p == list(range(24))
        elif n <= 512:
            assert {0, 23, 8 + 1, 16} <= set(p)       # first, last, second run's second rise, last run's first rise
    assert SV.MIN_PICKS == {32: 24, 64: 24, 128: 24, 256: 4, 512: 4, 1024: 2}


def test_tolerances_come_from_the_transform_measurements():
    assert SV.PIPE_TOL == 2e-5 and SV.SCORE_TOL == 2e-4
    for n in SV.SIZES:
        assert SV.LINEAR_TOL[n] == min(2e-4, max(2e-5, 4 * SV.TRANSFORM_LINEAR_ERR[n]))
        assert 2e-5 <= SV.LINEAR_TOL[n] <= 2e-4


@pytest.mark.parametrize("case", [c for c in SV.CASES if c.n <= 128], ids=lambda c: c.id)
def test_oracle_alone_scores_the_small_rows(case):
    imgs = SV.images(case, SV.oracle_simulate(case))
    ref = SV.oracle_scores(case, imgs, case.picks)
    assert ref.shape == (case.segments, 24) and np.isfinite(ref).all()
    assert (ref.std(axis=1) > 1e-3).all() and (np.abs(ref) < 1).all()


@pytest.mark.parametrize("name", SV.EDGE_MASKS)
@pytest.mark.parametrize("n", [32, 128])
def test_oracle_alone_scores_under_the_edge_masks(n, name):
    case, mask = SV.edge_case(n), SV.edge_mask(n, name)
    band = O.radial_band_mask(n, n)
    ky = np.abs(np.arange(n) - n // 2)
    assert mask.any() and not (mask & ~band).any()
    assert mask[ky < 8].any() == (name == "ky_block_0_only") and mask[ky >= 8].any() == (name == "without_ky_block_0")
    assert (SV.edge_mask(n, "without_ky_block_0") | SV.edge_mask(n, "ky_block_0_only") == band).all()
    minus = (n - np.arange(n)) % n                          # index of -k on an fftshifted axis of even length
    assert np.array_equal(mask, mask[np.ix_(minus, minus)])
    imgs = SV.images(case, SV.oracle_simulate(case))
    assert case.log and case.segments == 3
    # the correlation's denominators: both masked spectra vary
    for img in imgs:
        assert O.reference_spectrum(img, SV.APIX, log=True)[mask].std() > 0
    sim = SV.oracle_simulate(case)(*case.truth)
    assert O.compute_power_spectra(sim, SV.APIX, log=True)[0][mask].std() > 0
    ref = SV.oracle_scores(case, imgs, case.picks, mask)
    assert ref.shape == (3, 24) and np.isfinite(ref).all() and (ref.std(axis=1) > 1e-3).all()
    # ky blocks with weight: rows 8 kb ... 8 kb + 7 of the half plane; block 0 is launched whatever it weighs
    blocks = {int(k) // 8 for k in ky[mask.any(axis=1)] if k < n // 2} | {0}
    assert len(blocks) == SV.edge_ky_blocks(n, name)
