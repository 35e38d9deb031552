"""The square-plane probe of tests/square_bands.py, checked on the CPU with the reference alone: on every compiled size of the
tuned sweep the band masks partition the plane; a swap of two adjacent spectrum lines of an image's own candidate moves its
band's oracle score by at least ten times the tolerance tests/test_gpu_square_bands.py holds that band to, on both axes and
for both spectra, and so does a kx <-> -kx mirror; no own-candidate band score is below 0.9; under every signed quadrant
mask a partner index one line off moves the score by at least ten tolerances; the list is 4 runs of 8 with one rise column;
and the table of subunits, the cases and UNREACHABLE agree with the library's host arithmetic.

Measured (smallest change over all bands; worst of log1p|F| and |F|, N = 1024 log1p|F| only):
    N     swap |kx| cand 0 / last   swap |ky| cand 0 / last   mirror    float32 floor   smallest own score   fold shift
    32    2.7e-1 / 2.4e-1           2.1e-1 / 4.0e-1           1.6e-1    6.1e-8          0.934                3.3e-1
    64    1.7e-1 / 6.7e-2           8.2e-2 / 9.6e-2           2.5e-1    6.3e-8          0.951                3.5e-1
    128   1.1e-1 / 7.1e-2           5.3e-2 / 5.4e-2           2.8e-1    4.9e-8          0.960                3.5e-1
    256   5.0e-2 / 3.7e-2           2.7e-2 / 3.0e-2           4.9e-1    5.7e-8          0.964                5.7e-1
    512   2.7e-2 / 2.5e-2           1.9e-2 / 1.3e-2           7.3e-1    5.8e-8          0.966                4.6e-1
    1024  1.3e-2 / 1.1e-2           1.1e-2 / 9.0e-3           7.1e-1    5.9e-8          0.965                6.1e-1
"""
import ctypes as C

import numpy as np
import pytest

import spectrum_bands as SB
import square_bands as Q
from helicon_amd import _lib
from tests import sweep_variants as SV

HOST_CASES = [c for c in Q.CASES if c[0] < 1024 or c[1]]      # N = 1024: the log spectrum only (the oracle's CPU time)


def test_cases_subunits_and_unreachable_agree_with_the_library():
    L = _lib.lib()
    assert Q.SIZES == SV.SIZES == (32, 64, 128, 256, 512, 1024) and list(Q.PATHS) == ["transform", "run_tables", "fused/rises", "fused/twists"]
    assert sorted(Q.CASES) == sorted((n, log, axis) for n in Q.SIZES for log in (False, True) for axis in (0, 1))
    assert len({Q.case_id(c) for c in Q.CASES}) == len(Q.CASES) == 24
    for n in Q.SIZES:
        fits = []
        for u in (5, 4, 3, 2):                              # the most subunits that fit: stop at the first
            if Q.footprint(n, None if u == Q.N_UNITS[n] else u) is not None:
                fits.append(u)
                break
        reachable = [p for p in ("fused/rises", "fused/twists") if (n, p) not in Q.UNREACHABLE]
        if not fits:                                        # no probe leaves the size on the fused pass: both walks are listed
            assert not reachable, n
            continue
        assert Q.N_UNITS[n] == max(fits) == len(Q.probe_of(n).units), (n, fits)
        assert reachable == ["fused/rises", "fused/twists"], n
        f = Q.footprint(n)
        built = L.hh_fused_lds_bytes(n, f["rows"], f["kg"], 2) > 0
        assert built == SV.twist_walk_built(n) == (f["lds_twists"] > 0)
        assert 0 < f["kg"] <= 16 and f["kg"] % Q.N_UNITS[n] == 0 and 0 < f["lds_rises"] <= 160 * 1024 - 1024
        assert Q.expected(n, "fused/rises") == ("fused", "rises", 8)
        assert Q.expected(n, "fused/twists") == ("fused", "twists" if built else "rises", 8)
        assert Q.expected(n, "transform") == ("transform", "none", 0) and Q.expected(n, "run_tables") == ("run_tables", "none", 0)
    for (n, path), reason in Q.UNREACHABLE.items():
        assert n in Q.SIZES and path in ("fused/rises", "fused/twists") and reason
    assert {n: Q.footprint(n)["kg"] for n in Q.SIZES} == {32: 15, 64: 15, 128: 15, 256: 10, 512: 10, 1024: 10}


@pytest.mark.parametrize("n", Q.SIZES)
def test_list_is_four_runs_of_eight_with_one_rise_column(n):
    L = _lib.lib()
    probe, base = Q.probe_of(n), SB.Probe(n, n, Q.N_UNITS[n])
    g = probe.params
    assert g.shape == (32, 4) and g.flags.c_contiguous and (g[:, 3] == 0).all()
    assert (g[:, 2].reshape(2, 16) == np.array(SB.CSYMS)[:, None]).all()                       # Csym-major ...
    assert (g[:, 0].reshape(2, 2, 8) == np.array(SB.TWISTS)[None, :, None]).all()              # ... then twist ...
    assert (g[:, 1].reshape(4, 8) == np.linspace(base.rises[0], 1.06 * base.rises[0], 8)[None, :]).all()   # ... then rise
    assert len(set(g[:8, 1])) == 8 and L.hh_rise_columns_shared(g.ctypes.data_as(C.POINTER(C.c_double)), 32, 8) == 1
    # geometry, units and both images are Probe(N, N)'s own; they were made from this list's first and last candidates
    assert probe.geometry()["apix"] == 2.0 and probe.diameter == 0.8 * n * 2.0 and probe.ball_radius == 1.0
    assert np.array_equal(probe.units, base.units) and np.array_equal(probe.image, base.image) and np.array_equal(probe.image2, base.image2)
    assert np.array_equal(g[0], base.params[0]) and np.array_equal(g[-1], base.params[-1]) and probe.cand2 == 31
    assert probe.diameter + probe.ball_radius < n * probe.apix * 0.99
    p = Q.picks(n)
    assert len(p) == len(set(p)) and p == sorted(p) and p[0] == 0 and p[-1] == 31
    if n <= 256:
        assert p == list(range(32))
    elif n == 512:
        assert p == [0, 7, 8, 15, 16, 23, 24, 31]                                              # both sides of each run boundary
    else:
        assert len(p) == 4
    fp = Q.fold_picks(n)
    assert len(fp) == 4 and fp[0] == 0 and fp[-1] == 31 and len(set(fp)) == 4


@pytest.mark.parametrize("axis", [1, 0])
@pytest.mark.parametrize("n", Q.SIZES)
def test_band_masks_partition_the_square_plane(n, axis):
    m = SB.band_masks(n, n, axis)
    assert m.shape == (16, n, n) and m.dtype == bool
    assert np.array_equal(m.sum(axis=0), np.ones((n, n), dtype=int))            # every bin in exactly one band
    assert m.any(axis=(1, 2)).all()
    lines = m.any(axis=2 - axis)                                                # [bands, n]: whole lines of the other axis
    assert np.array_equal(m, np.broadcast_to(lines[:, :, None] if axis == 0 else lines[:, None, :], m.shape))
    minus = (n - np.arange(n)) % n                                              # the place of -k on an fftshifted even axis
    assert np.array_equal(m, m[:, minus][:, :, minus])                          # a band holds k and -k: its fold weights are 0 or 2


@pytest.mark.parametrize("case", HOST_CASES, ids=Q.case_id)
def test_a_swapped_line_moves_its_band_by_ten_tolerances(case):
    n, log, axis = case
    paired = Q.paired_bands(n)
    assert len(paired) >= 15
    for image in (0, 1):
        o = Q.oracle_side(n, log, axis, image, "own")
        assert o.scores.shape == (16, 1) and np.isfinite(o.scores).all()
        assert (o.tol == np.maximum(Q.ORACLE_TOL, 4 * o.floor)).all() and (o.tol <= Q.SCORE_TOL).all()
        swap = o.swap_sensitivity(0)
        mirror = o.mirror_sensitivity(0)
        print(f"{Q.case_id(case)} image {image}: swap {swap.min():.2e}, mirror {mirror[paired].min():.2e}, floor {o.floor.max():.2e}, "
              f"tolerance {o.tol.max():.1e}, swap / tolerance {(swap / o.tol).min():.0f}, smallest own score {o.scores.min():.3f}")
        assert swap.shape == (16,) and (swap >= Q.MARGIN * o.tol).all(), (case, image, swap / o.tol)
        assert (o.scores[:, 0] >= Q.MIN_OWN_SCORE).all(), (case, image, o.scores[:, 0])
        if image == 0:      # a Csym 2 helix projects to an image that is its own mirror (tests/test_spectrum_bands_host.py)
            assert (mirror[paired] >= Q.MARGIN * o.tol[paired]).all(), (case, mirror / o.tol)
        else:
            assert mirror.max() < 1e-9


@pytest.mark.parametrize("n", Q.SIZES)
def test_a_fold_partner_one_line_off_moves_its_quadrant_mask_by_ten_tolerances(n):
    f = Q.fold_side(n)
    k = np.arange(n) - n // 2
    assert len(f.masks) == len(f.names) >= 63 and f.scores.shape == (2, len(f.masks), 4)
    minus = (n - np.arange(n)) % n
    for m, (axis, b, sign) in zip(f.masks, f.names):
        assert m.sum() >= Q.MIN_FOLD_BINS and not m[k >= 0].any() and not m[:, k * sign <= 0].any()    # ky < 0, one sign of kx
        own = m & m[minus][:, minus]                # W is mask(-k) alone: no bin meets its partner, but for the bin that is its
        own[0, 0] = False                           # own (ky = kx = -N/2, in the last band of the kx < 0 masks)
        assert not own.any()
        assert not (m & ~SB.band_masks(n, n, axis)[b]).any()
    assert {(a, s) for a, _, s in f.names} == {(1, 1), (1, -1), (0, 1), (0, -1)}
    assert (f.tol == np.maximum(Q.ORACLE_TOL, 4 * f.floor)).all() and (f.tol <= Q.SCORE_TOL).all()
    for image in (0, 1):
        own = 3 if image else 0
        shift = f.shift_sensitivity(image)
        print(f"n{n} image {image}: {len(f.masks)} quadrant masks, smallest one-line shift {shift.min():.2e}, floor {f.floor.max():.2e}, "
              f"smallest own score {f.scores[image, :, own].min():.3f}")
        assert (shift >= Q.MARGIN * f.tol).all(), (n, image, shift / f.tol)
        assert (f.scores[image, :, own] >= 0.5).all()
