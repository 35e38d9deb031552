"""The band-mask probe of tests/spectrum_bands.py, checked on the CPU with the reference alone: the masks partition the
plane, a misplaced spectrum column moves its band's oracle score by at least ten times the tolerance the GPU census
(tests/test_gpu_row_lengths.py) applies to that band, and the host-side census of row lengths is 109 / 326 / 582."""
import numpy as np
import pytest

import spectrum_bands as SB
from oracle import path_b as O

# the issue's lengths; one two-step pair per compilation part of gen_rows.hip (part 0: 36 = 6 x 6, part 1: 64 = 8 x 8,
# part 2: 896 = 32 x 28, part 3: 35 = 7 x 5 — test_lengths_cover_every_compilation_part reads the lists); one length with a
# prime factor above 31; the widest Stockham-only lengths with their reduced probes
LENGTHS = (8, 26, 154, 169, 625, 961, 960, 1000, 1001, 1024, 36, 64, 896, 35, 80, 74, 997, 899, 1023)


@pytest.mark.parametrize("ny,nx,axis", [(3, 8, 1), (8, 8, 1), (24, 9, 1), (24, 26, 1), (24, 33, 1), (24, 960, 1), (24, 1001, 1),
                                       (8, 40, 0), (9, 40, 0), (33, 40, 0), (512, 16, 0), (1023, 8, 0)])
def test_band_masks_partition_the_plane(ny, nx, axis):
    m = SB.band_masks(ny, nx, axis)
    n = nx if axis == 1 else ny
    assert m.shape == (min(16, n // 2 + 1), ny, nx) and m.dtype == bool
    assert np.array_equal(m.sum(axis=0), np.ones((ny, nx), dtype=int))          # every bin in exactly one band
    assert m.any(axis=(1, 2)).all()                                             # no empty band
    k = np.abs(np.arange(n) - n // 2)
    line = m.any(axis=1) if axis == 1 else m.any(axis=2)                        # [bands, n]: the band's frequencies
    for b in range(len(m)):
        assert np.array_equal(m[b], np.broadcast_to(line[b][None, :] if axis == 1 else line[b][:, None], (ny, nx)))   # all of the other axis
        ks = np.unique(k[line[b]])
        assert np.array_equal(ks, np.arange(ks[0], ks[-1] + 1))                 # contiguous in |k| ...
        if b:
            assert ks[0] == np.unique(k[line[b - 1]])[-1] + 1                   # ... and in order
        mirror = (n // 2 - (np.arange(n) - n // 2)) % n                         # the place of -k (the Nyquist bin is its own)
        assert np.array_equal(line[b], line[b][mirror])                         # a band holds k and -k
    assert k[line[0]].min() == 0 and k[line[-1]].max() == n // 2


def test_probe_amplitude_is_the_oracle_spectrum_up_to_its_affine_normalisation():
    for ny, nx in ((24, 154), (24, 81), (9, 40)):
        probe = SB.Probe(ny, nx)
        for log in (True, False):
            a = SB.amplitude(probe.image, log)
            ref = O.reference_spectrum(probe.image, probe.apix, log=log)
            assert abs(O.cross_correlation_coefficient(a, ref) - 1.0) < 1e-12
            lo, hi = a.min(), a.max()
            np.testing.assert_allclose((a - lo) / (hi - lo), ref, rtol=0, atol=1e-12)


def test_probe_spectrum_has_no_empty_column():
    """Every column of the candidate's amplitude spectrum carries a speckle of its own, out to Nyquist."""
    for nx in (154, 960, 1001):
        o = SB.OracleSide(SB.probe_for_length(nx), log=False, with_floor=False)
        p = o.pwrs[0]
        col = p.std(axis=0)
        assert col.min() > 0.05 * np.median(col), (nx, col.min(), np.median(col))


def test_lengths_cover_every_compilation_part():
    """gen_rows.hip deals its pairs to four translation units (GEN_ROWS_PAIRS_0 ... 3): LENGTHS holds a pair of each."""
    import re
    from pathlib import Path

    src = (Path(__file__).resolve().parents[1] / "helicon_amd" / "csrc" / "gen_rows.hip").read_text()
    two, _, _ = SB.census()
    seen = 0
    for part in range(4):
        body = re.search(r"#define GEN_ROWS_PAIRS_%d\(X\)((?:.*\\\n)*.*)" % part, src).group(1)
        pairs = {(int(a), int(b)) for a, b in re.findall(r"X\((\d+), (\d+)\)", body)}
        assert len(pairs) >= 27 and all(two[a * b] == (a, b) for a, b in pairs), part
        assert any(two.get(nx) in pairs for nx in LENGTHS), part
        seen += len(pairs)
    assert seen == 109


@pytest.mark.parametrize("nx", LENGTHS)
@pytest.mark.parametrize("log", [True, False])
@pytest.mark.parametrize("second", [False, True])
def test_a_misplaced_column_moves_its_band_by_ten_tolerances(nx, log, second):
    """For the candidate an experimental image was made from: candidate 0 and the probe's image, the last candidate (Csym 2,
    the other twist and rise) and the second image."""
    probe = SB.probe_for_length(nx)
    o = SB.OracleSide(probe, log, image=probe.image2 if second else None)
    cand = probe.cand2 if second else 0
    assert (o.tol >= SB.ORACLE_TOL).all() and (o.tol == np.maximum(SB.ORACLE_TOL, 4 * o.floor)).all()
    swap = o.swap_sensitivity(cand)
    mirror = o.mirror_sensitivity(cand)
    print(f"nx {nx} log {log} second {second} units {len(probe.units)}: swap {swap.min():.2e}, mirror {mirror[1:-1].min() if len(mirror) > 2 else 0:.2e}, "
          f"floor {o.floor.max():.2e}, tol {o.tol.max():.2e}, ratio {(swap / o.tol).min():.0f}")
    assert (swap >= SB.MARGIN * o.tol).all(), (nx, log, swap / o.tol)
    # a band that holds more than its self-mirrored columns (kx = 0, Nyquist) sees a kx <-> -kx mirror as well — through
    # the Csym 1 candidate: a Csym 2 helix projects to an image that is symmetric about the axis, so its true spectrum is
    # its own kx mirror
    if second:
        assert mirror.max() < 1e-9
        return
    band = SB.band_of_frequency(nx)
    k = np.abs(np.arange(nx) - nx // 2)
    for b in range(len(mirror)):
        if np.any((band == b) & (k > 0) & (2 * k != nx)):
            assert mirror[b] >= SB.MARGIN * o.tol[b], (nx, log, b, mirror[b])


@pytest.mark.parametrize("ny,nx", [(8, 40), (17, 154), (40, 40), (65, 154), (255, 40), (1024, 154)])
def test_a_misplaced_row_moves_its_ky_band_by_ten_tolerances(ny, nx):
    probe = SB.probe_for_length(nx, ny)
    o = SB.OracleSide(probe, log=True, axis=0)
    swap = o.swap_sensitivity(0)
    o2 = SB.OracleSide(probe, log=True, axis=0, image=probe.image2)
    swap2 = o2.swap_sensitivity(probe.cand2)
    assert (swap2 >= SB.MARGIN * o2.tol).all(), (ny, nx, swap2 / o2.tol)
    print(f"ny {ny} nx {nx}: swap {swap.min():.2e}, floor {o.floor.max():.2e}, tol {o.tol.max():.2e}, ratio {(swap / o.tol).min():.0f}")
    assert (swap >= SB.MARGIN * o.tol).all(), (ny, nx, swap / o.tol)


def test_census_of_row_lengths():
    """109 lengths with an instantiated two-step pair, 326 more that are 31-smooth (Stockham kernel), 582 with a prime
    factor above 31 (float64 direct path); every pair keeps its kernel under the census's probe, and every Stockham-only
    length has a probe that fits the kernel's LDS."""
    two, stockham, direct = SB.census()
    assert (len(two), len(stockham), len(direct)) == (109, 326, 582)
    assert all(r1 * r2 == nx and r1 <= 32 and r2 <= 32 for nx, (r1, r2) in two.items())
    assert all(SB.is_31_smooth(nx) for nx in list(two) + stockham) and not any(SB.is_31_smooth(nx) for nx in direct)
    assert {37, 74, 127, 997, 1021} <= set(direct) and set(SB.DIRECT_SAMPLE) <= set(direct) and len(set(SB.DIRECT_SAMPLE)) >= 20
    # every prime radix of the Stockham kernel appears in a Stockham-only length
    for p in (7, 11, 13, 17, 19, 23, 29, 31):
        assert any(nx % p == 0 for nx in stockham), p
    for nx in two:
        assert len(SB.probe_for_length(nx).units) == 5, nx
    over = [nx for nx in stockham if SB.Probe(SB.NY, nx).stockham_lds() > SB.LDS_LIMIT]
    assert len(over) == 36 and min(over) == 891
    for nx in over:
        probe = SB.probe_for_length(nx)
        assert 2 <= len(probe.units) < 5 and probe.stockham_lds() <= SB.LDS_LIMIT
