"""Structure factors on the device (hh_sf_*; helicon_amd/structure_factor.py) against the float64 restatement of the reference
(tests/structure_factor_oracle.py, pinned to the reference by tests/golden/g24_structure_factor.npz) and against the
reference's recorded output.

Two probes decide the binning rule exactly: a unit impulse has |F|^2 = 1 everywhere, so its profile must round to the
reference's voxel counts per bin; and a cosine at a frequency that ties with a bin edge carries most of a small map's power,
so a voxel put on the wrong side of the edge moves the profile and the matched map far outside any tolerance
(tests/test_structure_factor_host.py shows that each plausible wrong rule is noticed).

Inputs carry a white noise floor (every bin's mean power per voxel at least 1e-4 of the strongest bin's; asserted here on
every input): a float32 transform's error is relative to the whole map.  No bin and no case is left out of a comparison.

Bounds: the largest error against float64 measured on an MI355X over the cases of this file (profiles/structure_factor.json,
"accuracy") times 4, rounded up to one significant digit; a matched map's bound is never above 4e-6 max|want| (forward plus
inverse: six passes, twice the rule of tests/fft_resample_oracle.py).  Measured maxima: per-bin sums 3.2e-7 of the bin's own
sum (33 x 47, mask), matched maps 4.3e-7 of max|want| (12 x 20 x 36 on the matcher, mask and thresh; 3.8e-7 on the fixture).
The spike maps have bounds of their own, because their bins of noise sit beside a bin 1e3 times stronger per voxel and a
float32 transform's error is relative to the whole map: sums 6.5e-7 (24 x 20), maps 8.0e-7 (9^3, apix 5.0).  Every
test prints its figure before it asserts."""
import numpy as np
import pytest

import structure_factor_oracle as O
import helicon_amd as H
from helicon_amd import structure_factor as S
from helicon_amd.mrc import read_mrc, write_mrc

pytestmark = pytest.mark.gpu

TOL_SF = 2e-6      # per bin, of the bin's own sum: 3.2e-7 measured x 4
TOL_MATCH = 2e-6   # of max |want|: 4.3e-7 measured x 4 (the cap is 4e-6)
TOL_SF_SPIKE = 3e-6     # the spike maps: 6.5e-7 measured x 4
TOL_MATCH_SPIKE = 4e-6  # 8.0e-7 measured x 4 (and the cap)
FLOOR = 1e-4


@pytest.fixture(scope="module")
def g24(golden_dir):
    return np.load(golden_dir / "g24_structure_factor.npz")


def _sf_error(got, want):
    assert (want > 0).all()
    return float(np.abs(got / want - 1.0).max())


def _map_error(got, want):
    return float(np.abs(got - want).max() / np.abs(want).max())


# ---------------------------------------------------------------------------------------------------------------------------
# the impulse probe
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,apix", O.FIXTURE_CASES + O.IMPULSE_EXTRA, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_impulse_profile_is_the_voxel_count_of_every_bin(shape, apix):
    data = np.zeros(shape, dtype=np.float32)
    data[(0,) * len(shape)] = 1.0
    qbins, sf = H.calculate_structural_factor(data, apix)
    want_qbins = O.bins(shape, apix)[0]
    want = O.counts(shape, apix)
    assert qbins.dtype == np.float64 and np.array_equal(qbins, want_qbins)          # bit-equal to the reference's linspace
    dev = float(np.abs(sf - want).max())
    print(f"SF_FIGURE impulse shape={shape} apix={apix} nbins={len(qbins)} max|sf - count|={dev:.3e}")
    assert sf.dtype == np.float64 and np.array_equal(np.round(sf).astype(np.int64), want)
    assert int(want.sum()) == int(np.prod(shape))                                   # the weighted half counts the full spectrum


# ---------------------------------------------------------------------------------------------------------------------------
# the spike probe
# ---------------------------------------------------------------------------------------------------------------------------
def _spike_map(shape, k, seed):
    rng = np.random.default_rng(seed)
    grids = np.meshgrid(*[np.arange(n) for n in shape], indexing="ij")
    phase = 2.0 * np.pi * sum(kk * g / n for kk, g, n in zip(k, grids, shape))
    return (rng.standard_normal(shape) + 10.0 * np.cos(phase + 0.3)).astype(np.float32)


SPIKE_TARGET_FACTOR = 0.8   # the target reaches beyond the data's last edge: ratio[-1] != 0, so "at" and "above" differ in the map
SPIKES = [((8, 8, 8), (4, 4, 2), 1.0, "at"), ((8, 8, 8), (4, 4, 2), 0.83, "below"),
          ((9, 9, 9), None, 1.0, "at"), ((9, 9, 9), None, 1.7, "below"), ((9, 9, 9), None, 5.0, "above"),
          ((24, 20), (0, 8), 1.5, "at")]


@pytest.mark.parametrize("shape,k,apix,verdict", SPIKES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_spike_at_a_tie_frequency(shape, k, apix, verdict):
    ties = O.tie_voxels(shape, apix)
    if k is None:
        k = ties[0][0]                                       # a tie triple of the 9^3 cube
    found = {idx: (edge, v) for idx, edge, v in ties}
    assert found[tuple(k)][1] == verdict                     # the reference's own verdict at this voxel size
    data = _spike_map(shape, k, 77)
    target = _spike_map(shape, k, 78) * 0.5
    qbins, want_sf = O.calculate_structural_factor(data, apix)
    power_share = float(want_sf[found[tuple(k)][0] - (verdict == "below")] / want_sf.sum())
    assert power_share > 0.9                                 # the spike's bin holds the map's power: a wrong verdict moves it
    got_qbins, got_sf = H.calculate_structural_factor(data, apix)
    assert np.array_equal(got_qbins, qbins)
    want = O.match_structural_factors(data, apix, target, apix * SPIKE_TARGET_FACTOR)
    got = H.match_structural_factors(data, apix, target, apix * SPIKE_TARGET_FACTOR)
    e_sf, e_map = _sf_error(got_sf, want_sf), _map_error(got, want)
    print(f"SF_FIGURE spike shape={shape} k={tuple(k)} apix={apix} verdict={verdict} share={power_share:.3f} sf={e_sf:.3e} match={e_map:.3e}")
    assert e_sf <= TOL_SF_SPIKE and e_map <= TOL_MATCH_SPIKE


# ---------------------------------------------------------------------------------------------------------------------------
# parity
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(len(O.FIXTURE_CASES)), ids=lambda k: "x".join(map(str, O.FIXTURE_CASES[k][0])) + f"-{O.FIXTURE_CASES[k][1]}")
def test_fixture_cases_against_the_reference_and_the_restatement(g24, k):
    shape, apix = O.FIXTURE_CASES[k]
    data, target, mask = (g24[f"c{k}_{n}"].astype(np.float32) for n in ("data", "target", "mask"))
    apix_t = apix * float(g24["apix_target_factor"][0])
    for variant in O.VARIANTS:
        thresh, thresh_t, m = O.variant_args(variant, mask)
        key = O.case_key(k, variant)
        ref_sf, ref_match = g24[f"{key}_sf"], g24[f"{key}_match"]
        assert O.floor_ratio(shape, apix, ref_sf) >= FLOOR and O.floor_ratio(shape, apix_t, g24[f"{key}_tsf"]) >= FLOOR
        qbins, sf = H.calculate_structural_factor(data, apix, thresh, m)
        assert np.array_equal(qbins, g24[f"{key}_qbins"]) and sf.dtype == np.float64
        got = H.match_structural_factors(data, apix, target, apix_t, thresh, thresh_t, m)
        got_set = H.set_structural_factors(data, apix, g24[f"{key}_tbins"], g24[f"{key}_tsf"], thresh, m)
        assert got.dtype == np.float64 and got.shape == tuple(shape)
        own_sf = O.calculate_structural_factor(data, apix, thresh, m)[1]
        own_match = O.match_structural_factors(data, apix, target, apix_t, thresh, thresh_t, m)
        e = (_sf_error(sf, ref_sf), _sf_error(sf, own_sf), _map_error(got, ref_match), _map_error(got, own_match), _map_error(got_set, ref_match))
        print(f"SF_FIGURE fixture shape={shape} apix={apix} {variant}: sf={e[0]:.3e} (restatement {e[1]:.3e}) match={e[2]:.3e} "
              f"(restatement {e[3]:.3e}) set={e[4]:.3e}")
        assert max(e[0], e[1]) <= TOL_SF and max(e[2], e[3], e[4]) <= TOL_MATCH


def test_return_fft_is_the_full_spectrum(g24):
    for k in (5, 8):   # an unequal odd box and an odd image
        shape, apix = O.FIXTURE_CASES[k]
        data, mask = g24[f"c{k}_data"].astype(np.float32), g24[f"c{k}_mask"].astype(np.float32)
        qbins, sf, F = H.calculate_structural_factor(data, apix, O.THRESH, mask, True)
        want = O.calculate_structural_factor(data, apix, O.THRESH, mask, True)[2]
        e = float(np.abs(F - want).max() / np.abs(want).max())
        print(f"SF_FIGURE spectrum shape={shape} max|F - float64| / max|F| = {e:.3e}")
        assert F.shape == tuple(shape) and F.dtype == np.complex128 and e <= TOL_MATCH


def test_target_of_another_shape_and_voxel_size_and_an_empty_tail():
    shape, apix = (15, 18, 21), 1.7
    data = O.make_inputs(shape, 31)[0]
    target = O.make_inputs((20, 14, 26), 32)[1]
    want = O.match_structural_factors(data, apix, target, 1.2)
    got = H.match_structural_factors(data, apix, target, 1.2)
    e_shape = _map_error(got, want)
    # a target profile that ends inside the data's range: fill_value = 0 gives ratio 0 on the tail
    qbins, sf = O.calculate_structural_factor(data, apix)
    tbins, tsf = qbins[: len(qbins) // 2] * 1.01, sf[: len(qbins) // 2][::-1].copy()
    want = O.set_structural_factors(data, apix, tbins, tsf)
    got = H.set_structural_factors(data, apix, tbins, tsf)
    tail = O.calculate_structural_factor(got, apix)[1][len(qbins) // 2 + 1:]
    e_tail = _map_error(got, want)
    print(f"SF_FIGURE other target: match={e_shape:.3e}; empty tail: set={e_tail:.3e} tail power / total = {float(tail.sum() / sf.sum()):.3e}")
    assert e_shape <= TOL_MATCH and e_tail <= TOL_MATCH
    assert tail.sum() <= 1e-10 * sf.sum()


# ---------------------------------------------------------------------------------------------------------------------------
# determinism and the batch
# ---------------------------------------------------------------------------------------------------------------------------
def test_sums_and_matched_maps_do_not_depend_on_the_run_or_the_batch():
    shape, apix = (12, 20, 36), 1.1
    maps = np.stack([O.make_inputs(shape, 50 + j)[0] for j in range(5)])
    target, mask = O.make_inputs(shape, 60)[1:]
    tbins, tsf = O.calculate_structural_factor(target, 1.4, O.THRESH_TARGET, mask)
    with H.StructureFactorMatcher(shape, apix, tbins, tsf) as m:
        for kw in (dict(), dict(mask=mask, thresh=O.THRESH)):
            sf1, sf2 = m.profile(maps, **kw), m.profile(maps, **kw)
            out1, out2 = m.match(maps, **kw), m.match(maps, **kw)
            assert np.array_equal(sf1, sf2) and np.array_equal(out1, out2)                       # run to run
            alone_sf, alone_out = m.profile(maps[2], **kw), m.match(maps[2], **kw)
            for order in ([2, 0, 1], [0, 1, 2], [3, 2, 4, 0]):                                    # first, last, in the middle
                at = order.index(2)
                assert np.array_equal(m.profile(maps[order], **kw)[at], alone_sf)
                assert np.array_equal(m.match(maps[order], **kw)[at], alone_out)
            singles = np.stack([m.match(x, **kw) for x in maps])
            assert np.array_equal(out1, singles)                                                  # B maps = B single calls
            want = O.set_structural_factors(maps[2], apix, tbins, tsf, **kw)
            e = _map_error(alone_out, want)
            print(f"SF_FIGURE matcher {sorted(kw)}: match={e:.3e}")
            assert e <= TOL_MATCH


def test_a_batch_across_the_chunk_cap():
    """65535 // nz maps per launch of the y pass: 8191 at nz = 8 (pinned by tests/test_structure_factor_host.py)."""
    shape, apix, batch = (8, 2, 2), 1.0, 8200
    cap = 65535 // shape[0]
    assert cap < batch < 2 * cap
    rng = np.random.default_rng(9)
    maps = rng.standard_normal((batch,) + shape).astype(np.float32)
    tbins, tsf = O.calculate_structural_factor(rng.standard_normal(shape), apix)
    with H.StructureFactorMatcher(shape, apix, tbins, tsf) as m:
        out, sf = m.match(maps, return_profile=True)
        worst_sf = worst = 0.0
        for j in (0, 1, cap - 1, cap, cap + 1, batch - 1):
            assert np.array_equal(m.profile(maps[j]), sf[j]) and np.array_equal(m.match(maps[j]), out[j])
            worst_sf = max(worst_sf, _sf_error(sf[j], O.calculate_structural_factor(maps[j], apix)[1]))
            worst = max(worst, _map_error(out[j], O.set_structural_factors(maps[j], apix, tbins, tsf)))
        print(f"SF_FIGURE chunks batch={batch} cap={cap}: sf={worst_sf:.3e} match={worst:.3e}")
        assert worst_sf <= TOL_SF and worst <= TOL_MATCH


# ---------------------------------------------------------------------------------------------------------------------------
# edges
# ---------------------------------------------------------------------------------------------------------------------------
def test_edges():
    for shape in ((2, 2, 2), (3, 3, 3)):
        with pytest.raises(ValueError, match="nbins"):
            H.calculate_structural_factor(np.ones(shape, np.float32), 1.0)
    data, target, mask = O.make_inputs((9, 9, 9), 5)
    with pytest.raises(ValueError, match="mask"):
        H.calculate_structural_factor(data, 1.0, None, mask[:8])
    with pytest.raises(ValueError, match="mask"):
        H.match_structural_factors(data, 1.0, target, 1.0, mask=np.ones((9, 9, 8), np.float32))
    # thresh = 0 is no threshold (`if thresh:`)
    assert np.array_equal(H.calculate_structural_factor(data, 1.0, 0)[1], H.calculate_structural_factor(data, 1.0)[1])
    assert np.array_equal(H.match_structural_factors(data, 1.0, target, 1.3, 0, 0), H.match_structural_factors(data, 1.0, target, 1.3))
    # a NaN: NaN sums, no fault, and the next call is sound
    bad = data.copy()
    bad[3, 4, 5] = np.nan
    assert np.isnan(H.calculate_structural_factor(bad, 1.0)[1]).all()
    assert np.isfinite(H.calculate_structural_factor(data, 1.0)[1]).all()
    # a bin with sf == 0 gives ratio 0: an all-zero map comes back as zeros
    zeros = H.match_structural_factors(np.zeros((9, 9, 9), np.float32), 1.0, target, 1.0)
    assert np.array_equal(zeros, np.zeros((9, 9, 9)))
    assert np.array_equal(H.calculate_structural_factor(np.zeros((9, 9, 9), np.float32), 1.0)[1], np.zeros(6))


def test_command_line_round_trip(tmp_path, capsys):
    shape, apix = (12, 20, 36), 1.1
    data, target, mask = O.make_inputs(shape, 70)
    write_mrc(tmp_path / "in.mrc", data, apix)
    write_mrc(tmp_path / "target.mrc", target, 1.4)
    write_mrc(tmp_path / "mask.mrc", mask, apix)
    apix32, apix_t32 = read_mrc(tmp_path / "in.mrc")[1], read_mrc(tmp_path / "target.mrc")[1]   # as the header holds them
    assert S.main([str(tmp_path / "in.mrc"), str(tmp_path / "out.mrc"), "--target", str(tmp_path / "target.mrc"), "--mask",
                   str(tmp_path / "mask.mrc"), "--thresh", "0.75", "--thresh-target", "0.5"]) == 0
    out, apix_out = read_mrc(tmp_path / "out.mrc")
    want = O.match_structural_factors(data, apix32, target, apix_t32, 0.75, 0.5, mask)
    e = _map_error(np.asarray(out, dtype=np.float64), want)
    print(f"SF_FIGURE command line: match={e:.3e} apix {apix_out}")
    assert out.shape == shape and apix_out == pytest.approx(apix, rel=1e-6) and e <= TOL_MATCH
    capsys.readouterr()
    assert S.main([str(tmp_path / "in.mrc"), "--profile"]) == 0
    rows = np.array([[float(v) for v in line.split()] for line in capsys.readouterr().out.strip().splitlines()])
    qbins, sf = O.calculate_structural_factor(data, apix32)
    assert np.array_equal(rows[:, 0], qbins) and _sf_error(rows[:, 1], sf) <= TOL_SF
