"""Host side of the structure factors: the float64 restatement (tests/structure_factor_oracle.py) equals the reference's
recorded output, the tie census of the binning rule, the GPU tests' probes notice every plausible wrong rule, and the
package's host arithmetic, header and argument checks.  Nothing here needs a GPU."""
import re
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import structure_factor_oracle as O
import test_gpu_structure_factor as G
from helicon_amd import _lib
from helicon_amd import structure_factor as S

ROOT = Path(__file__).resolve().parent.parent
SMALL_IMPULSE = [c for c in O.FIXTURE_CASES + O.IMPULSE_EXTRA if np.prod(c[0]) <= 10000]


@pytest.fixture(scope="module")
def g24(golden_dir):
    return np.load(golden_dir / "g24_structure_factor.npz")


def test_the_restatement_equals_the_reference(g24):
    assert [tuple(int(v) for v in s if v) for s in g24["shapes"]] == [s for s, _ in O.FIXTURE_CASES]
    assert np.array_equal(g24["apix"], [a for _, a in O.FIXTURE_CASES])
    assert any(v.startswith("numpy ") for v in g24["versions"]) and any(v.startswith("scipy ") for v in g24["versions"])
    for k, (shape, apix) in enumerate(O.FIXTURE_CASES):
        data, target, mask = (g24[f"c{k}_{n}"].astype(np.float64) for n in ("data", "target", "mask"))
        apix_t = apix * float(g24["apix_target_factor"][0])
        for variant in O.VARIANTS:
            thresh, thresh_t, m = O.variant_args(variant, mask)
            key = O.case_key(k, variant)
            qbins, sf = O.calculate_structural_factor(data, apix, thresh, m)
            tbins, tsf = O.calculate_structural_factor(target, apix_t, thresh_t, m)
            assert np.array_equal(qbins, g24[f"{key}_qbins"]) and np.array_equal(tbins, g24[f"{key}_tbins"])
            # the same labels, another order of the float64 sums
            assert np.allclose(sf, g24[f"{key}_sf"], rtol=1e-12, atol=0) and np.allclose(tsf, g24[f"{key}_tsf"], rtol=1e-12, atol=0)
            want = g24[f"{key}_match"]
            for got in (O.match_structural_factors(data, apix, target, apix_t, thresh, thresh_t, m),
                        O.set_structural_factors(data, apix, g24[f"{key}_tbins"], g24[f"{key}_tsf"], thresh, m)):
                assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()


def test_the_raw_spectrum_quirk_is_in_the_fixture(g24):
    """with a mask the reference scales the spectrum of the raw data: scaling the masked one is far from the recorded output"""
    for k, (shape, apix) in enumerate(O.FIXTURE_CASES):
        data, target, mask = (g24[f"c{k}_{n}"].astype(np.float64) for n in ("data", "target", "mask"))
        for variant in ("mask", "both"):
            thresh, thresh_t, m = O.variant_args(variant, mask)
            want = g24[f"{O.case_key(k, variant)}_match"]
            wrong = O.match_structural_factors(data, apix, target, apix * O.TARGET_APIX_FACTOR, thresh, thresh_t, m, rule="masked_spectrum")
            assert np.abs(wrong - want).max() > 1e4 * G.TOL_MATCH * np.abs(want).max()


# ---------------------------------------------------------------------------------------------------------------------------
# the tie census
# ---------------------------------------------------------------------------------------------------------------------------
def _census(shape, apix):
    ties = O.tie_voxels(shape, apix)
    lab = O.labels(shape, apix)
    for idx, edge, verdict in ties:   # the verdict is the label
        assert lab[idx] == (edge - 1 if verdict == "below" else edge)
    return len(ties), sorted({e for _, e, _ in ties}), sorted({v for _, _, v in ties})


@pytest.mark.parametrize("n,nbins", [(8, 6), (16, 12)])
def test_cubes_of_side_8_and_16_tie_with_the_last_edge(n, nbins):
    assert len(O.bins((n,) * 3, 1.0)[0]) == nbins
    for apix in (1.0, 1.3, 2.2):
        assert _census((n,) * 3, apix) == (6, [nbins - 1], ["at"])
    for apix in (0.83, 0.9, 5.0):
        assert _census((n,) * 3, apix) == (6, [nbins - 1], ["below"])
    want = {tuple(p) for p in ((n // 2, n // 2, n // 4), (n // 2, n // 4, n // 2), (n // 4, n // 2, n // 2))}
    assert {tuple(min(i, n - i) for i in idx) for idx, _, _ in O.tie_voxels((n,) * 3, 1.0)} == want


def test_the_cube_of_side_9_ties_at_below_and_above_the_last_edge():
    assert len(O.bins((9, 9, 9), 1.0)[0]) == 6
    assert _census((9, 9, 9), 1.0) == (24, [5], ["at"])
    assert _census((9, 9, 9), 1.7) == (24, [5], ["below"])
    assert _census((9, 9, 9), 5.0) == (24, [5], ["above"])
    # above the last edge: counted in the last bin, multiplied by 0
    qbins, _, qr = O.bins((9, 9, 9), 5.0)
    idx = O.tie_voxels((9, 9, 9), 5.0)[0][0]
    assert O.labels((9, 9, 9), 5.0)[idx] == 5 and O.ratio_on_grid(qbins, np.ones(6), qr)[idx] == 0.0
    qbins, _, qr = O.bins((9, 9, 9), 1.0)
    idx = O.tie_voxels((9, 9, 9), 1.0)[0][0]
    assert O.ratio_on_grid(qbins, np.arange(6.0) + 1, qr)[idx] == 6.0   # ratio[-1] on the edge


def test_images_and_unequal_boxes():
    for apix in (1.0, 0.83, 1.3, 5.0):
        assert _census((8, 8), apix) == (2, [3], ["at"])   # nbins = 4: the last edge
    assert len(O.bins((24, 20), 1.5)[0]) == 16
    ties = O.tie_voxels((24, 20), 1.5)
    assert sorted(idx for idx, _, _ in ties) == [(0, 8), (0, 12)] and {e for _, e, _ in ties} == {9}   # an inner edge
    for n in (10, 12, 24, 32):
        assert O.tie_voxels((n,) * 3, 1.0) == []


# ---------------------------------------------------------------------------------------------------------------------------
# the probes of tests/test_gpu_structure_factor.py notice each wrong rule
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rule", ["left", "fsc_shell", "qstep_width", "closed_last", "exact_ties"])
def test_the_impulse_probe_notices(rule):
    cases = [c for c in SMALL_IMPULSE if c in O.FIXTURE_CASES] if rule == "exact_ties" else SMALL_IMPULSE
    caught = [c for c in cases if not np.array_equal(O.counts(*c, rule=rule), O.counts(*c))]
    assert caught, rule
    if rule == "exact_ties":   # exactly the cases whose ties NumPy does not put on the edge
        assert caught == [((8, 8, 8), 0.83), ((9, 9, 9), 1.7)]


@pytest.mark.parametrize("rule", ["left", "closed_last", "exact_ties", "fsc_shell", "qstep_width"])
def test_the_spike_probe_notices(rule):
    worst = 0.0
    for shape, k, apix, verdict in G.SPIKES:
        k = O.tie_voxels(shape, apix)[0][0] if k is None else k
        data = G._spike_map(shape, k, 77)
        want = O.calculate_structural_factor(data, apix)[1]
        got = O.calculate_structural_factor(data, apix, rule=rule)[1]
        worst = max(worst, np.abs(got / want - 1.0).max())
    assert worst > 1e3 * G.TOL_SF      # the spike on the wrong side of an edge, never a rounding


@pytest.mark.parametrize("rule", ["keep_above", "exact_ties", "left"])
def test_the_spike_probe_s_matched_map_notices(rule):
    worst = 0.0
    for shape, k, apix, verdict in G.SPIKES:
        k = O.tie_voxels(shape, apix)[0][0] if k is None else k
        data, target = G._spike_map(shape, k, 77), G._spike_map(shape, k, 78) * 0.5
        want = O.match_structural_factors(data, apix, target, apix * G.SPIKE_TARGET_FACTOR)
        got = O.match_structural_factors(data, apix, target, apix * G.SPIKE_TARGET_FACTOR, rule=rule)
        worst = max(worst, np.abs(got - want).max() / np.abs(want).max())
    assert worst > 1e3 * G.TOL_MATCH


def test_the_spike_moves_the_power_between_the_last_two_bins_of_the_cube_of_side_8():
    data = G._spike_map((8, 8, 8), (4, 4, 2), 77)
    at, below = O.calculate_structural_factor(data, 1.0)[1], O.calculate_structural_factor(data, 0.83)[1]
    assert at[5] / at.sum() > 0.97 and below[4] / below.sum() > 0.97


def test_the_other_target_case_notices_a_kept_tail():
    """the corners beyond the last edge hold noise power: keeping ratio[-1] there is far outside the bound"""
    shape, apix = (15, 18, 21), 1.7
    data, target = O.make_inputs(shape, 31)[0], O.make_inputs((20, 14, 26), 32)[1]
    want = O.match_structural_factors(data, apix, target, 1.2)
    got = O.match_structural_factors(data, apix, target, 1.2, rule="keep_above")
    assert np.abs(got - want).max() > 1e3 * G.TOL_MATCH * np.abs(want).max()


# ---------------------------------------------------------------------------------------------------------------------------
# the package's host side
# ---------------------------------------------------------------------------------------------------------------------------
def test_the_bins_without_the_grid_are_the_reference_s():
    for shape, apix in O.FIXTURE_CASES + O.IMPULSE_EXTRA + [((33, 47, 20), 0.77), ((300, 512), 3.1), ((7, 64, 5), 12.5)]:
        qbins, freqs = S.structure_factor_bins(shape, apix)
        assert np.array_equal(qbins, O.bins(shape, apix)[0])
        assert all(np.array_equal(f, np.fft.fftfreq(n)) for f, n in zip(freqs, shape))
    assert len(S.structure_factor_bins((512, 512, 512), 1.0)[0]) == 442 and len(S.structure_factor_bins((1024, 1024), 1.0)[0]) == 724


def test_the_full_spectrum_from_the_half():
    rng = np.random.default_rng(3)
    for shape in ((5, 6, 7), (4, 3, 8), (6, 9), (7, 2)):
        a = rng.standard_normal(shape)
        assert np.allclose(S._full_spectrum(np.fft.rfftn(a), shape), np.fft.fftn(a), rtol=0, atol=1e-12)


def test_the_header_exports_the_entry_points():
    header = (ROOT / "include" / "helicon_hip.h").read_text()
    names = set(re.findall(r"\b(hh_sf_\w+)\(", header))
    assert names == {"hh_sf_create", "hh_sf_profile", "hh_sf_match", "hh_sf_kernel_ms", "hh_sf_destroy"}
    assert names <= set(_lib.EXPORTS)
    assert "typedef struct hh_sf hh_sf;" in header


def test_the_chunk_cap_is_the_one_the_gpu_test_crosses():
    text = re.sub(r"\s+", " ", re.sub(r"//[^\n]*", "", (ROOT / "helicon_amd" / "csrc" / "structure_factor.inc").read_text()))
    assert "constexpr int64_t SF_SCRATCH_BYTES = (int64_t)4 << 30;" in text
    assert "const int64_t bytes_per_map = (int64_t)(c->nz ? 8 : 6) * c->per_map * (int64_t)sizeof(float);" in text
    assert "int64_t chunk = std::max<int64_t>(1, SF_SCRATCH_BYTES / bytes_per_map);" in text
    assert "chunk = std::min<int64_t>(chunk, c->nz ? 65535 / c->nz : 65535);" in text
    assert "return std::min<int64_t>(chunk, batch);" in text
    assert "for (int64_t b0 = 0; b0 < batch; b0 += chunk) {" in text
    assert (4 << 30) // (8 * 8 * 2 * 2 * 4) > 65535 // 8 == 8191      # the grid limit, not the scratch, cuts the GPU test's batch
    assert "constexpr int SF_MAX_BINS = 726;" in text and S._MAX_BINS == 726


def test_importing_the_module_does_not_touch_the_gpu():
    code = ("import sys; import helicon_amd.structure_factor as S; from helicon_amd import _lib; "
            "assert _lib._lib is None and 'torch' not in sys.modules and not _lib.hip_runtime_paths(); print('ok')")
    done = subprocess.run([sys.executable, "-c", code], cwd=str(ROOT), capture_output=True, text=True)
    assert done.returncode == 0 and done.stdout.strip() == "ok", done.stderr


def test_argument_errors_come_before_any_device_call(monkeypatch):
    def no_device():
        raise AssertionError("the library was loaded")

    monkeypatch.setattr(_lib, "lib", no_device)
    ok = np.ones((9, 9, 9), np.float32)
    bad_calls = [
        lambda: S.calculate_structural_factor(np.ones(9), 1.0),                          # 1-D
        lambda: S.calculate_structural_factor(np.ones((2, 9, 9, 9)), 1.0),               # 4-D
        lambda: S.calculate_structural_factor(np.ones((2, 2, 2)), 1.0),                  # nbins = 0
        lambda: S.calculate_structural_factor(np.ones((3, 3, 3)), 1.0),
        lambda: S.calculate_structural_factor(np.ones((1, 9, 9)), 1.0),                  # a side below 2
        lambda: S.calculate_structural_factor(np.ones((4, 4, 513)), 1.0),                # a side above 512
        lambda: S.calculate_structural_factor(np.ones((4, 1025)), 1.0),
        lambda: S.calculate_structural_factor(ok, 0.0),                                  # apix
        lambda: S.calculate_structural_factor(ok, float("nan")),
        lambda: S.calculate_structural_factor(ok, 1.0, None, np.ones((9, 9, 8))),        # a mask of another shape
        lambda: S.calculate_structural_factor(ok.astype(complex), 1.0),
        lambda: S.set_structural_factors(ok, 1.0, np.arange(4.0), np.ones(5)),           # bins and profile of two lengths
        lambda: S.set_structural_factors(ok, 1.0, np.arange(4.0), np.ones(4), mask=np.ones((8, 9, 9))),
        lambda: S.match_structural_factors(ok, 1.0, np.ones((8, 8, 8)), 1.0, mask=np.ones((9, 9, 9))),   # the one mask fits both
        lambda: S.StructureFactorMatcher((9, 9, 9), 1.0, np.arange(4.0), None),
    ]
    for call in bad_calls:
        with pytest.raises(ValueError):
            call()
