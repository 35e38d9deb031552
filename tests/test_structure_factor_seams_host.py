"""Host side of tests/test_gpu_structure_factor_seams.py: the facts of the probe table hold (from the package's own bins and the
constants the kernels compile in, read from the sources), every probe input meets the floor and leaves no bin empty, the
unit-impulse probe of tests/test_gpu_structure_factor.py is blind to the launch-geometry defects while each new probe moves by
at least 100 times its bound, the absmax probe's sums overflow when the strided tail is missed, and the exact scaling probes
stay inside float32's normal range.  Nothing here needs a GPU."""
import math
import re
from pathlib import Path

import numpy as np
import pytest

import structure_factor_oracle as O
import structure_factor_seams as Q
from helicon_amd import structure_factor as S

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "helicon_amd" / "csrc"
IMPULSE_SHAPE, IMPULSE_APIX = (66, 70, 130), 1.2


def _source(name):
    return re.sub(r"\s+", " ", re.sub(r"//[^\n]*", "", (CSRC / name).read_text()))


# ---------------------------------------------------------------------------------------------------------------------------
# the table
# ---------------------------------------------------------------------------------------------------------------------------
def test_the_constants_are_the_ones_the_kernels_compile_in():
    fc, tile, sf = _source("fourier_correlation.inc"), _source("mfma_tile.inc"), _source("structure_factor.inc")
    assert f"constexpr int FC_T = {Q.FC_T};" in fc and f"constexpr int FC_K = {Q.FC_K};" in fc
    assert f"constexpr int TILE_THREADS = {Q.THREADS};" in tile
    assert f"constexpr int SF_MAX_BINS = {Q.SF_MAX_BINS};" in sf and S._MAX_BINS == Q.SF_MAX_BINS
    # the capped grids and their strides
    assert f"hipLaunchKernelGGL(k_sf_prepare, dim3((unsigned)std::min<int64_t>((per_map + 255) / 256, {Q.GRID_CAP}), (unsigned)nb), dim3(256)" in sf
    assert f"hipLaunchKernelGGL(k_sf_scale, dim3((unsigned)std::min<int64_t>((per_spec + 255) / 256, {Q.GRID_CAP}), (unsigned)nb), dim3(256)" in sf
    assert f"hipLaunchKernelGGL(k_fc_absmax, dim3((unsigned)std::min<int64_t>((per_map + 255) / 256, {Q.ABSMAX_GRID_CAP}), (unsigned)nb), dim3(256)" in sf
    assert sf.count("i += (int64_t)gridDim.x * 256") == 2 and fc.count("i += (int64_t)gridDim.x * 256") == 1
    # the loops over the bin table, one turn per 256 threads
    assert sf.count("for (int e = t.tid; e < g.nbins; e += 256)") == 1 and sf.count("for (int e = threadIdx.x; e < g.nbins; e += 256)") == 1
    assert "for (int e = tid; e < n; e += TILE_THREADS)" in fc
    # the tiles and slices of the x pass and of the c2r pass
    assert "for (int k0 = 0; k0 < nx; k0 += FC_K)" in sf and "for (int k0 = 0; k0 < g.ncol; k0 += FC_K)" in _source("true_fsc.inc")
    assert "dim3((unsigned)((c->rows + FC_T - 1) / FC_T), (unsigned)((c->ncol + FC_T - 1) / FC_T), (unsigned)nb)" in sf
    assert "dim3((unsigned)((c->rows + FC_T - 1) / FC_T), (unsigned)((c->nx + FC_T - 1) / FC_T), (unsigned)nb)" in sf
    assert Q.PREPARE_REACH == 1048576 and Q.ABSMAX_REACH == 65536


@pytest.mark.parametrize("name", [p.name for p in Q.PROBES])
def test_the_facts_of_the_table_hold(name):
    p = Q.BY_NAME[name]
    qbins, _ = S.structure_factor_bins(p.shape, p.apix)
    g = Q.geometry(p.shape, len(qbins))
    assert p.facts, name
    for fact, value in p.facts:
        assert g[fact] == value, (name, fact, g[fact], value)
    assert g["nbins"] <= Q.SF_MAX_BINS
    assert set(p.variants) <= set(Q.ALL) and len(p.variants) >= 1
    for v in Q.ALL:     # every variant runs, or the table says why not
        assert (v in p.variants) != bool(Q.VARIANTS_LEFT_OUT.get((p.name, v))), (name, v)


def test_the_table_crosses_every_seam_the_existing_cases_do_not():
    def geo(shape, apix):
        return Q.geometry(shape, len(S.structure_factor_bins(shape, apix)[0]))

    old = [geo(s, a) for s, a in O.FIXTURE_CASES] + [geo((15, 18, 21), 1.7), geo((12, 20, 36), 1.1)]
    assert max(g["x_col_tiles"] for g in old) == 1 and max(g["x_slices"] for g in old) == 2 and max(g["waves_active"] for g in old) < 4
    assert max(g["c2r_out_tiles"] for g in old) == 1 and max(g["c2r_slices"] for g in old) == 1
    assert max(g["y_tiles"] for g in old) == 1 and max(g["z_tiles"] for g in old) == 1 and max(g["bin_turns"] for g in old) == 1
    assert not any(g["prepare_tail"] or g["scale_tail"] or g["absmax_tail"] for g in old)
    new = {p.name: geo(p.shape, p.apix) for p in Q.PROBES}
    for key, least in (("x_col_tiles", 2), ("x_slices", 5), ("waves_active", 4), ("c2r_out_tiles", 3), ("c2r_slices", 3), ("y_tiles", 2),
                       ("z_tiles", 2), ("bin_turns", 3), ("prepare_tail", 1), ("scale_tail", 1), ("absmax_tail", 1)):
        assert max(g[key] for g in new.values()) >= least, key
    # the legal maxima, and the largest image exactly at the cap: its last workgroup is the 4096th and there is no tail
    assert new["512x4x6"]["nbins"] == new["4x512x6"]["nbins"] == new["4x6x512"]["nbins"] == 442
    assert new["1024x6"]["nbins"] == new["6x1024"]["nbins"] == new["1024x1024"]["nbins"] == 724
    assert new["1024x1024"]["per_map"] == Q.PREPARE_REACH and new["1024x1024"]["prepare_tail"] == 0
    # every variant on the first three rows; the prepare tail runs with mask and threshold
    left_out = {(p.name, v) for p in Q.PROBES for v in Q.ALL if v not in p.variants}
    assert left_out == set(Q.VARIANTS_LEFT_OUT) == {("104x100x202", "thresh"), ("40x41x42-spike8192", "both")}


@pytest.mark.parametrize("name", [p.name for p in Q.PROBES])
def test_no_bin_is_empty(name):
    p = Q.BY_NAME[name]
    for apix in (p.apix, p.apix_target):
        c = O.counts(p.shape, apix)
        assert c.min() >= 1 and int(c.sum()) == int(np.prod(p.shape))


@pytest.mark.parametrize("name,variant", Q.CASES)
def test_every_profile_that_is_compared_meets_the_floor(name, variant):
    p = Q.BY_NAME[name]
    data, target = Q.floors(p, variant)
    y = Q.profiles(p, variant)
    assert (y["sf"] > 0).all() and (y["tsf"] > 0).all()
    assert data >= Q.FLOOR and target >= Q.FLOOR, (name, variant, data, target)


def test_the_inputs_are_float32_that_float16_holds_and_the_thresholds_leave_spikes():
    p = Q.BY_NAME["5x6x130"]
    inp = Q.inputs(p)
    for key in ("data", "target", "mask"):
        assert inp[key].dtype == np.float32 and np.array_equal(inp[key].astype(np.float16).astype(np.float32), inp[key])
    for key, t in (("data", inp["thresh"]), ("target", inp["thresh_target"])):
        assert float(np.float16(t)) == t
        left = O.threshold_data(inp[key].astype(np.float64), t)
        assert 0.005 < (left > 0).mean() < 0.06 and left.std() > 3 * left.mean()


# ---------------------------------------------------------------------------------------------------------------------------
# the defects
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,variant", [("5x6x130", "plain"), ("5x6x130", "both"), ("67x129", "mask"), ("20x380", "thresh")])
def test_the_model_without_a_defect_is_the_yardstick(name, variant):
    p = Q.BY_NAME[name]
    e = Q.figures(Q.yardstick(p, variant), *Q.model(p, variant))
    assert max(e) <= 1e-12, e


# (defect, arg, probe, variant, the figure that must move: 0 spectrum, 1 per bin, 2 matched map, whether the impulse probe is blind)
NOTICED = [
    ("slice_lost", 1, "5x6x130", "plain", 0, True),
    ("slice_lost", 2, "5x6x130", "plain", 0, True),
    ("slice_lost", 3, "5x6x130", "plain", 0, True),
    ("slice_lost", 4, "5x6x130", "plain", 0, True),      # the last slice, of 2 columns
    ("slice_lost", 2, "6x5x66", "plain", 0, True),
    ("column_tile_lost", None, "5x6x130", "plain", 0, False),
    ("column_tile_misread", None, "5x6x130", "plain", 0, True),
    ("column_tile_misread", None, "67x129", "plain", 0, True),
    ("rows_swapped", None, "67x129", "plain", 0, True),
    ("rows_swapped", None, "66x70x130", "plain", 0, True),
    ("bins_beyond_256_lost", None, "20x380", "plain", 1, True),
    ("prepare_tail_raw", None, "104x100x202", "both", 0, True),
    ("prepare_tail_raw", None, "104x100x202", "both", 1, True),
    ("scale_tail_lost", None, "104x100x202", "plain", 2, True),
    ("absmax_tail_lost", None, "40x41x42-spike8192", "plain", 1, True),
]


@pytest.fixture(scope="module")
def impulse_counts():
    return O.counts(IMPULSE_SHAPE, IMPULSE_APIX)


@pytest.mark.parametrize("defect,arg,name,variant,which,blind", NOTICED)
def test_the_impulse_is_blind_and_the_probe_is_not(defect, arg, name, variant, which, blind, impulse_counts):
    p = Q.BY_NAME[name]
    y = Q.yardstick(p, variant)
    F, sf, out = Q.model(p, variant, defect, arg)
    if which == 0:
        moved = Q.spectrum_error(F, y["F"])
    elif which == 1:
        moved = float(np.abs(sf / y["sf"] - 1.0).max())
    else:
        moved = Q.map_error(np.nan_to_num(out, nan=np.inf), y["want"])
    assert moved >= 100 * Q.bounds(p)[which], (defect, arg, name, moved, Q.bounds(p))
    seen = not np.array_equal(np.round(Q.impulse_profile(IMPULSE_SHAPE, IMPULSE_APIX, defect, arg)).astype(np.int64), impulse_counts)
    assert seen != blind, (defect, arg)


def test_a_missed_absmax_tail_overflows_the_sums_only_when_the_tail_voxel_dominates():
    """With the maximum of the first 65,536 voxels in place of the map's, the scale is spike^2 too large.  The Parseval bound
    2 (voxels max|x|)^2 has voxels / 2 of slack against a map of one dominant voxel (sum |F|^2 = voxels x^2), so the sums
    overflow once spike^2 > 2 voxels or so: at 8192 they exceed 2^63 and wrap, at 8 they do not and the profile is unchanged
    (finer, still exact) — the scale then depends on the tail without any result showing it."""
    for name, overflows in (("40x41x42-spike8192", True), ("40x41x42-spike8", False)):
        p = Q.BY_NAME[name]
        inp, y = Q.inputs(p), Q.profiles(p, "plain")
        flat = inp["data"].reshape(-1)
        at = int(np.abs(flat).argmax())
        head = float(np.abs(flat[:Q.ABSMAX_REACH]).max())
        assert at >= Q.ABSMAX_REACH and abs(float(flat[at])) == p.spike * head
        ncol = p.shape[-1] // 2 + 1
        power, lab = Q.half_power(y["F"], p.shape), O.labels(p.shape, p.apix)[..., :ncol]
        nbins = len(y["qbins"])
        # the whole map's maximum: every sum stays below 2^62 and gives the yardstick's profile
        scale, exact, wrapped, sf = Q.fixed_point_sums(power, lab, nbins, abs(float(flat[at])), flat.size)
        assert max(exact) < 2**62 and exact == wrapped and sum(exact) < 2**62
        assert np.abs(sf / y["sf"] - 1.0).max() < 1e-7             # the rounding to integers, far inside the bound
        # the head's maximum
        scale_head, exact, wrapped, sf = Q.fixed_point_sums(power, lab, nbins, head, flat.size)
        assert scale_head == scale * p.spike**2
        if overflows:
            assert max(exact) > 2**63 and exact != wrapped
            assert np.abs(sf / y["sf"] - 1.0).max() >= 100 * Q.bounds(p)[1]
        else:
            assert max(exact) < 2**63 and exact == wrapped and np.abs(sf / y["sf"] - 1.0).max() < 1e-7


def test_another_map_s_scale_is_noticed_by_the_batch_probe_and_not_by_a_batch_of_impulses():
    b = Q.batch_inputs()
    maps = b["maps"]
    sums = [O.calculate_structural_factor(m, Q.BATCH_APIX)[1] for m in maps]
    assert all(O.floor_ratio(Q.BATCH_SHAPE, Q.BATCH_APIX, s) >= Q.FLOOR for s in sums)
    amax = [np.abs(m).max() for m in maps]
    wrong = Q.wrong_map_scale(sums, amax, maps[0].size)
    tol = Q.bounds(Q.BY_NAME["5x6x130"])[1]
    for j in range(len(maps)):
        assert np.abs(wrong[j] / sums[j] - 1.0).max() >= 100 * tol       # stack != singles, by powers of two
    # every map of a batch of impulses has the maximum 1: one scale
    counts = O.counts(IMPULSE_SHAPE, IMPULSE_APIX).astype(np.float64)
    same = Q.wrong_map_scale([counts] * 3, [1.0] * 3, int(np.prod(IMPULSE_SHAPE)))
    assert np.array_equal(same, np.stack([counts] * 3))
    # neighbours in the batch are at least 2^7 apart in magnitude
    assert min(abs(a - c) for a, c in zip(Q.BATCH_EXPONENTS, Q.BATCH_EXPONENTS[1:] + Q.BATCH_EXPONENTS[:1])) >= 7
    assert Q.BATCH_EXPONENTS == (0, 40, -40, 13, -7)


def _target_on(qbins, tbins, tsf):
    from scipy import interpolate

    return interpolate.interp1d(tbins, tsf, bounds_error=False, fill_value=0)(qbins)


def test_the_batch_and_scaling_inputs_stay_in_float32_s_normal_range():
    """The values, the planes after every forward pass, the scaled spectrum and the planes after the inverse passes: no
    non-zero real or imaginary part leaves float32's normal range at any exponent of the probes."""
    b = Q.batch_inputs()
    qbins = O.bins(Q.BATCH_SHAPE, Q.BATCH_APIX)[0]
    target = _target_on(qbins, b["tbins"], b["tsf"])
    mask = b["mask"].astype(np.float64)
    for base, k, m in zip(b["bases"], Q.BATCH_EXPONENTS, b["maps"]):
        base = base.astype(np.float64)
        assert m.dtype == np.float32 and np.array_equal(m.astype(np.float64), np.ldexp(base, k))
        # plain, and thresholded and masked with the map's own threshold: 2^k (clip(x, t) - t) mask
        for v in (base, O.threshold_data(base, b["thresh"]) * mask):
            forward, scaled = Q.device_stages(v, qbins, target, Q.BATCH_APIX)
            assert Q.stays_normal(v, k) and all(Q.stays_normal(f, k) for f in forward) and all(Q.stays_normal(f, 0) for f in scaled)
        # under another map's threshold 2^c t the prepared map is what it is, not a multiple: its own values are checked
        for c in Q.BATCH_EXPONENTS:
            v = O.threshold_data(m.astype(np.float64), float(np.ldexp(b["thresh"], c))) * mask
            assert Q.stays_normal(v, 0) and all(Q.stays_normal(f, 0) for f in Q.device_stages(v, qbins, target, Q.BATCH_APIX)[0])
    for shape, apix in Q.SCALING_SHAPES:
        s = Q.scaling_inputs(shape, apix)
        qbins = O.bins(shape, apix)[0]
        target = _target_on(qbins, s["tbins"], s["tsf"])
        data = s["data"].astype(np.float64)
        masked = (data * s["mask"]).astype(np.float32).astype(np.float64)
        for v in (data, masked):
            forward, scaled = Q.device_stages(v, qbins, target, apix)
            assert all(Q.stays_normal(f, 0) for f in scaled)
            for k in Q.SCALING_EXPONENTS:
                assert Q.stays_normal(v, k) and all(Q.stays_normal(f, k) for f in forward)
                # the power |F|^2 and the profile 4^k sf are float64: far inside its range
                power = np.abs(forward[-1]) ** 2
                assert 1e-200 < math.ldexp(float(power.min()), 2 * k) and math.ldexp(float(power.sum()), 2 * k) < 1e200
        for k in Q.SCALING_EXPONENTS:
            assert np.array_equal(np.ldexp(s["data"], k).astype(np.float32).astype(np.float64), np.ldexp(data, k))
    assert set(Q.SCALING_EXPONENTS) == {20, -20, 40, -40} and Q.SCALING_ROUTES == ("profile", "match", "match_mask")


def test_the_two_cells_left_out_cannot_be_compared():
    p = Q.BY_NAME["104x100x202"]
    assert min(Q.floors(p, "thresh")) < Q.FLOOR
    p = Q.BY_NAME["40x41x42-spike8192"]
    inp = Q.inputs(p)
    flat, mask = inp["data"].reshape(-1), inp["mask"].reshape(-1)
    assert not mask[Q.ABSMAX_REACH:].any()                                              # the mask is 0 on the whole strided tail
    assert not (O.threshold_data(flat.astype(np.float64), inp["thresh"]) * mask).any()   # and the threshold removes the rest


def test_the_bounds_are_four_times_the_measured_figures_and_never_below_the_existing_ones():
    import json

    import test_gpu_structure_factor as G

    assert Q.TOL_SF == G.TOL_SF and Q.TOL_MATCH == G.TOL_MATCH and Q.FLOOR == G.FLOOR and Q.MARGIN == 4.0
    assert Q.bound_from(1e-7, 2e-6) == 2e-6 and Q.bound_from(1.99e-6, 2e-6) == 2e-6        # within the existing constant: that constant
    assert math.isclose(Q.bound_from(2.6e-6, 2e-6), 2e-5) and math.isclose(Q.bound_from(2.053e-6, 2e-6), 9e-6)
    assert math.isclose(Q.bound_from(2.5e-6, 2e-6), 1e-5) and math.isclose(Q.bound_from(6.733e-6, 2e-6), 3e-5)
    assert math.isclose(Q.bound_from(Q.MEASURED_BATCH_SF, Q.TOL_SF), 2e-5)
    seams = json.loads((ROOT / "profiles" / "structure_factor.json").read_text())["accuracy"]["seams"]
    assert seams["batch_5x6x130"]["sf_rel"] == Q.MEASURED_BATCH_SF
    assert set(Q.MEASURED) == {p.shape for p in Q.PROBES}
    for shape, m in Q.MEASURED.items():
        rec = seams["shapes"]["x".join(map(str, shape))]
        assert (rec["spectrum_rel"], rec["sf_rel"], rec["match_rel"]) == tuple(m)
        p = next(q for q in Q.PROBES if q.shape == shape)
        assert np.allclose(rec["bounds"], Q.bounds(p), rtol=1e-12, atol=0)
        assert all(b >= fig for b, fig in zip(Q.bounds(p), m))
