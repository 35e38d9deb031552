"""Host side of the 3-D map geometry probes (tests/map_geometry_probes.py; the device side is
tests/test_gpu_map_geometry_probes.py).  No device is needed: every probe's reference runs and is finite, the NumPy restatements
the variants are built on ARE oracle/symmetrize.py bit for bit, the probes reach the rules they name (shown from the reference's
own coordinates), no probe's exact items hang on the last bit of a cos / sin or of a matrix entry, the 1 % threshold gives one z
range whichever precision NumPy forms it in, and every wrong-rule variant is bitten by a probe listed for it — an exact item
changes (shape, type, zero pattern, an empty slab's zeros) or a compared number moves by at least 100 times the comparison's
bound — so the device test would notice the same defect in a kernel.  Where arithmetic rules a bite out, that is asserted too."""
import functools

import numpy as np
import pytest
from scipy import ndimage as ndi

import map_geometry_probes as Q
from oracle import symmetrize as S


def _of(kind, *contains):
    return [p for p in Q.PROBES if p.kind == kind and all(c in p.name for c in contains)]


@functools.lru_cache(maxsize=None)
def _ref(name):
    p = Q.BY_NAME[name]
    inp = p.inputs()
    want = Q.reference(p, inp)
    for a in (want if isinstance(want, list) else [want]):
        a.setflags(write=False)
    return inp, want


def _trace(p, **kw):
    inp, _ = _ref(p.name)
    t = {}
    out = Q.helical_numpy(inp["vol"], *Q._helical_args(p.args), trace=t, **kw)
    return out, t


def test_every_reference_runs_and_is_finite_and_the_table_has_the_size_asked_for():
    kinds = {k: len(_of(k)) for k in ("transform_map", "helical", "projections", "symmetrize")}
    print(f"{len(Q.PROBES)} probes: {kinds}")
    assert len(Q.PROBES) >= 300 and kinds["symmetrize"] >= 5 and min(kinds.values()) >= 5
    for p in Q.PROBES:
        assert p.rule.count(":") >= 1 and p.name.startswith(p.kind + "/"), p.name
        inp, want = _ref(p.name)
        vol = inp["vol"]
        assert vol.size <= 6000, p.name
        if p.kind != "transform_map":
            assert 0.0 <= vol.min() and vol.max() <= 1.0, p.name                  # the absolute bounds are made for [0, 1]
        assert (vol.astype(np.float32) == vol).all(), p.name                          # float32 holds every input: the device reads what the reference reads
        for w in (want if isinstance(want, list) else [want]):
            assert np.isfinite(w).all(), p.name
        assert Q.compare(p, want, want, inp).ok, p.name                               # the comparison accepts the reference itself
        if not isinstance(want, list) and want.size == 0:
            assert "/size_side1_" in p.name and 0 in want.shape, p.name                  # a requested side of 1: the empty output
            continue
        one_off = [w.copy() for w in want] if isinstance(want, list) else want.copy()
        (one_off[0] if isinstance(want, list) else one_off).flat[0] += 1e-3 * max(1.0, float(np.abs(vol).max()))
        assert not Q.compare(p, one_off, want, inp).ok, p.name                        # and no pixel is left out


def test_the_oracle_spline_is_scipys_on_small_sides():
    """What makes sides of 1, 2 and 3 fair game: the oracle's cubic interpolation against scipy.ndimage.map_coordinates."""
    for shape in ((1, 5, 7), (2, 3, 4), (3, 3, 3), (5, 7, 11)):
        rng = np.random.default_rng(sum(shape))
        vol = rng.random(shape)
        coords = np.stack([rng.uniform(-0.5, n - 0.5, 400) for n in shape])
        coords[:, :8] = np.array([[0, n - 1] * 4 for n in shape])                    # and exactly on the border
        got, want = S.map_coordinates_cubic(vol, coords), ndi.map_coordinates(vol, coords, order=3)
        print(f"{shape}: max |oracle - scipy| = {np.abs(got - want).max():.2e}")
        np.testing.assert_allclose(got, want, rtol=0, atol=2e-15)
        np.testing.assert_array_equal(got == 0, want == 0)


def test_the_restatements_are_the_oracle():
    for p in _of("transform_map"):
        inp, want = _ref(p.name)
        got = Q.transform_map_numpy(inp["vol"], **p.args)
        assert got.dtype == want.dtype, p.name
        np.testing.assert_array_equal(got, want, err_msg=p.name)
    for p in _of("helical"):
        inp, want = _ref(p.name)
        got = Q.helical_numpy(inp["vol"], *Q._helical_args(p.args))
        assert got.dtype == want.dtype == np.float32, p.name
        np.testing.assert_array_equal(got, want, err_msg=p.name)
    from tests.test_gpu_map_input import np_filter_3d

    x = np.random.default_rng(3).normal(size=(12, 11, 13)).astype(np.float32)
    for lp, hp in ((0.8, 0), (0, 0.2), (0.5, 0.1), (1.5, 0)):
        np.testing.assert_array_equal(Q.np_filter_3d(x, lp, hp), np_filter_3d(x, lp, hp))
    for nz in range(1, 9):
        for apix in (4.75, 4.75 / nz, 2.4, 0.5, 0.2, 10.0):
            b, e = Q.amyloid_slab(nz, apix)
            nzc = int(round(4.75 / apix))
            z0 = nz // 2 - nzc // 2
            v = np.arange(nz * 2.0).reshape(nz, 2)
            np.testing.assert_array_equal(v[b:e].sum(axis=0), v[z0:z0 + nzc].sum(axis=0))


def test_the_transform_probes_reach_what_they_name():
    on_border, borders = 0, set()
    for p in _of("transform_map"):
        tag, shape = p.name.split("/")[1], _ref(p.name)[0]["vol"].shape
        a = p.args
        c = Q.map_coords(shape, **a)
        inside = np.all([(c[d] >= 0) & (c[d] <= shape[d] - 1) for d in range(3)], axis=0)
        if tag[:2] in ("dx", "dy", "dz") and float(a[tag[:2]]).is_integer():
            d = "zyx".index(tag[1])
            assert not Q.inexact_entries(a["rot"], a["tilt"], a["psi"]), p.name      # identity: every entry exact
            hit_low, hit_high = inside & (c[d] == 0), inside & (c[d] == shape[d] - 1)
            assert hit_low.any() or hit_high.any(), p.name                            # exactly on 0 or on n - 1, and inside
            assert (~inside).any(), p.name                                            # and some samples outside
            borders |= {(shape, d, 0)} if hit_low.any() else set()
            borders |= {(shape, d, 1)} if hit_high.any() else set()
            on_border += 1
        if tag == "scale2":
            assert (~inside).mean() > 0.4 and inside.any(), p.name
        if tag.startswith("step"):
            inp, want = _ref(p.name)
            assert want.max() > inp["vol"].max() + 1e-2 or want[want != 0].min() < inp["vol"].min() - 1e-2, p.name   # the overshoot
    assert on_border >= 40
    for shape in Q.TM_SIDES:                                                          # both ends of every axis longer than 1
        assert {(shape, d, e) for d in range(3) for e in (0, 1) if shape[d] > 1} <= borders, shape
    lines = set()
    for p in _of("transform_map", "/seam"):
        shape = _ref(p.name)[0]["vol"].shape
        lines |= {(ax, int(np.prod(shape)) // shape[ax]) for ax in range(3)}
    for ax in range(3):
        assert {(ax, 127), (ax, 128), (ax, 129)} <= lines, lines                      # either side of the prefilter's 128-lane workgroup
    assert {255, 256, 257} <= {int(np.prod(_ref(p.name)[0]["vol"].shape)) for p in _of("transform_map", "/seam")}
    # rot alone and psi alone are one matrix; rot-then-tilt and tilt-then-psi are not
    np.testing.assert_array_equal(Q.euler_matrix(37.0, 0, 0), Q.euler_matrix(0, 0, 37.0))
    assert np.abs(Q.euler_matrix(37.0, 25.0, 0) - Q.euler_matrix(0, 25.0, 37.0)).max() > 0.1
    # three distinct prime sides, all odd
    assert any(_ref(p.name)[0]["vol"].shape == (5, 7, 11) for p in _of("transform_map"))


def test_the_helical_probes_reach_what_they_name():
    parities, odd_sums = set(), set()
    for p in _of("helical"):
        tag = p.name.split("/")[1]
        inp, want = _ref(p.name)
        a = p.args
        _, t = _trace(p)
        nz0 = inp["vol"].shape[0]
        if tag.startswith("parity_c1"):
            parities.add(tuple(n % 2 for n in inp["vol"].shape))
        if tag.startswith(("rise2", "profile_zero_ends_rise2", "fraction0.5", "fraction0.625")) and not tag.endswith("_general"):
            assert (t["k2"] == np.round(t["k2"])).all(), p.name                       # every k2 an integer: kf == kc
            assert (t["k2"] == t["z1"]).any() and (t["k2"] == t["z0"]).any(), p.name  # both comparisons met exactly
        if tag.startswith("size_"):
            ns = a["new_size"]
            work = t["work_shape"]
            py_slice = np.zeros(work)[tuple(slice(n // 2 - n1 // 2, n // 2 + n1 // 2) for n, n1 in zip(work, ns))].shape
            assert want.shape == (py_slice if tuple(ns) != work else work), p.name   # (no crop when the work volume is the request)
            assert work == tuple(max(n, m) for n, m in zip(inp["vol"].shape, ns)), p.name
        if tag.startswith("hmax1_"):
            assert int(t["work_shape"][0] * a["new_apix"] / a["rise"]) == 0 and t["hmax"] == 1, p.name
        if tag.startswith("hmax8_"):
            assert 7 <= t["hmax"] <= 10, (p.name, t["hmax"])
        if tag.startswith("profile_zero_") and sum(Q.z_range(inp["vol"], 1.0)[:2]) % 2 == 1:
            odd_sums.add(inp["vol"].shape)                                            # z0 + z1 odd: zmid takes the remainder
        if tag.startswith("profile_zero_ends"):
            assert Q.z_range(inp["vol"], 1.0)[:2] == (2, nz0 - 4), p.name
        if tag.startswith("profile_single") or tag.startswith("fraction0.05"):
            assert t["z0"] == t["z1"] and not want.any(), p.name                      # an empty range: all-zero output
        elif not tag.startswith(("size_tiny", "size_side1")):
            assert (want != 0).mean() > 0.2, p.name
        if tag.startswith("profile_one_percent"):
            prof = inp["vol"].sum(axis=(1, 2))
            assert prof.max() == 100.0 and prof[1] == 1.0 and prof[0] == 0.0 and t["z0"] >= 2, p.name
    assert len(parities) == 8 and odd_sums == {(12, 11, 13), (13, 10, 12)}
    p = Q.BY_NAME["helical/size_mixed_a_r1.0/12x11x13"]
    assert p.args["new_size"] == (14, 9, 13) and _ref(p.name)[1].shape == (14, 8, 12)  # the odd-crop rule
    # fraction values whose nz0 * fraction + 0.5 crosses an integer change the half width
    for nz0 in (12, 13):
        assert any(int(nz0 * f + 0.5) // 2 != int(nz0 * f) // 2 for f in (0.625, 0.58, 0.3))


def test_the_projection_probes_reach_what_they_name():
    slabs = {}
    for p in _of("projections"):
        inp, want = _ref(p.name)
        nz, ny, nx = inp["vol"].shape
        assert [w.shape for w in want] == [(nz, ny), (nz, nx), (ny, nx)], p.name
        assert all(w.dtype == (np.float32 if inp["vol"].dtype == np.float32 else np.float64) for w in want), p.name
        slabs[p.name] = Q.probe_slab(p, nz)
    assert {(ny, nx) for ny in (1, 3, 4, 5) for nx in (1, 63, 64, 65, 255, 256, 257)} <= {_ref(p.name)[0]["vol"].shape[1:] for p in _of("projections", "/thin/")}
    assert slabs["projections/amyloid_one/6x5x9/f32"] == (3, 4) and slabs["projections/amyloid_nz/6x5x9/f32"] == (0, 6)
    assert slabs["projections/amyloid_nz/7x5x9/f32"] == (0, 7)
    assert slabs["projections/amyloid_beyond/6x5x9/f32"] == (4, 6)                    # z0 = -2: counted from the end
    assert slabs["projections/amyloid_beyond/7x5x9/f32"] == (5, 7)
    assert slabs["projections/amyloid_none/6x5x9/f32"][0] == slabs["projections/amyloid_none/6x5x9/f32"][1]
    empty = [n for n, (b, e) in slabs.items() if b == e]
    assert len(empty) >= 6 and all(not _ref(n)[1][2].any() and _ref(n)[1][0].any() for n in empty)


def test_no_exact_item_hangs_on_the_last_bit_of_the_host_trigonometry():
    """transform_map: each matrix entry a non-zero angle enters, one ulp either way, one at a time: the zero pattern stays and
    the values move by at most a quarter of the bound.  helical: every cos and sin of a non-zero angle one ulp either way
    (coordinates are linear in both, so the four corners bound every mixture): the contribution counts of the compared
    region stay and the values move by at most a quarter of the bound."""
    worst = {"transform_map": 0.0, "helical": 0.0}
    for p in _of("transform_map"):
        inp, want = _ref(p.name)
        a = p.args
        entries = Q.inexact_entries(a["rot"], a["tilt"], a["psi"])
        assert bool(entries) == bool(a["rot"] or a["tilt"] or a["psi"]), p.name
        coef = Q.spline_coefficients(inp["vol"])
        bound = Q.BOUND_TRANSFORM * float(np.abs(want).max())
        for e in entries:
            for sign in (1, -1):
                got = Q.transform_map_numpy(inp["vol"], **a, nudge=(e, sign), coefficients=coef)
                np.testing.assert_array_equal(got == 0, want == 0, err_msg=f"{p.name} entry {e} {sign:+d}")
                moved = float(np.abs(got.astype(np.float64) - want).max())
                worst["transform_map"] = max(worst["transform_map"], moved / bound)
                assert moved <= bound / 4, (p.name, e, sign, moved, bound)
    for p in _of("helical"):
        inp, want = _ref(p.name)
        _, t0 = _trace(p)
        for nudge in ((1, 1), (1, -1), (-1, 1), (-1, -1)):
            got, t = _trace(p, nudge=nudge)
            np.testing.assert_array_equal(t["w"][t["crop"]], t0["w"][t0["crop"]], err_msg=f"{p.name} {nudge}")
            moved = float(np.abs(got.astype(np.float64) - want).max()) if got.size else 0.0
            worst["helical"] = max(worst["helical"], moved / Q.BOUND_HELICAL)
            assert moved <= Q.BOUND_HELICAL / 4, (p.name, nudge, moved)
    print("largest move under a one-ulp nudge, in units of the bound:", worst)


def test_the_one_percent_threshold_gives_one_z_range_in_float32_and_float64():
    """NumPy 2 forms 0.01 * float32 in float32, NumPy 1 in float64, the device in float64 on float64 slice sums: no probe
    places a slice sum between the thresholds, and the z range is the same under both (and under float64 slice sums)."""
    for p in _of("helical") + _of("symmetrize"):
        inp, _ = _ref(p.name)
        vol, fr = inp["vol"], p.args["fraction"]
        r32, r64 = Q.z_range(vol, fr, threshold_dtype=np.float32), Q.z_range(vol, fr, threshold_dtype=np.float64)
        assert r32[:2] == r64[:2] == Q.z_range(vol, fr)[:2], p.name
        lo, hi = sorted((r32[2], r64[2]))
        prof32, prof64 = vol.sum(axis=(1, 2)), vol.astype(np.float64).sum(axis=(1, 2))
        for prof in (prof32.astype(np.float64), prof64):
            assert not ((prof > lo) & (prof <= hi)).any(), p.name
            hit = np.flatnonzero(prof > 0.01 * prof64.max())
            assert (hit[0], hit[-1]) == tuple(np.flatnonzero(prof32 > r32[2])[[0, -1]]), p.name


@pytest.mark.parametrize("name", list(Q.VARIANTS))
def test_every_variant_is_bitten_by_a_probe_listed_for_it(name):
    v = Q.VARIANTS[name]
    assert v.probes, name
    bitten = []
    for pname in v.probes:
        p = Q.BY_NAME[pname]
        inp, want = _ref(pname)
        verdict = Q.compare(p, v.run(p, inp), want, inp)
        if verdict.bitten():
            assert not verdict.ok
            bitten.append((pname, verdict.mismatches, verdict.figure, verdict.bound))
    print(f"{name}: bitten by {len(bitten)} of {len(v.probes)} listed probes, e.g. " +
          "; ".join(f"{n} (exact items {m}, moved {f:.3g} against {b:.3g})" for n, m, f, b in bitten[:3]))
    assert bitten, name


def test_what_no_probe_can_bite_by_arithmetic():
    """w3 formed directly: the four weights sum to 1 to rounding either way, so the values move by a few ulps of float64.
    floor + 1 for ceil: at a non-integer coordinate they are the same corner; at an integer one the other corner carries
    weight 0 exactly and 0 * finite = 0, and it is in range (k2 < z1 <= nz0 - 1, jf < ny0 - 1, if < nx0 - 1): the variant IS
    the reference bit for bit on finite data.  A float64 running sum in place of the float32 one: each of cnt roundings costs
    at most 2^-24 of a sum of at most cnt, so cnt 2^-24 after the division — below 100 bounds (1e-4) for any cnt < 1677; a
    float32 running sum of n <= 257 inputs in [0, 1] likewise moves a projection by at most n 2^-24 of it, below 100 bounds.
    A prefilter skipped on an axis of side 1 is no change (len < 2 returns), nor is axis 2's stride on axis 1 where nx = 1."""
    for name, v in Q.UNBITABLE.items():
        worst = 0.0
        for pname in v.probes:
            p = Q.BY_NAME[pname]
            inp, want = _ref(pname)
            got = v.run(p, inp)
            verdict = Q.compare(p, got, want, inp)
            assert not verdict.bitten(), (name, pname, verdict)
            worst = max(worst, verdict.figure / verdict.bound if verdict.bound else 0.0)
            if name == "helical: floor + 1 for ceil":
                np.testing.assert_array_equal(got, want, err_msg=pname)
            if name == "transform_map: w3 formed directly":
                assert verdict.ok and verdict.figure <= 1e-12 * max(1.0, float(np.abs(want).max())), (pname, verdict)
        print(f"{name}: largest move {worst:.3g} bounds over {len(v.probes)} probes")
    for p in _of("transform_map"):
        inp, want = _ref(p.name)
        shape = inp["vol"].shape
        for ax in range(3):
            if shape[ax] == 1:
                np.testing.assert_array_equal(Q.VARIANTS[f"transform_map: prefilter skipped on axis {ax}"].run(p, inp), want, err_msg=p.name)
        if shape[2] == 1:
            np.testing.assert_array_equal(Q.VARIANTS["transform_map: axis-1 lines walked with axis-2's stride"].run(p, inp), want, err_msg=p.name)
    cnt = max(int(_trace(p)[1]["w"].max()) for p in _of("helical"))
    print(f"largest contribution count of a helical probe: {cnt}")
    assert cnt < 1677
