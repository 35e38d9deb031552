"""Host side of the alignment probes (tests/align_probes.py; the device side is tests/test_gpu_align_probes.py).  No device is
needed: the float32 restatements are what they claim (np.roll on integer shifts, oracle.prep.warp_affine for the first warp,
the float64 yardstick to float32's rounding), the probes reach every rule they name on a counted number of pixels, every
wrong-rule variant changes an exactly compared item of a probe listed for it (or is shown to be beyond any finite plane), and
every candidate is fit for the score comparison: kappa <= 1e4 and a finite reference, or deliberately degenerate and listed."""
import numpy as np
import pytest

from oracle import prep as P
import align_cases as Y
import align_probes as Q

NAMES = [p.name for p in Q.PROBES]


def test_the_table_holds_what_the_probes_are_named_for():
    by = lambda prefix: [p for p in Q.PROBES if p.name.startswith(prefix)]
    assert {p.shape for p in by("second_x_block/")} == {(6, 257), (5, 258), (8, 256), (3, 300)}
    assert {p.shape for p in by("tall/")} == {(257, 6), (300, 3)}
    assert {p.shape for p in by("smallest_sides/")} == {(2, 2), (2, 3), (3, 2), (5, 7), (7, 4)}
    assert {p.shape for p in by("largest_sides/")} == {(2, 1024), (1024, 2)}
    assert {p.shape for p in by("far_and_odd/")} == {(9, 14), (16, 24)} and {p.shape for p in by("seam/")} == {(16, 24), (5, 7)}
    for p in Q.PROBES:
        cands = Q.candidates(p.name)
        ref, mov, tap = Q.planes(p.name)
        assert ref.shape == p.shape and mov.shape == tap.shape == (p.n_planes, *p.shape)
        assert all(v.dtype == np.float32 and np.isfinite(v).all() for v in (ref, mov, tap, Q.caller_plane(p.name)))
        assert all(0 <= c.plane < p.n_planes and np.isfinite(c.inv).all() and len(c.inv) == 6 for c in cands)
        tags = {c.tag for c in cands}
        if p.name.startswith("largest_sides/"):
            assert len(cands) == 3
        else:
            assert {"identity", "quarter turn", "half turn", "half pixel", "quarter pixel", "hair", "3.5 sides", "-40 sides", "shear", "reflection",
                    "scale 0.5, angle 0.0", "scale 2.0, angle 0.0", "scale 1.03, angle 37.3", "scale 0.97, angle -121.9"} <= tags
        if p.name.startswith("smallest_sides/"):
            assert len(cands) >= 40
            # 32 rows of a wavefront of k_align_c2r over sides 2 ... 7: it spans 5 ... 16 candidates
            assert 5 <= -(-32 // p.shape[0]) <= 16 and p.shape[1] // 2 + 1 in (2, 3, 4)
        if p.name.startswith("seam/"):
            assert len(cands) >= 2 * Q.CHUNK + 1 and len({c.plane for c in cands[:2 * Q.CHUNK + 1]}) >= 3
            planes = [c.plane for c in cands]
            assert planes[Q.CHUNK - 1] != planes[Q.CHUNK] or planes[2 * Q.CHUNK - 1] != planes[2 * Q.CHUNK]     # the index changes at a seam
        # a (scale, angle) candidate's matrix is what evaluate() would send; the identity's is exact
        for c in cands:
            if c.tag == "identity":
                assert np.array_equal(np.asarray(c.inv), np.asarray(Q.IDENTITY6))
    mov, tap = Q.planes("range_rules/12x20")[1], Q.planes("taper_rules/12x20")[2]
    assert 5 <= mov[0].min() and mov[0].max() <= 9 and -9 <= mov[1].min() and mov[1].max() <= -5 and mov[2].min() < 0 < mov[2].max()
    assert (mov[3] == 3).all() and not mov[4].any()
    assert tap[0].min() > 0 and tap[1].max() == 0 and tap[2].min() < 0 < tap[2].max() and tap[3].min() >= 2 and 0 == tap[4].min() < tap[4].max() == 1
    for stack in (mov[:4], tap):          # no two rows of the range table agree: a wrong row is another clip
        ranges = [Q.plane_range(v) for v in stack]
        assert len(set(ranges)) == len(ranges), ranges


def test_the_restatements_are_what_they_restate():
    """(1) integer shifts are np.roll bit for bit; (2) the first warp with its rules exposed is oracle.prep.warp_affine bit for
    bit on every candidate; (3) the float32 wrap warp against the float64 yardstick.  Bilinear interpolation of a periodic
    image is continuous with slope at most (max - min) per pixel along each axis and the clip does not stretch, so the two differ
    by at most (max - min)(|dc| + |dr|), dc / dr the difference of the float32 and float64 coordinates, plus the rounding of the
    mixes themselves: three float32 operations in the horizontal mix and the final cast, 4 ulp of the largest magnitude.  Where
    the float32 coordinates are exact (dyadic matrices) that is 4 ulp alone, no pixel left out."""
    for name in ("far_and_odd/9x14", "smallest_sides/2x3", "second_x_block/6x257", "range_rules/12x20"):
        ref, mov, tap = Q.planes(name)
        ny, nx = ref.shape
        for shift in ((0, 0), (1, 0), (0, -1), (-3, 5), (ny // 2 + 1, -(nx // 2) - 1), (ny + 2, -nx - 3), (-41 * ny, 40 * nx + 1)):
            for v in (mov[0], tap[-1], Q.caller_plane(name)):
                np.testing.assert_array_equal(Q.warp_wrap_f32(v, Q.IDENTITY6, shift), np.roll(v, shift, axis=(0, 1)), err_msg=f"{name} {shift}")
    worst, exact = 0.0, 0
    for name in NAMES:
        ref, mov, tap = Q.planes(name)
        for cand, idx in zip(Q.candidates(name), Q.host_indices(name)):
            img = mov[cand.plane]
            np.testing.assert_array_equal(Q.warp_constant_f32(img, cand.inv), P.warp_affine(img, Q.full3(cand.inv)), err_msg=f"{name} {cand.tag}")
            shift = Q.midpoint_shift(idx, ref.shape)
            assert shift == Y.shift_of(Y.cross_power(ref, Q.first_warp(name, cand))[1])
            h = Q.shifted6(cand.inv, shift)
            np.testing.assert_array_equal(h, Y.shifted(Q.full3(cand.inv), shift)[:2].ravel())
            c32, r32 = Q.coordinates(ref.shape, h)
            r64, c64 = Y._coords(ref.shape, Q.full3(h))
            slack = float(np.abs(c32 - c64).max() + np.abs(r32 - r64).max())
            exact += slack == 0
            for v in (img, tap[cand.plane]):
                lo, hi = Q.plane_range(v)
                ulp = float(np.spacing(np.float32(max(abs(lo), abs(hi)))))
                diff = float(np.abs(Q.warp_wrap_f32(v, cand.inv, shift).astype(np.float64) - Y.warp_wrap(v, Q.full3(h))).max())
                bound = 4 * ulp + float(hi - lo) * slack
                worst = max(worst, diff / bound if bound else float(diff > 0))
                assert diff <= bound, (name, cand.tag, diff, bound, slack)
    print(f"float32 wrap warp against the float64 yardstick: largest share of its bound {worst:.3f}; {exact} candidates with exact float32 coordinates")
    assert exact >= 100


def test_census_every_named_rule_is_reached():
    total = dict.fromkeys(Q.CENSUS_RULES, 0)
    for name in NAMES:
        for k, v in Q.census(name).items():
            total[k] += v
    print("census (pixels, or candidates for 'warp wholly outside'): " + "; ".join(f"{k}: {v}" for k, v in total.items()))
    for k, v in total.items():
        assert v > 0, k
    # the rules that need particular planes are reached where the table says
    c = Q.census("range_rules/12x20")
    assert c["preserved zero"] > 0 and c["clipped up"] > 0 and c["clipped down"] > 0
    assert all(Q.census(n)["float64 decides the mask differently"] > 0 for n in ("far_and_odd/9x14", "far_and_odd/16x24", "seam/16x24"))
    assert all(Q.census(n)["two periods away"] > 0 for n in NAMES if not n.startswith("largest_sides/"))


@pytest.mark.parametrize("vname", list(Q.VARIANTS))
def test_every_wrong_rule_changes_an_exact_item(vname):
    v = Q.VARIANTS[vname]
    bites = {name: Q.variant_bites(vname, name) for name in v.probes}
    hit = {name: b for name, b in bites.items() if b}
    if v.finite_blind:
        # arithmetic rules the bite out on any finite plane of normal numbers: asserted, and shown on a plane no context accepts
        assert not hit, (vname, hit)
        kw = dict(v.kw)
        if "ceil_rule" in kw:
            img = Q.planes("far_and_odd/9x14")[1][0].copy()
            img[4, 7] = np.nan
            good, bad = Q.warp_wrap_f32(img, Q.IDENTITY6, (2, -3)), Q.warp_wrap_f32(img, Q.IDENTITY6, (2, -3), **kw)
            assert np.isnan(good).sum() == 1 and np.isnan(bad).sum() > 1
            what = f"a NaN pixel leaks into {int(np.isnan(bad).sum())} pixels for 1"
        else:
            img = np.full((9, 14), np.float32(1e-45))                       # the smallest subnormal: half of it rounds to 0
            good, bad = Q.warp_wrap_f32(img, (1.0, 0.0, 0.5, 0.0, 1.0, 0.0), (0, 0)), Q.warp_wrap_f32(img, (1.0, 0.0, 0.5, 0.0, 1.0, 0.0), (0, 0), **kw)
            assert (good == img).all() and (bad == 0).all()
            what = "an underflowed mix stays 0 for the plane's minimum"
        print(f"{vname} ({v.rule}): no finite plane of normal numbers can show it ({v.finite_blind}); on a host-only plane: {what}")
        return
    for name, b in hit.items():
        print(f"{vname} ({v.rule}): {name}: {len(b)} items, e.g. {b[0]}")
    assert hit, vname


def test_every_candidate_is_fit_for_the_score_comparison():
    """kappa <= 1e4 and a finite reference score on every candidate at the host's shift, except the deliberately degenerate
    ones, which are listed with the reference's value: NaN (empty mask), 0 (constant plane), 0 (zero plane)."""
    worst, listed, n = 0.0, {}, 0
    for name in NAMES:
        ref, mov, tap = Q.planes(name)
        for cand, idx in zip(Q.candidates(name), Q.host_indices(name)):
            r = Q.restate(name, cand, Q.midpoint_shift(idx, ref.shape))
            why = Q.degenerate_reason(name, cand, r)
            n += 1
            if why is None:
                assert np.isfinite(r["score"]) and max(r["kappa"]) <= Q.KAPPA_MAX and r["nmask"] >= 2, (name, cand.tag, r["score"], r["kappa"], r["nmask"])
                assert 0 < r["allowance"] <= 8 * r["nmask"] * Q.U * Q.KAPPA_MAX
                worst = max(worst, max(r["kappa"]))
                continue
            assert Q.BY_NAME[name].degenerate, (name, cand.tag, why)
            reason, value = why
            assert (np.isnan(r["score"]) and np.isnan(value)) or r["score"] == value == 0.0, (name, cand.tag, why, r["score"])
            assert r["allowance"] == 0.0
            listed.setdefault((name, reason), []).append(cand.tag)
    print(f"{n} candidates; largest kappa of the others {worst:.1f}")
    for (name, reason), tags in sorted(listed.items()):
        value = "NaN" if reason == "empty mask" else "0"
        print(f"  {name}: {reason} (reference {value}) on {len(tags)} candidates: " + ", ".join(tags[:4]) + (" ..." if len(tags) > 4 else ""))
    reasons = {reason for _, reason in listed}
    assert reasons == {"empty mask", "constant plane", "zero plane"}
    assert {name for name, reason in listed if reason == "empty mask"} == {"taper_rules/12x20"}
    assert {name for name, reason in listed if reason == "zero plane"} == {"range_rules/12x20"}
