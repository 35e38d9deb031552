"""Host side of the image preparation probes (tests/image_prep_probes.py; the device side is tests/test_gpu_image_prep_probes.py).
No device is needed: every probe's reference runs and is finite where it should be, the NumPy / SciPy restatements the variants
are built on ARE the oracle, and every wrong-rule variant is bitten by a probe listed for it — it changes an exactly compared
item (a count, a verdict, a NaN position, an order-0 pixel) or moves a compared number by at least 100 times that comparison's
bound — so the device test would notice the same defect in a kernel.  Where arithmetic rules a bite out, that is asserted too."""
import numpy as np
import pytest

from oracle import prep as P
import image_prep_probes as Q


def _of(kind):
    return [p for p in Q.PROBES if p.kind == kind]


def _device_shaped(probe, ref):
    return ref[0] if probe.kind == "moments" else ref


def test_every_reference_runs_and_is_finite_where_it_should_be():
    assert len(Q.PROBES) > 600
    for p in Q.PROBES:
        inp = p.inputs()
        ref = Q.reference(p, inp)
        assert Q.compare(p, _device_shaped(p, ref), ref, inp).ok, p.name           # the comparison accepts the reference itself
        for v in inp.values():
            finite = v[np.isfinite(v)]
            assert finite.size == 0 or (-1.2 <= finite.min() and finite.max() <= 6.0), p.name
        if p.kind == "moments":
            out, bound = ref
            mask = P.closing_cross(inp["image"] > p.args["threshold"])
            assert out[0] == mask.sum() and (out[0] == 0) == (p.name.split("/")[1] == "empty" or ("/equal" in p.name and "/1x9/" in p.name)), p.name
            if out[0] == 0:
                continue                                              # (the other seven outputs mean nothing: the wrapper stops at the count)
            if np.isnan(inp["image"][mask]).any():
                assert "/nan_" in p.name and np.isnan(out[1:6]).all() and np.isfinite(out[6:]).all(), p.name
            else:
                assert np.isfinite(out).all() and np.isfinite(bound).all() and (bound[1:6] <= 1e-5).all(), p.name
        elif p.kind == "hist":
            assert ref.sum() == inp["a"].size and ref.shape == (p.args["bins"],) * 2
        else:
            r = np.asarray(ref, dtype=np.float64)
            nan_in = any(np.isnan(v).any() for v in inp.values())
            assert nan_in or np.isfinite(r).all(), p.name


def test_the_probes_reach_what_they_name():
    """The inputs do what the rule column says: mixed border pixels are clipped and zeros stay, a NaN keeps the clip off, the
    step edge overshoots, the empty-range and thin shapes are what they claim."""
    for dtype in ("f32", "f64"):
        p = Q.BY_NAME[f"warp/mixed_border_clip/5x257/{dtype}"]
        img, ref = p.inputs()["image"], Q.reference(p)
        raw = P.warp_affine(img, p.args["matrix"], clip=False)
        mixed = (raw > 0) & (raw < img.min())
        assert mixed.sum() >= 5 and (ref[mixed] == img.min()).all() and (ref == 0).sum() >= 5 and (ref[raw == 0] == 0).all()
        p = Q.BY_NAME[f"warp/nan_no_clip/5x257/{dtype}"]
        ref = Q.reference(p)
        assert np.isnan(ref).sum() >= 2 and ((ref > 0) & (ref < 5)).sum() >= 5                         # NaN spreads, nothing clipped
        p = Q.BY_NAME[f"warp/cval7_clip/5x257/{dtype}"]
        assert (Q.reference(p) == 7).sum() >= 5 and (Q.reference(Q.BY_NAME[f"warp/cval7_noclip/5x257/{dtype}"]) > 2).sum() >= 5
        p, q = Q.BY_NAME[f"rescale/step_noclip/12x34/o3/{dtype}"], Q.BY_NAME[f"rescale/step_clip/12x34/o3/{dtype}"]
        img = p.inputs()["image"]
        over, clipped = Q.reference(p), Q.reference(q)
        assert over.max() > img.max() + 1e-2 and over.min() < img.min() - 1e-2                          # the cubic overshoot, kept
        assert clipped.max() == img.max() and clipped.min() == img.min()
        # a Gaussian radius beyond the line: several folds
        for name, side in ((f"rescale/s0.1/4x4/o3/{dtype}", 4), (f"rescale/s0.143/7x7/o3/{dtype}", 7)):
            sigma = (side - 1) / 2
            assert int(4 * sigma + 0.5) >= 2 * side - 2                  # the radius spans a whole mirror period: more than one fold
            assert Q.reference(Q.BY_NAME[name]).shape == (1, 1)
    # the projective probes divide by a z that stays well above 0 at every shape
    for shape in Q.WARP_SHAPES:
        y, x = np.meshgrid(np.arange(shape[0]), np.arange(shape[1]), indexing="ij")
        z = Q.PROJECTIVE[2, 0] * x + Q.PROJECTIVE[2, 1] * y + 1
        assert z.min() > 0.9
    # up-scaling folds on both sides (cc < 0 and cc > len - 1) in both orders
    for p in _of("rescale"):
        if "/s2/" in p.name:
            shape = p.inputs()["image"].shape
            out = Q.rescale_shape(shape, 2.0)
            cc = (np.arange(out[1]) + 0.5) * (shape[1] / out[1]) - 0.5
            assert cc[0] < 0 and cc[-1] > shape[1] - 1


def test_the_restatements_are_the_oracle():
    """What the variants change one rule of: with no rule changed they are oracle/prep.py (or SciPy, or NumPy) bit for bit —
    except the affine restatement, which is SciPy's verdict exactly and its order-1 values to the device's own bound."""
    for p in _of("warp"):
        inp, a = p.inputs(), p.args
        np.testing.assert_array_equal(Q.warp_numpy(inp["image"], a["matrix"], a["order"], a["cval"], bool(a["clip"])), Q.reference(p, inp), err_msg=p.name)
    for p in _of("rescale"):
        inp, a = p.inputs(), p.args
        got = Q.resize_scipy(inp["image"], Q.rescale_shape(inp["image"].shape, a["scale"]), a["order"], a["anti_aliasing"], a["clip"])
        np.testing.assert_array_equal(got, Q.reference(p, inp), err_msg=p.name)
    for p in _of("rotate"):
        inp, a = p.inputs(), p.args
        want = Q.reference(p, inp)
        got = Q.affine_numpy(inp["image"], *Q.rotate_matrix(inp["image"].shape, a["angle"], a["pre"], a["post"]))
        np.testing.assert_array_equal(got == 0, want == 0, err_msg=p.name)            # SciPy forms (m00 y + m01 x) + o
        if a["order"] == 1:
            np.testing.assert_allclose(got, want, rtol=0, atol=1e-6, err_msg=p.name)
    for p in _of("ssim"):
        inp = p.inputs()
        assert Q.ssim_numpy(inp["a"], inp["b"]) == Q.reference(p, inp), p.name
    for p in _of("hist"):
        inp = p.inputs()
        np.testing.assert_array_equal(Q.hist_numpy(inp["a"], inp["b"], *Q.hist_edges(p, inp)), Q.reference(p, inp), err_msg=p.name)
    for p in _of("moments"):
        inp = p.inputs()
        np.testing.assert_array_equal(Q.moments_numpy(inp["image"], p.args["threshold"], closing=Q.closing_variant())[0], Q.reference(p, inp)[0])


@pytest.mark.parametrize("name", list(Q.VARIANTS))
def test_every_variant_is_bitten_by_a_probe_listed_for_it(name):
    v = Q.VARIANTS[name]
    assert v.probes, name
    bitten = []
    for pname in v.probes:
        p = Q.BY_NAME[pname]
        inp = p.inputs()
        verdict = Q.compare(p, v.run(p, inp), Q.reference(p, inp), inp)
        if verdict.bitten():
            assert not verdict.ok
            bitten.append((pname, verdict.mismatches, verdict.figure, verdict.bound))
    print(f"{name}: bitten by {len(bitten)} of {len(v.probes)} listed probes, e.g. " +
          "; ".join(f"{n} (exact items {m}, moved {f:.3g} against {b:.3g})" for n, m, f, b in bitten[:3]))
    assert bitten, name


def test_what_no_probe_can_bite_by_arithmetic():
    """floor + 1 for ceil: at a non-integer coordinate they are the same corner, at an integer one the other corner carries
    weight dc = 0 exactly, and 0 * finite = 0 — on a finite image with a finite cval the variant IS the reference, bit for bit;
    only a NaN neighbour (0 * NaN) shows it, which is what the nan_identity probes are for.  The second Gaussian pass reading
    the input cannot show where one axis is filtered; the missing last edge cannot show where no value sits on it (the last
    edge is the maximum, so only a probe without its own maximum could — there is none: asserted the other way round)."""
    v = Q.VARIANTS["warp: floor + 1 for ceil"]
    for p in _of("warp"):
        inp = p.inputs()
        if np.isfinite(inp["image"]).all():
            np.testing.assert_array_equal(v.run(p, inp), Q.reference(p, inp), err_msg=p.name)
    v = Q.VARIANTS["gauss: axis 1 filtered from the input"]
    for p in _of("rescale"):
        if "axis0_only" in p.name or "axis1_only" in p.name or "/1x40/" in p.name or "/40x1/" in p.name:
            inp = p.inputs()
            np.testing.assert_array_equal(v.run(p, inp), Q.reference(p, inp), err_msg=p.name)
    v = Q.VARIANTS["hist: the last edge dropped"]
    for p in _of("hist"):
        if "/constant/" not in p.name and "/n1/" not in p.name:      # (widened edges: no value on the last edge)
            inp = p.inputs()
            assert not Q.compare(p, v.run(p, inp), Q.reference(p, inp), inp).ok, p.name
    v = Q.VARIANTS["affine: the offset added first"]
    for p in _of("rotate"):
        if "/a0_" in p.name:                                         # identity matrix: one product is exact, the sums agree
            inp = p.inputs()
            np.testing.assert_array_equal(v.run(p, inp) == 0, Q.reference(p, inp) == 0, err_msg=p.name)


def test_warp_probes_that_share_one_matrix_leave_no_pixel_out_and_the_python_level_one_has_its_margin():
    """hh_warp_affine_2d probes hand one float64 matrix to the device and to the oracle, and the kernel makes the oracle's
    float32 (float64) operations in its order with contraction off: the comparison leaves no pixel out (compare() asks that).
    transform_image composes its matrix in the wrapper, so a coordinate may differ from the oracle's in its last float32 bit:
    the probe's image is smooth enough that the oracle, evaluated with each coordinate one ulp either side, stays within the
    bound on all but the project's cap, 2e-4, of the pixels — so a device result outside it is a defect, not rounding."""
    for p in _of("warp"):                                             # one wrong pixel fails a shared-matrix probe
        inp = p.inputs()
        want = Q.reference(p, inp)
        one_off = want.copy()
        one_off.flat[0] = (0.0 if np.isnan(one_off.flat[0]) else one_off.flat[0]) + 1e-3
        assert not Q.compare(p, one_off, want, inp).ok, p.name
    p = Q.BY_NAME["transform_image/general_angle/33x47/f32"]
    inp = p.inputs()
    img, want = inp["image"], Q.reference(p, inp)
    inv = np.linalg.inv(P.transform_image_matrix(img.shape, rotation=p.args["rotation"], post_translation=p.args["post_translation"]))
    np.testing.assert_array_equal(Q.warp_numpy(img, inv), want)
    assert ((want > 0) & (want < img.max())).mean() > 0.7            # most samples are interpolated, not outside
    for nudge in ((1, 0), (-1, 0), (0, 1), (0, -1), (1, 1), (-1, -1), (1, -1), (-1, 1)):
        verdict = Q.compare(p, Q.warp_numpy(img, inv, nudge=nudge), want, inp)
        print(f"{p.name}: coordinates nudged {nudge}: share of pixels outside the bound {verdict.figure:.2e}")
        assert verdict.ok, (nudge, verdict)
    # and the comparison is not blind: the same warp a tenth of a pixel off is far outside
    off = P.warp_affine(img, inv @ np.array([[1, 0, 0.1], [0, 1, 0], [0, 0, 1.0]]))
    assert Q.compare(p, off, want, inp).figure > 0.5
