"""The structure-factor kernels at every tile seam, table turn and launch cap: each probe of tests/structure_factor_seams.py runs
on the device against the float64 restatement (tests/structure_factor_oracle.py) — the spectrum elementwise, the profile per
bin and the map matched onto a target of another voxel size, on noise-floored random data — and prints its figures before it
asserts.  tests/test_structure_factor_seams_host.py shows, without a device, that the unit-impulse probe of
tests/test_gpu_structure_factor.py is blind to a lost slice, a misread column tile, swapped row tiles and every strided tail,
and that each comparison made here moves by at least 100 times its bound under the defect it is for.

Bounds: per shape, the existing 2e-6 where the figure an MI355X gave lies within it, else that figure times 4, rounded up to
one significant digit (structure_factor_seams.MEASURED, bounds(); profiles/structure_factor.json, "accuracy" / "seams").  The floor
(every bin's mean power per voxel at least 1e-4 of the strongest bin's) is asserted on both profiles of every comparison; no
bin and no voxel is left out.  The batch and scaling probes are exact: a power-of-two factor commutes with every float32 and
float64 step, shifts the exponent of the fixed-point scale by twice its own and leaves the integer sums as they are."""
import numpy as np
import pytest

import structure_factor_oracle as O
import structure_factor_seams as Q
import helicon_amd as H

pytestmark = pytest.mark.gpu


def run_probe(p, variant):
    """(figures, floors, qbins equal) of one probe and variant on the device"""
    inp = Q.inputs(p)
    y = Q.yardstick(p, variant)
    thresh, thresh_t, mask = Q.variant_args(inp, variant)
    qbins, sf, F = H.calculate_structural_factor(inp["data"], p.apix, thresh, mask, True)
    out = H.match_structural_factors(inp["data"], p.apix, inp["target"], p.apix_target, thresh, thresh_t, mask)
    assert F.shape == p.shape and out.shape == p.shape and sf.dtype == np.float64
    return Q.figures(y, F, sf, out), Q.floors(p, variant), bool(np.array_equal(qbins, y["qbins"]))


@pytest.mark.parametrize("name,variant", Q.CASES)
def test_probe_on_the_device_against_the_float64_restatement(name, variant):
    p = Q.BY_NAME[name]
    e, floors, same_bins = run_probe(p, variant)
    b = Q.bounds(p)
    print(f"SF_FIGURE seam {name} {variant}: spectrum={e[0]:.3e} (bound {b[0]:.0e}) sf={e[1]:.3e} ({b[1]:.0e}) match={e[2]:.3e} ({b[2]:.0e}) "
          f"floor data={floors[0]:.2e} target={floors[1]:.2e} | {p.seam}")
    assert same_bins and min(floors) >= Q.FLOOR
    assert e[0] <= b[0] and e[1] <= b[1] and e[2] <= b[2], (name, variant, e, b)


def test_a_batch_of_maps_of_very_different_magnitude_equals_the_single_calls():
    """Five maps 2^k x_k, k = (0, 40, -40, 13, -7): every map's own scale (k_sf_scales, scale[b], scale[i / nbins]) next to
    neighbours 2^80 apart.  With a mask and a threshold, the threshold follows the map: one call of the stack per threshold."""
    b = Q.batch_inputs()
    maps, mask = b["maps"], b["mask"]
    worst = 0.0
    with H.StructureFactorMatcher(Q.BATCH_SHAPE, Q.BATCH_APIX, b["tbins"], b["tsf"]) as m:
        calls = [dict()] + [dict(mask=mask, thresh=float(np.ldexp(b["thresh"], k))) for k in Q.BATCH_EXPONENTS]
        for kw in calls:
            sf, out = m.profile(maps, **kw), m.match(maps, **kw)
            for j in range(len(maps)):
                assert np.array_equal(sf[j], m.profile(maps[j], **kw)), (j, sorted(kw))
                assert np.array_equal(out[j], m.match(maps[j], **kw)), (j, sorted(kw))
            if not kw:
                for j in range(len(maps)):
                    want = O.calculate_structural_factor(maps[j], Q.BATCH_APIX)[1]
                    assert O.floor_ratio(Q.BATCH_SHAPE, Q.BATCH_APIX, want) >= Q.FLOOR
                    worst = max(worst, Q.sf_error(sf[j], want))
    tol = Q.bound_from(Q.MEASURED_BATCH_SF, Q.TOL_SF)
    print(f"SF_FIGURE seam batch {Q.BATCH_SHAPE} exponents {Q.BATCH_EXPONENTS}: stack == singles bit for bit; sf={worst:.3e} (bound {tol:.0e})")
    assert worst <= tol


@pytest.mark.parametrize("route", Q.SCALING_ROUTES)
@pytest.mark.parametrize("shape,apix", Q.SCALING_SHAPES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_a_power_of_two_factor_moves_nothing_but_the_exponent(shape, apix, route):
    """profile(2^k x) == 4^k profile(x) and match(2^k x) == match(x), bit for bit, k in {+-20, +-40}"""
    s = Q.scaling_inputs(shape, apix)
    kw = dict(mask=s["mask"]) if route == "match_mask" else dict()
    with H.StructureFactorMatcher(shape, apix, s["tbins"], s["tsf"]) as m:
        call = m.profile if route == "profile" else m.match
        base = call(s["data"], **kw)
        assert np.isfinite(base).all() and np.abs(base).max() > 0
        for k in Q.SCALING_EXPONENTS:
            got = call(np.ldexp(s["data"], k).astype(np.float32), **kw)
            want = np.ldexp(base, 2 * k) if route == "profile" else base
            same = bool(np.array_equal(got, want))
            print(f"SF_FIGURE seam scaling {shape} {route} k={k}: {'bit-equal' if same else 'DIFFERENT'}")
            assert same, (shape, route, k, float(np.abs(got / want - 1.0).max()))
