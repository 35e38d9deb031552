"""The 3-D map resampling kernels at every rule, border and side: each probe of tests/map_geometry_probes.py runs on the device —
transform_map (k_f32_to_f64, k_spline_prefilter on three axes, k_map_cubic), apply_helical_symmetry (k_apply_helical_symmetry and
its host plan), symmetrize_transform_map, generate_xyz_projections (k_map_proj_slices, k_map_proj_columns; through
hh_map_projections where the wrapper cannot reach the slab) — against its reference, and prints its figure before it asserts.
tests/test_map_geometry_probes_host.py shows, without a device, that each comparison made here notices its rule being wrong and
that none of its exact items hangs on the last bit of the host's cos / sin.

Bounds are those of the existing tests of the same function: transform_map 2e-6 max|want| with the zero pattern equal,
apply_helical_symmetry 1e-6 absolute on inputs in [0, 1], projections 1e-6 max|want| of each projection (an empty slab exactly),
symmetrize_transform_map 2e-6 max|want|.  No pixel is left out and no bound was measured or widened; the largest figures an
MI355X gave are in profiles/map_geometry.json."""
import ctypes as C

import numpy as np
import pytest

import map_geometry_probes as Q
import helicon_amd as H
from helicon_amd import _lib

pytestmark = pytest.mark.gpu


def _fptr(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def run_on_device(p, inp):
    a, vol = p.args, inp["vol"]
    if p.kind == "transform_map":
        return H.transform_map(vol, a["scale"], a["rot"], a["tilt"], a["psi"], a["dx"], a["dy"], a["dz"])
    if p.kind == "helical":
        return H.apply_helical_symmetry(vol, a["apix"], a["twist"], a["rise"], a["csym"], a["fraction"], a["new_size"], a["new_apix"])
    if p.kind == "symmetrize":
        return H.symmetrize_transform_map(vol, a["apix"], a["twist"], a["rise"], a["csym"], a["fraction"], a["new_size"], a["new_apix"],
                                          a["axial_rotation"], a["tilt"])
    if p.kind == "projections":
        if "slab" not in a:
            return H.generate_xyz_projections(vol, **a)
        v = np.ascontiguousarray(vol, dtype=np.float32)
        nz, ny, nx = v.shape
        out = [np.full(s, np.nan, np.float32) for s in ((nz, ny), (nz, nx), (ny, nx))]
        _lib.check(_lib.lib().hh_map_projections(0, _fptr(v), (C.c_int32 * 3)(nz, ny, nx), int(a["slab"][0]), int(a["slab"][1]),
                                                 *(_fptr(o) for o in out)), None)
        return out
    raise KeyError(p.kind)


@pytest.mark.parametrize("name", [p.name for p in Q.PROBES])
def test_probe_on_the_device_against_its_reference(name):
    p = Q.BY_NAME[name]
    inp = p.inputs()
    want = Q.reference(p, inp)
    got = run_on_device(p, inp)
    v = Q.compare(p, got, want, inp)
    print(f"MAPGEO_FIGURE {name} {v.figure:.3e} {v.bound:.3e} | exact-mismatches {v.mismatches} | {p.rule} {v.note}")
    assert v.ok, (name, p.rule, v)


@pytest.mark.parametrize("name", ["transform_map/euler/5x7x11/f32", "helical/size_mixed_a_r0.8/12x11x13", "projections/thin/2x5x257/f32",
                                  "symmetrize/filter_mixed/12x11x13"])
def test_a_probe_of_each_kind_is_bit_identical_from_run_to_run(name):
    p = Q.BY_NAME[name]
    inp = p.inputs()
    first, again = run_on_device(p, inp), run_on_device(p, inp)
    for a, b in zip(first, again) if isinstance(first, list) else ((first, again),):
        np.testing.assert_array_equal(a, b)
