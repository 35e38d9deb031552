"""The image preparation kernels and the non-cosine scores at every boundary rule and seam: each probe of
tests/image_prep_probes.py runs on the device — through the Python wrapper, or through the C entry point where the wrapper
cannot reach the path (a projective matrix, cval, clip = 0, raw moments, raw counts) — against its reference, and prints its
figure before it asserts.  tests/test_image_prep_probes_host.py shows, without a device, that each comparison made here
notices its rule being wrong.

Bounds are those of the existing tests of the same function, times max |input| where the input is not of order 1: warp 2e-6
(float32) / 1e-12 (float64) with no pixel left out, since one matrix goes to both sides; rotate_shift_image 1e-6 (order 1) /
2e-6 (order 3); rescale 3e-6 / 1e-11; ssim 2e-6, ms_ssim 5e-6, mutual information 1e-12.  Compared exactly: histogram counts;
mask pixel count, first and last row; outside verdicts (got == 0 against want == 0); NaN positions; order-0 warps.  The five
moment quotients are held to the cost of a float64 sum in another order, 4 n 2^-53 of the sum of the absolute terms per case
(image_prep_probes.moments_numpy): their figure is printed in units of that bound.  No bound was measured or widened; the
largest figures an MI355X gave are in DESIGN.md, "Image preparation probes"."""
import ctypes as C

import numpy as np
import pytest

import image_prep_probes as Q
from helicon_amd import _lib
from helicon_amd import denovo3D as D
from helicon_amd import solver as S

pytestmark = pytest.mark.gpu


def _dptr(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _fptr(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def run_on_device(p, inp):
    a, L = p.args, _lib.lib()
    if p.kind == "warp":
        img = np.ascontiguousarray(inp["image"])
        m = np.ascontiguousarray(a["matrix"], dtype=np.float64)
        out = np.empty_like(img)
        _lib.check(L.hh_warp_affine_2d(0, img.ctypes.data, int(img.dtype == np.float64), img.shape[0], img.shape[1], _dptr(m), int(a["order"]),
                                       float(a["cval"]), int(a["clip"]), out.ctypes.data), None)
        return out
    if p.kind == "transform_image":
        return D.transform_image(inp["image"], **a)
    if p.kind == "rotate":
        return D.rotate_shift_image(inp["image"], a["angle"], a["pre"], a["post"], order=a["order"])
    if p.kind == "rescale":
        return D.rescale(inp["image"], a["scale"], order=a["order"], anti_aliasing=a["anti_aliasing"], clip=a["clip"])
    if p.kind == "moments":
        img = np.ascontiguousarray(inp["image"])
        out = np.zeros(8)
        _lib.check(L.hh_helix_moments(0, img.ctypes.data, int(img.dtype == np.float64), img.shape[0], img.shape[1], float(a["threshold"]), _dptr(out)), None)
        return out
    if p.kind == "ssim":
        return S.ssim_score(inp["a"], inp["b"])
    if p.kind == "ms_ssim":
        return S.ms_ssim_score(inp["a"], inp["b"])
    if p.kind == "mi":
        return S.mutual_information_score(inp["a"], inp["b"])
    if p.kind == "hist":
        x, y = np.ascontiguousarray(inp["a"].ravel()), np.ascontiguousarray(inp["b"].ravel())
        ea, eb = Q.hist_edges(p, inp)
        bins = a["bins"]
        counts = np.full((bins, bins), -1, dtype=np.int64)
        _lib.check(L.hh_joint_histogram(0, _fptr(x), _fptr(y), x.size, _dptr(ea), _dptr(eb), bins, counts.ctypes.data_as(C.POINTER(C.c_int64))), None)
        return counts
    raise KeyError(p.kind)


@pytest.mark.parametrize("name", [p.name for p in Q.PROBES])
def test_probe_on_the_device_against_its_reference(name):
    p = Q.BY_NAME[name]
    inp = p.inputs()
    want = Q.reference(p, inp)
    got = run_on_device(p, inp)
    v = Q.compare(p, got, want, inp)
    print(f"PROBE {name} | {p.rule} | figure {v.figure:.3e} bound {v.bound:.3e} exact-mismatches {v.mismatches} {v.note}")
    assert v.ok, (name, p.rule, v)
