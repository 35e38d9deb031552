"""The score, arg-max and threshold reductions at every seam: each probe of tests/reduction_probes.py runs on the device —
k_pair_sums through cross_correlation_coefficient / cosine_similarity, k_argmax_rows through hh_argmax_device on scores uploaded
with torch (indices through a caller's device buffer or through h_index, as the probe says), k_array_max / k_threshold through
SweepEngine.threshold_data — against its reference, and prints its figure before it asserts.  The hh_argmax probes run the host
twin on the same rows.  tests/test_reduction_probes_host.py shows, without a device, that each comparison made here notices its
rule being wrong.

Bounds: the pair scores are held to 8 K(n) 2^-53, K(n) the longest chain of float64 additions (derived in the docstring of
reduction_probes.py; 9.2e-13 at the largest length); indices, refusals and threshold outputs are compared exactly, the latter
bit for bit with NaN positions.  No bound was measured or widened."""
import ctypes as C

import numpy as np
import pytest

import reduction_probes as Q
import helicon_amd as H
from helicon_amd import _lib

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    with H.SweepEngine(64) as e:
        yield e


def _device_argmax(eng, scores, rows, n, ld, route):
    import torch

    t = torch.from_numpy(np.ascontiguousarray(scores)).cuda()
    torch.cuda.synchronize()
    if route == "h":
        return eng.argmax_device(t.data_ptr(), rows, n, ld)
    idx = torch.full((rows,), -7, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    assert eng.argmax_device(t.data_ptr(), rows, n, ld, d_index=idx.data_ptr()) is None
    eng.synchronize()
    return idx.cpu().numpy()


def _host_argmax(scores, n):
    L = _lib.lib()
    out = np.full(scores.shape[0], -7, dtype=np.int64)
    idx = C.c_int64(-7)
    for r in range(scores.shape[0]):
        row = np.ascontiguousarray(scores[r, :n])
        assert L.hh_argmax(row.ctypes.data_as(C.POINTER(C.c_float)), n, C.byref(idx)) == 0
        out[r] = idx.value
    return out


def run_on_device(p, inp, eng):
    a = p.args
    if p.kind == "pearson":
        return eng.cross_correlation_coefficient(inp["a"], inp["b"])
    if p.kind == "cosine":
        return eng.cosine_similarity(inp["a"], inp["b"])
    if p.kind == "argmax":
        return _device_argmax(eng, inp["scores"], len(a["cases"]), a["n"], a["ld"], a["route"])
    if p.kind == "argmax_host":
        return _host_argmax(inp["scores"], a["n"])
    if p.kind == "argmax_refusal":
        import torch

        t = torch.from_numpy(inp["scores"]).cuda()
        torch.cuda.synchronize()
        rows, n, ld = a["bad"]
        out = np.full(max(len(a["cases"]), 2), -7, dtype=np.int64)
        rc = _lib.lib().hh_argmax_device(eng._ctx, C.c_void_p(t.data_ptr()), rows, n, ld, None, out.ctypes.data_as(C.POINTER(C.c_int64)))
        refused = rc != 0 and (out == -7).all() and b"hh_argmax_device: bad argument" in _lib.lib().hh_last_error(eng._ctx)
        return ("refused" if refused else f"rc {rc}", _device_argmax(eng, inp["scores"], len(a["cases"]), a["n"], a["ld"], a["route"]))
    if p.kind == "threshold":
        kw = dict(thresh_fraction=a["thresh"]) if a["mode"] == "fraction" else dict(thresh_value=a["thresh"])
        return eng.threshold_data(inp["data"], **kw)
    raise KeyError(p.kind)


@pytest.mark.parametrize("name", [p.name for p in Q.PROBES])
def test_probe_on_the_device_against_its_reference(name, eng):
    p = Q.BY_NAME[name]
    inp = p.inputs()
    want = Q.reference(p, inp)
    got = run_on_device(p, inp, eng)
    v = Q.compare(p, got, want, inp)
    print(f"REDUCTION_FIGURE {name} | {p.rule} | figure {v.figure:.3e} bound {v.bound:.3e} exact-mismatches {v.mismatches} {v.note}")
    assert v.ok, (name, p.rule, v)


REPEATED = ("pearson/noise/n524295/f32", "pearson/noise/n262145/f64", "cosine/noise/n524295/f32", "cosine/spike262144/n524295/f32",
            "argmax/r5/n100003/ld100040/d/g0", "argmax/r1/n2049/ld0/h/tie_5_1029", f"argmax/r{Q.ROW_CAP}/n3/ld0/h/cap",
            "threshold/mixed/n524295/fraction0.3", "threshold/neg/n262145/fraction0.5", "threshold/nan262144/n262401/value0.5")


@pytest.mark.parametrize("name", REPEATED)
def test_a_probe_gives_the_same_bits_run_after_run(name, eng):
    p = Q.BY_NAME[name]
    inp = p.inputs()
    first = run_on_device(p, inp, eng)
    for _ in range(3):
        again = run_on_device(p, inp, eng)
        assert np.asarray(first).tobytes() == np.asarray(again).tobytes(), name
