"""The soft masks built on the device (csrc/soft_mask.inc: hh_edt_3d, hh_soft_mask_3d, hh_tfsm_set_support / _soft_mask /
_soft_masked) against SciPy's exact distance transform, the host's soft_mask (pinned to the reference by
tests/golden/g20_true_fsc.npz) and the float64 restatement of the true FSC.

Inputs: the ellipsoid supports of tests/soft_mask_cases.py (24^3, 26^3, 44^3 and 20 x 27 x 33) at the widths 2.5, 9.3 and 13.7
(steps 1, 2, 3).  No case holds a tie (an outside voxel whose distance equals the width to within rounding, where the edge
jumps from 0.5 to 0): every test asserts min |dist - w| >= 1e-9 first (the twelve values lie between 4.2e-4 and 5.1e-2).
44^3 at 13.7 shows the last-plane quirk (1,936 outside voxels at 1 on each last plane), 24^3 and 20 x 27 x 33 at 13.7 hold
outside voxels whose interpolated distance is exactly 0.

Bounds, none of them measured:
* the squared distances: exact (integers);
* the mask against np.float32(soft_mask): the same zeros, and max |d| <= 2^-24: both sides round one float64 value, equal to
  within a few ulp, to float32, the values lie in {0} and [0.5, 1], and the spacing of float32 there is 2^-24;
* curves through the resident context against curves through an uploaded copy of the same mask: bit for bit;
* against float64: the project's TOL_FSC_3D = 3e-7 for fsc_t and 9e-7 for fsc_n, under its FLOOR condition on the shells'
  denominators (tests/test_gpu_true_fsc.py).
Every test prints its figures (SOFT_MASK_FIGURE) before it asserts."""
import importlib

import numpy as np
import pytest

import fsc_oracle as O
import soft_mask_cases as SC
import true_fsc_oracle as TO
import helicon_amd as H
from tests import test_gpu_true_fsc as TT

T = importlib.import_module("helicon_amd.true_fsc")

pytestmark = pytest.mark.gpu

TOL_MASK = 2.0**-24
CASES = [(b, w) for b in SC.BOXES for w in SC.WIDTHS]
_host = {}


def _reference(box, w):
    """(support, the host's mask, min |dist - w| outside), computed once."""
    key = (box[0], w)
    if key not in _host:
        S = SC.ellipsoid(*box)
        _host[key] = (S, T.soft_mask(S, w), SC.tie_margin(S, w))
    return _host[key]


def _edt_reference(S, s):
    from scipy.ndimage import distance_transform_edt

    return np.rint(distance_transform_edt(~(S[::s, ::s, ::s] != 0)) ** 2).astype(np.int32)


def _edt_cases():
    cases = [(f"{'x'.join(map(str, b[0]))}/{s}", SC.ellipsoid(*b), s) for b in SC.BOXES for s in (1, 2, 3)]
    corner = np.zeros((5, 6, 70), np.uint8)
    corner[0, 0, 0] = 1
    far = np.zeros((5, 6, 70), np.uint8)
    far[4, 5, 69] = 1
    line = np.zeros((1, 1, 64), np.uint8)
    line[0, 0, [9, 40]] = 1
    long = (np.random.RandomState(5).uniform(size=(8, 8, 1024)) < 0.002).astype(np.uint8)
    long[:, :, 300:700] = 0
    long[3, 4, 1023] = 1
    tall = np.zeros((1024, 3, 2), np.uint8)
    tall[[5, 900], 1, 1] = 1
    cases += [("corner", corner, 1), ("far corner", far, 1), ("corner/3", corner, 3), ("full", np.ones((7, 9, 11), np.uint8), 1),
              ("full/2", np.ones((7, 9, 11), np.uint8), 2), ("line 1x1x64", line, 1), ("8x8x1024", long, 1), ("8x8x1024/2", long, 2),
              ("1024x3x2", tall, 1)]
    return cases


@pytest.mark.parametrize("name,S,s", _edt_cases(), ids=[c[0] for c in _edt_cases()])
def test_squared_distance_transform_is_exact(name, S, s):
    want = _edt_reference(S, s)
    got = H.distance_transform_edt_sq(S, s)
    print(f"SOFT_MASK_FIGURE edt {name} shape={got.shape} max={int(want.max())} differing={int((got != want).sum())} "
          f"kernel_ms={T.distance_transform_edt_sq.kernel_ms:.3f}")
    assert got.dtype == np.int32 and got.shape == want.shape and np.array_equal(got, want)
    assert np.array_equal(got, H.distance_transform_edt_sq(S, s))                     # run to run
    if name == "full":
        assert not got.any()
    if name == "8x8x1024":
        assert int(want.max()) > 150**2                                               # the envelope runs far along the longest line


@pytest.mark.parametrize("box,w", CASES, ids=[f"{'x'.join(map(str, b[0]))}-{w}" for b, w in CASES])
def test_soft_mask_device_against_the_host(box, w):
    S, host, margin = _reference(box, w)
    assert margin >= SC.TIE                                                           # the tie condition
    want = np.float32(host)
    got = H.soft_mask_device(S, w)
    err = float(np.abs(got.astype(np.float64) - want).max())
    print(f"SOFT_MASK_FIGURE mask box={box[0]} w={w} tie_margin={margin:.3e} max_err={err:.3e} not_bit_equal={float((got != want).mean()):.3e} "
          f"zeros={int((want == 0).sum())} edge={int(((want > 0) & (want < 1)).sum())}")
    if box[0] == (44, 44, 44) and w == 13.7:                                          # the last-plane quirk
        for plane, sup in ((host[-1], S[-1]), (host[:, -1], S[:, -1]), (host[:, :, -1], S[:, :, -1])):
            assert int(((plane == 1) & (sup == 0)).sum()) == 1936
    if box[0] in ((24, 24, 24), (20, 27, 33)) and w == 13.7:                          # interpolated distance exactly 0
        assert ((SC.distance(S, w) == 0) & (S == 0)).any()
    assert got.dtype == np.float32 and got.shape == S.shape
    assert np.array_equal(got == 0, want == 0)
    assert err <= TOL_MASK
    assert np.array_equal(got, H.soft_mask_device(S.astype(np.float64), w))            # run to run, any dtype of the support


def test_soft_mask_device_edge_cases():
    S = SC.cube_support(24)
    assert np.array_equal(H.soft_mask_device(S, 0), S.astype(np.float32))
    lonely = np.zeros((24, 24, 24), np.uint8)
    lonely[5, 7, 9] = 1
    with pytest.raises(ValueError, match="step 2"):
        H.soft_mask_device(lonely, 9.3)
    with pytest.raises(ValueError, match="NaN"):
        H.soft_mask_device(S, float("nan"))
    # the library's own refusals, past the Python ones
    import ctypes as C
    from helicon_amd import _lib

    L = _lib.lib()
    out, d2 = np.zeros(S.shape, np.float32), np.zeros((12, 12, 12), np.int32)
    u8p, f32p, i32p = C.POINTER(C.c_uint8), C.POINTER(C.c_float), C.POINTER(C.c_int32)
    assert L.hh_soft_mask_3d(0, lonely.ctypes.data_as(u8p), 24, 24, 24, 9.3, out.ctypes.data_as(f32p), None) == -1
    assert b"step 2" in L.hh_last_error(None)
    assert L.hh_edt_3d(0, lonely.ctypes.data_as(u8p), 24, 24, 24, 2, d2.ctypes.data_as(i32p), None) == -1
    assert b"step 2" in L.hh_last_error(None)
    assert np.array_equal(H.soft_mask_device(lonely, 2.5) == 1, lonely == 1)           # and the device still works


def _shifted(n):
    """A second support for the n^3 maps."""
    box = [b for b in SC.BOXES if b[0] == (n, n, n)][0]
    return SC.ellipsoid(box[0], tuple(c - 2 for c in box[1]), box[2] * 0.8)


@pytest.mark.parametrize("n", (24, 44))
def test_context_equals_the_upload_path_bit_for_bit(n):
    a, b, u = TT._inputs(n)
    S, S2 = SC.cube_support(n), _shifted(n)
    for w in SC.WIDTHS:
        assert SC.tie_margin(S, w) >= SC.TIE
    with H.TrueFSC(a, b, TT.APIX, TT._cutoff(n), phases=u) as dev, H.TrueFSC(a, b, TT.APIX, TT._cutoff(n), phases=u) as again:
        dev.set_support(S)
        again.set_support(S)
        singles = {}
        for w in SC.WIDTHS:
            mask = dev.soft_mask(w)
            assert mask.dtype == np.float32 and np.array_equal(mask, H.soft_mask_device(S, w))
            assert np.array_equal(mask, dev.soft_mask(w, which=1))                     # one support: both members
            for per_shell in (False, True):
                got, want = dev.soft_masked(w, per_shell), dev.masked(mask, per_shell=per_shell)
                assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
                other = again.soft_masked(w, per_shell)
                assert np.array_equal(got[0], other[0]) and np.array_equal(got[1], other[1])
            singles[w] = dev.soft_masked_sums([w])[0]
            assert np.array_equal(singles[w], dev.masked_sums(mask[None])[0])
        order = [13.7, 2.5, 2.5, 9.3, 13.7, 0.0, 9.3]
        batch = dev.soft_masked_sums(order)
        assert batch.shape == (len(order), 2, n // 2 + 1, 3)
        for j, w in enumerate(order):
            want = singles[w] if w > 0 else dev.masked_sums(S.astype(np.float32)[None])[0]      # w = 0: the support itself
            assert np.array_equal(batch[j], want), (j, w)
        assert np.array_equal(batch, again.soft_masked_sums(order))
        t, nz = dev.soft_masked_batch(order[:4])
        assert np.array_equal(t[1], dev.soft_masked(2.5)[0]) and np.array_equal(nz[3], dev.soft_masked(9.3)[1])
        # two supports against one
        dev.set_support(S, S2)
        for w in (2.5, 13.7):
            m1, m2 = dev.soft_mask(w, 0), dev.soft_mask(w, 1)
            assert np.array_equal(m1, H.soft_mask_device(S, w)) and np.array_equal(m2, H.soft_mask_device(S2, w)) and not np.array_equal(m1, m2)
            got = dev.soft_masked_sums([w, w])
            assert np.array_equal(got[0], dev.masked_sums(m1[None], m2[None])[0]) and np.array_equal(got[0], got[1])
            assert not np.array_equal(got[0], singles[w])
        dev.set_support(S, S)
        assert np.array_equal(dev.soft_masked_sums([9.3])[0], singles[9.3])
        dev.set_support(S)
        assert np.array_equal(dev.soft_masked_sums([9.3])[0], singles[9.3])


@pytest.mark.parametrize("n", (24, 44))
def test_context_against_float64(n):
    a, b, u = TT._inputs(n)
    cutoff = TT._cutoff(n)
    S = SC.cube_support(n)
    ora = TO.OracleTrueFSC(a, b, TT.APIX, cutoff, phases=u)
    with H.TrueFSC(a, b, TT.APIX, cutoff, phases=u) as dev:
        dev.set_support(S)
        for w in SC.WIDTHS:
            assert SC.tie_margin(S, w) >= SC.TIE
            host = T.soft_mask(S, w)
            for per_shell in (False, True):
                sums = ora.masked_sums(host[None], None, per_shell)[0]
                floor = min(O.floor_ratio(sums[0]), O.floor_ratio(sums[1]))
                t, nz = dev.soft_masked(w, per_shell)
                wt, wn = ora.masked(host, per_shell=per_shell)
                if not per_shell:
                    t, nz, wt, wn = t[:, 1], nz[:, 1], wt[:, 1], wn[:, 1]
                e_t, e_n = TT._err(t, wt), TT._err(nz, wn)
                print(f"SOFT_MASK_FIGURE float64 n={n} w={w} per_shell={int(per_shell)} floor={floor:.3e} fsc_t={e_t:.3e} fsc_n={e_n:.3e}")
                assert floor >= TT.FLOOR
                assert e_t <= TT.TOL_FSC_3D and e_n <= TT.TOL_ROUND_TRIP


def test_true_fsc_with_device_masks():
    n, W = 32, 6.2         # 3.1 pixels: between sqrt(9) and sqrt(10), no tie at step 1
    a, b = TT._blob_pair(n, 4100)
    rng = np.random.RandomState(41)
    u = tuple(rng.uniform(0, 2 * np.pi, size=(n, n, n // 2 + 1)) for _ in range(2))
    cutoff = TT._cutoff(n)
    support = T.adaptive_mask((a.astype(np.float64) + b) / 2, TT.APIX, cutoff)
    assert SC.tie_margin(support, W / TT.APIX) >= SC.TIE
    dev = T.true_fsc(a, b, TT.APIX, cutoff_res=cutoff, phases=u, one_mask=True, mask_soft=W, device_masks=True)
    host = T.true_fsc(a, b, TT.APIX, cutoff_res=cutoff, phases=u, one_mask=True, mask_soft=W)
    e = {k: TT._err(dev[k][:, 1], host[k][:, 1]) for k in ("masked", "randomized_masked", "true")}
    print("SOFT_MASK_FIGURE true_fsc " + " ".join(f"{k}={v:.3e}" for k, v in e.items()) +
          f" host_mask_s device={dev['host_mask_s']:.4f} host={host['host_mask_s']:.4f}")
    assert e["masked"] <= TT.TOL_FSC_3D and e["randomized_masked"] <= TT.TOL_ROUND_TRIP and e["true"] <= TT.TOL_ROUND_TRIP
    assert dev["mask_soft_px"] == host["mask_soft_px"] == W / TT.APIX and dev["mask1"] is dev["mask2"]
    assert dev["mask1"].dtype == np.float32 and np.array_equal(dev["mask1"], H.soft_mask_device(support, W / TT.APIX))
    assert np.array_equal(dev["unmasked"], host["unmasked"])
    with pytest.raises(ValueError, match="device_masks"):
        T.true_fsc(a, b, TT.APIX, cutoff_res=cutoff, phases=u, mask=host["mask1"], device_masks=True)
    ref = T.true_fsc(a, b, TT.APIX, cutoff_res=cutoff, phases=u, one_mask=True, refine_mask=True, device_masks=True)
    print(f"SOFT_MASK_FIGURE true_fsc refine width={ref['mask_soft_px']:.4f} res={ref['resolution']['true']:.4f}")
    assert 0 < ref["mask_soft_px"] < n / 3
    assert np.array_equal(ref["mask1"], H.soft_mask_device(support, ref["mask_soft_px"]))


def test_widths_across_the_launch_cut():
    """2,060 widths on one 8^3 context: launches of 2047 and 13 widths, after a call with 3 widths (the scratch grows)."""
    n, cap = 8, 65535 // (4 * 8)
    assert cap == 2047
    a, b, u = TT._inputs(n)
    S = np.zeros((n, n, n), np.uint8)
    S[2:6, 3:6, 2:5] = 1
    widths = np.random.RandomState(8).uniform(0.5, 2.6, size=2060)
    idx = np.unique(np.concatenate([np.arange(cap - 8, cap + 8), [0, 1, len(widths) - 2, len(widths) - 1]]))
    with H.TrueFSC(a, b, TT.APIX, TT._cutoff(n), phases=u) as dev, H.TrueFSC(a, b, TT.APIX, TT._cutoff(n), phases=u) as fresh:
        dev.set_support(S)
        fresh.set_support(S)
        first = dev.soft_masked_sums(widths[:3])
        for per_shell in (False, True):
            big = dev.soft_masked_sums(widths, per_shell)
            assert big.shape == (2060, 2, n // 2 + 1, 3) and np.isfinite(big).all()
            for i in idx:
                assert np.array_equal(big[i], dev.soft_masked_sums(widths[i: i + 1], per_shell)[0]), i
            assert np.array_equal(big, fresh.soft_masked_sums(widths, per_shell))      # no small call came first there
        assert np.array_equal(first, dev.soft_masked_sums(widths[:3]))
        distinct = len({big[i].tobytes() for i in idx})
        print(f"SOFT_MASK_FIGURE launch cut widths={len(widths)} compared={len(idx)} distinct={distinct}")
        assert distinct > len(idx) // 2                                                 # the members differ: a shifted index would show
