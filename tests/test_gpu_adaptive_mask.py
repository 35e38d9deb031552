"""The adaptive mask built on the device (csrc/adaptive_mask.inc: hh_am_gaussian_3d, hh_am_label_3d, hh_am_mask_3d,
hh_am_context_support) against SciPy, the host's adaptive_mask and the reference's recorded masks
(tests/golden/g20_true_fsc.npz).

Bounds, none of them measured:
* the Gaussian against scipy.ndimage.gaussian_filter in float64: |d| <= B = 3 (2 r + 3) 2^-53 max |V|: 2 r + 1 products and
  sums per pass with weights that sum to 1, three passes.  The device uses SciPy's taps, order of passes and order of
  operations with unfused products and sums, so the expected number of voxels that differ at all is 0; it is printed;
* the labels: the partition equals scipy.ndimage.label's under the 26-neighbourhood exactly, and the root array is the same
  from run to run;
* the mask: equal to the host's adaptive_mask (to the reference's recorded mask for the fixtures) in every voxel.  Before the
  device is called each case asserts on the CPU (tests/adaptive_mask_cases.py: check_margins) that no voxel of the host's
  low-passed map lies within 2 B of the threshold, no non-zero voxel within 2 B of an inner histogram edge, the values next to
  the mass rank and next to rank 1000 are more than 2 B apart, and that exactly 1000 voxels are >= v* or the all-ties rule
  gives the host's mask: under these a filter within B of SciPy's cannot change the mask.  Unfiltered maps need no margin;
* the context: supports equal to the host's masks, soft-masked curves bit for bit those after set_support(host mask).
Every test prints its figures (ADAPTIVE_FIGURE) before it asserts."""
import importlib

import numpy as np
import pytest

import adaptive_mask_cases as AC
import helicon_amd as H
from tests import test_gpu_true_fsc as TT

T = importlib.import_module("helicon_amd.true_fsc")

pytestmark = pytest.mark.gpu

GAUSS = [(shape, sigma, np.float64) for shape, sigma in AC.GAUSS_CASES] + [((8, 8, 300), 10.5, np.float64), ((20, 27, 33), 2.1, np.float32)]


@pytest.mark.parametrize("shape,sigma,dtype", GAUSS, ids=[f"{'x'.join(map(str, s))}-{g}-{np.dtype(d).name}" for s, g, d in GAUSS])
def test_gaussian_against_scipy(shape, sigma, dtype):
    from scipy.ndimage import gaussian_filter

    V = AC.volume(shape, 31).astype(dtype)
    want = gaussian_filter(V.astype(np.float64), sigma)
    got = H.gaussian_filter_device(V, sigma)
    B = AC.bound(sigma, V)
    err = float(np.abs(got - want).max())
    print(f"ADAPTIVE_FIGURE gaussian shape={shape} sigma={sigma} r={AC.radius(sigma)} dtype={np.dtype(dtype).name} bound={B:.3e} max_err={err:.3e} "
          f"not_bit_identical={int((got != want).sum())}")
    assert got.dtype == np.float64 and got.shape == V.shape
    assert err <= B
    assert np.array_equal(got, H.gaussian_filter_device(V, sigma))                     # run to run


_LABEL_CASES = AC.label_cases()


@pytest.mark.parametrize("name,S", _LABEL_CASES, ids=[c[0] for c in _LABEL_CASES])
def test_labels_equal_scipys_partition(name, S):
    want, n_want = AC.scipy_labels(S)
    got, n = H.label_components(S)
    same = np.array_equal(AC.canonical(got), AC.canonical(want))
    print(f"ADAPTIVE_FIGURE labels {name} shape={S.shape} foreground={int(S.sum())} components={n} scipy={n_want} partition_equal={same}")
    assert got.dtype == np.int32 and got.shape == S.shape and n == n_want
    assert np.array_equal(got == 0, S == 0)
    assert same
    assert np.array_equal(got, AC.canonical(got))                                      # numbered in order of the roots
    if name in ("corner", "edge", "checkerboard", "serpentine", "comb", "helix", "full", "single"):
        assert n == 1
    if name == "empty":
        assert n == 0 and not got.any()


def test_roots_are_the_smallest_index_and_the_same_from_run_to_run():
    import ctypes as C
    from helicon_amd import _lib

    S = dict(_LABEL_CASES)["bernoulli-0.12-70x66x130"]
    want, _ = AC.scipy_labels(S)
    roots = []
    for _ in range(2):
        r, n = np.empty(S.shape, np.int32), C.c_int64(0)
        _lib.check(_lib.lib().hh_am_label_3d(0, S.ctypes.data_as(C.POINTER(C.c_uint8)), *S.shape, r.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(n)), None)
        roots.append(r)
    assert np.array_equal(roots[0], roots[1])
    flat, lab = roots[0].ravel(), want.ravel()
    first = np.full(int(lab.max()) + 1, -1, dtype=np.int64)
    idx = np.flatnonzero(lab)
    first[lab[idx][::-1]] = idx[::-1]                                                  # the smallest flat index of every label
    assert np.array_equal(flat[idx], first[lab[idx]]) and (flat[lab == 0] == -1).all()


_FIXTURES = AC.fixture_cases()


@pytest.mark.parametrize("k,j,avg,apix,cutoff,mode,want", _FIXTURES, ids=[f"c{c[0]}-adaptive{c[1]}" for c in _FIXTURES])
def test_mask_equals_the_recorded_reference_mask(k, j, avg, apix, cutoff, mode, want):
    fig = AC.check_margins(avg, apix, cutoff, want, **mode)
    got, info = H.adaptive_mask_device(avg, apix, cutoff, info=True, **mode)
    print(f"ADAPTIVE_FIGURE fixture c{k} mode={j} B={fig['B']:.3e} margins={ {q: v for q, v in fig.items() if q != 'B'} } info={info} "
          f"threshold_equal={info['threshold'] == fig['threshold']} differing={int((got != want).sum())}")
    assert got.dtype == np.uint8 and np.array_equal(got, want)
    assert info["kept"] == int(want.sum()) and info["ties_at_v_star"] == (fig["n_ge"] > 1000) and not info["fallback"]


_SYNTHETIC = AC.synthetic_cases()


@pytest.mark.parametrize("name,V,apix,cutoff,mode", _SYNTHETIC, ids=[c[0] for c in _SYNTHETIC])
def test_mask_equals_the_hosts(name, V, apix, cutoff, mode):
    host = T.adaptive_mask(V, apix, cutoff, **mode)
    fig = AC.check_margins(V, apix, cutoff, host, **mode)
    got, info = H.adaptive_mask_device(V, apix, cutoff, info=True, **mode)
    print(f"ADAPTIVE_FIGURE synthetic {name} B={fig['B']:.3e} margins={ {q: v for q, v in fig.items() if q != 'B'} } info={info} "
          f"differing={int((got != host).sum())}")
    assert np.array_equal(got, host.astype(np.uint8))
    if name == "bright+dim-value":
        assert info["components"] >= 2 and info["kept"] < info["above"] and got[33, 33, 33] == 0
    if name == "two-blobs-fraction":
        assert info["components"] == 2 and info["kept"] == info["above"] and got[11, 12, 12] == 1 and got[29, 28, 29] == 1
    if name == "above-the-maximum":
        assert info["fallback"] and info["above"] == 0 and not got.any()
    else:
        assert not info["fallback"] and got.any()
    if name == "blob40-otsu":                                                         # a float32 volume is widened exactly
        V32 = V.astype(np.float32)
        host32 = T.adaptive_mask(V32.astype(np.float64), apix, cutoff, **mode)
        AC.check_margins(V32.astype(np.float64), apix, cutoff, host32, **mode)
        assert np.array_equal(H.adaptive_mask_device(V32, apix, cutoff, **mode), host32.astype(np.uint8))


def test_mask_refusals_on_the_device():
    V = AC.blob_noise((12, 12, 12), 3)
    with pytest.raises(ValueError, match="constant volume"):
        H.adaptive_mask_device(np.ones((10, 10, 10)), 1.0, 8.0)
    with pytest.raises(ValueError, match="at least 1000"):
        H.adaptive_mask_device(V[:6], 1.0, 8.0)
    # the library's own refusals, past the Python ones: a non-finite voxel and a constant volume are found on the device
    import ctypes as C
    from helicon_amd import _lib

    L = _lib.lib()
    out = np.zeros(V.shape, np.uint8)
    W = V.copy()
    W[1, 2, 3] = np.nan
    assert L.hh_am_mask_3d(0, W.ctypes.data_as(C.c_void_p), 1, 12, 12, 12, 0.0, None, 0, 0.0, out.ctypes.data_as(C.POINTER(C.c_uint8)), None) == -1
    assert b"NaN or infinite" in L.hh_last_error(None)
    W = np.full(V.shape, 2.5)
    assert L.hh_am_mask_3d(0, W.ctypes.data_as(C.c_void_p), 1, 12, 12, 12, 0.0, None, 0, 0.0, out.ctypes.data_as(C.POINTER(C.c_uint8)), None) == -1
    assert b"constant volume" in L.hh_last_error(None)
    assert H.adaptive_mask_device(V, 1.0, 8.0).any()                                   # and the device still works


@pytest.mark.parametrize("n", (24, 32))
def test_context_supports_equal_the_hosts_and_feed_the_soft_masks(n):
    a, b = TT._blob_pair(n, 4100 + n)
    rng = np.random.RandomState(n)
    u = tuple(rng.uniform(0, 2 * np.pi, size=(n, n, n // 2 + 1)) for _ in range(2))
    cutoff = TT._cutoff(n)
    a64, b64 = a.astype(np.float64), b.astype(np.float64)
    w = 3.1
    with H.TrueFSC(a, b, TT.APIX, cutoff, phases=u) as dev, H.TrueFSC(a, b, TT.APIX, cutoff, phases=u) as ref:
        for one_mask, mode in ((True, dict()), (False, dict()), (True, dict(mask_fraction_thresh=0.3)), (False, dict(mask_mass=30.0))):
            vols = [(a64 + b64) / 2] if one_mask else [a64, b64]
            hosts = [T.adaptive_mask(v, TT.APIX, cutoff, **mode) for v in vols]
            for v, h in zip(vols, hosts):
                AC.check_margins(v, TT.APIX, cutoff, h, **mode)
            info = dev.adaptive_support(one_mask=one_mask, **mode)
            got = [dev.support(k) for k in range(2)]
            print(f"ADAPTIVE_FIGURE context n={n} one_mask={one_mask} mode={mode} info={info} "
                  f"differing={[int((g != h).sum()) for g, h in zip(got, hosts)]}")
            assert len(info) == len(hosts)
            for k in range(2):
                assert got[k].dtype == np.uint8 and np.array_equal(got[k], hosts[k if not one_mask else 0].astype(np.uint8))
            ref.set_support(*hosts)
            for per_shell in (False, True):
                x, y = dev.soft_masked(w, per_shell), ref.soft_masked(w, per_shell)
                assert np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1])
            assert np.array_equal(dev.soft_mask(w, 1), ref.soft_mask(w, 1))


@pytest.mark.parametrize("n", (24, 32))
def test_true_fsc_with_device_support(n):
    a, b = TT._blob_pair(n, 4100 + n)
    rng = np.random.RandomState(41)
    u = tuple(rng.uniform(0, 2 * np.pi, size=(n, n, n // 2 + 1)) for _ in range(2))
    cutoff = TT._cutoff(n)
    for one_mask in (True, False):
        kw = dict(cutoff_res=cutoff, phases=u, one_mask=one_mask, mask_soft=6.2, device_masks=True)
        host = T.true_fsc(a, b, TT.APIX, **kw)
        dev = T.true_fsc(a, b, TT.APIX, device_support=True, **kw)
        print(f"ADAPTIVE_FIGURE true_fsc n={n} one_mask={one_mask} host_mask_s device={dev['host_mask_s']} host={host['host_mask_s']:.4f}")
        assert dev["host_mask_s"] == 0.0 and host["host_mask_s"] > 0
        for key in ("unmasked", "randomized_unmasked", "masked", "randomized_masked", "true", "true_fit"):
            assert np.array_equal(dev[key], host[key]), key
        assert np.array_equal(dev["mask1"], host["mask1"]) and np.array_equal(dev["mask2"], host["mask2"])
        assert (dev["mask1"] is dev["mask2"]) == one_mask and dev["resolution"] == host["resolution"]
