"""Host side of the Fourier resampling (no GPU): the float64 oracle against np.fft and the reference's fixtures, the
package's operator builders against the oracle, argument validation, and ``symmetry_search --resample`` with a stub
engine and a stub resampler."""
import argparse
import json
import re
from pathlib import Path

import numpy as np
import pytest

import fft_resample_oracle as O
import helicon_amd as H
from helicon_amd import _lib
from helicon_amd import symmetry_search as SS
from test_symmetry_search_host import StubEngine

ROOT = Path(__file__).resolve().parents[1]


def rel(got, want):
    return float(np.abs(np.asarray(got) - np.asarray(want)).max() / np.abs(want).max())


def apply(ops, x):
    """The three (or two) operators on x with einsum, float64."""
    x = np.asarray(x, dtype=np.float64).astype(np.complex128)
    if x.ndim == 2:
        return np.einsum("bj,ck,jk->bc", *ops, x, optimize=True)
    return np.einsum("ai,bj,ck,ijk->abc", *ops, x, optimize=True)


def test_entry_point_in_header_exports_and_library():
    hdr = (ROOT / "include" / "helicon_hip.h").read_text()
    declared = set(re.findall(r"^\s*int\s+(hh_separable_transform\w*)\s*\(", hdr, flags=re.M))
    assert declared == {"hh_separable_transform_3d", "hh_separable_transform_kernel_ms"} <= set(_lib.EXPORTS)
    for where in ("lib/transforms.py:714-743", "610-660", "plugins/proc3d/fft_resample.py:97-109"):
        assert where in hdr
    L = _lib.lib()   # loads the library and binds every export; no GPU call
    assert L.hh_separable_transform_3d(0, None, None, None, None, None, 0, 1.0, None, None) == -1
    assert b"hh_separable_transform_3d" in L.hh_last_error(None)
    assert 'fourier_resample.inc"' in (ROOT / "helicon_amd" / "csrc" / "helicon_hip.hip").read_text()


def test_entry_point_argument_errors_and_the_call_without_a_pass():
    """What hh_separable_transform_3d decides on the host: its argument errors, and a call in which no axis has an operator,
    which is the epilogue of the input itself and launches nothing."""
    import ctypes as C

    L = _lib.lib()
    f32p = C.POINTER(C.c_float)
    ptr = lambda a: a.ctypes.data_as(f32p)   # noqa: E731
    x = np.arange(-12, 12, dtype=np.float32).reshape(2, 3, 4)
    out0, out1 = np.empty_like(x), np.empty_like(x)
    op = np.ones((5, 4), np.float32)
    shape, none = (C.c_int32 * 3)(2, 3, 4), (f32p * 3)()

    def call(in_shape=shape, out_shape=shape, op_re=none, op_im=none, epilogue=2, o0=out0, o1=out1):
        return L.hh_separable_transform_3d(0, ptr(x), in_shape, out_shape, op_re, op_im, epilogue, 0.5, ptr(o0), None if o1 is None else ptr(o1))

    for bad in (dict(epilogue=3), dict(epilogue=-1), dict(epilogue=0, o1=None), dict(out_shape=(C.c_int32 * 3)(2, 3, 5)),
                dict(in_shape=(C.c_int32 * 3)(0, 3, 4)), dict(out_shape=(C.c_int32 * 3)(2, 3, 1025), op_re=(f32p * 3)(None, None, ptr(op))),
                dict(out_shape=(C.c_int32 * 3)(2, 3, 5), op_im=(f32p * 3)(None, None, ptr(op)))):
        assert call(**bad) == -1, bad
        assert L.hh_last_error(None).startswith(b"hh_separable_transform_3d: ")
    assert call(epilogue=2) == 0 and np.array_equal(out0, 0.5 * x)
    assert call(epilogue=1) == 0 and np.array_equal(out0, 0.5 * np.abs(x))
    assert call(epilogue=0) == 0 and np.array_equal(out0, x) and not out1.any()
    got, apix = H.fft_resample(x.reshape(2, 2, 6), 1.7, (2, 2, 6), output="real")     # even sides, same size: no pass
    assert apix == 1.7 and np.array_equal(got, x.reshape(2, 2, 6))
    ms = C.c_double(-1.0)
    assert L.hh_separable_transform_kernel_ms(C.byref(ms)) == 0 and ms.value == 0.0
    assert L.hh_separable_transform_kernel_ms(None) == -1


@pytest.mark.parametrize("shape", [(8, 10, 12), (6, 6, 6), (2, 4, 16)])
def test_oracle_rescale_with_default_arguments_is_fftn_on_even_sides(shape):
    x = O.blob_volume(shape, seed=1)
    assert rel(O.fft_rescale_3d(x), np.fft.fftn(x.astype(np.float64))) <= 1e-12
    assert rel(O.fft_rescale_3d(x, apix=1.7), np.fft.fftn(x.astype(np.float64))) <= 1e-12


def test_oracle_rescale_keeps_a_phase_factor_on_an_odd_side():
    x = O.blob_volume((7, 8, 8), seed=2)
    assert rel(O.fft_rescale_3d(x), np.fft.fftn(x.astype(np.float64))) > 1e-3


def test_oracle_resample_is_fourier_cropping_and_padding_on_even_sides():
    x = O.blob_volume((12, 12, 12), seed=3).astype(np.float64)
    spec = np.fft.fftshift(np.fft.fftn(x))
    down, apix = O.fft_resample(x, 1.5, (8, 8, 8), output="real")
    assert apix == 2.25
    cropped = np.fft.ifftshift(spec[2:10, 2:10, 2:10])
    assert rel(down, np.fft.ifftn(cropped).real * (8 / 12) ** 3) <= 1e-12
    same, _ = O.fft_resample(x, 1.5, (12, 12, 12), output="real")
    assert rel(same, x) <= 1e-12
    ab, _ = O.fft_resample(x, 1.5, (8, 8, 8))
    assert (ab >= 0).all() and rel(ab, np.abs(np.fft.ifftn(cropped)) * (8 / 12) ** 3) <= 1e-12


def test_oracle_crop_equals_the_reference_2d_fixtures(golden_dir):
    g = np.load(golden_dir / "g23_fft_crop.npz")
    assert int(g["n_cases"][0]) == 4 and set(json.loads(str(g["versions"]))) == {"helicon", "numpy", "scipy", "python"}
    seen = []
    for k in range(3):
        x, size, want = g[f"case{k}_in"], tuple(int(v) for v in g[f"case{k}_size"]), g[f"case{k}_out"]
        seen.append((x.shape, size))
        got = O.fft_crop(x, size)
        assert got.shape == want.shape == tuple(2 * (v // 2) for v in size)
        assert rel(got, want) <= 1e-12
    assert seen == O.CROP_CASES_2D
    x = g["case0_in"]
    assert O.fft_crop(x, x.shape) is x and O.fft_crop(x) is x


def test_the_reference_3d_crop_is_irfft2_not_irfftn(golden_dir):
    """The deviation helicon_amd.fft_crop makes on purpose: the reference leaves z untransformed."""
    g = np.load(golden_dir / "g23_fft_crop.npz")
    x, size, ref = g["case3_in"], tuple(int(v) for v in g["case3_size"]), g["case3_out"]
    assert x.shape == (12, 12, 12) and size == (8, 8, 8)
    assert rel(O.fft_crop_3d_as_reference(x, size), ref) <= 1e-12
    assert float(np.abs(O.fft_crop(x, size) - ref).max()) > 1.0
    # and irfftn is the map: cropping a band-limited map keeps it (up to the grid)
    spec = np.fft.fftn(O.blob_volume((8, 8, 8), 5).astype(np.float64))
    spec[4], spec[:, 4], spec[:, :, 4] = 0, 0, 0          # without the Nyquist planes the round trip is exact
    lo = np.fft.ifftn(spec).real
    up, _ = O.fft_resample(lo, 1.0, (12, 12, 12), output="real")
    assert up.shape == (12, 12, 12) and rel(O.fft_crop(up, (8, 8, 8)) * (8 / 12) ** 3, lo) <= 1e-12


@pytest.mark.parametrize("shape,size", O.CASES, ids=[f"{a}-{b}".replace(" ", "") for a, b in O.CASES])
def test_builders_against_the_oracle(shape, size):
    from helicon_amd.fft_resample import crop_operator, resample_operator, rescale_operator

    x = O.blob_volume(shape, seed=sum(shape))
    apix = 1.3
    # fft_resample: abs and real
    ops = [H.resample_operator(n, on) for n, on in zip(shape, size)]
    assert H.resample_operator is resample_operator and ops[0].shape == (size[0], shape[0]) and ops[0].dtype == np.complex128
    c = apply(ops, x) * (np.prod(size) / np.prod(shape))
    for kind, got in (("abs", np.abs(c)), ("real", c.real)):
        want, new_apix = O.fft_resample(x, apix, size, output=kind)
        assert rel(got, want) <= 1e-12, kind
        assert new_apix == round(apix * shape[2] / size[2], 4)
    # fft_rescale at the GPU test's cutoffs, and at the defaults
    cut = O.rescale_cutoffs(shape, size, apix)
    ops = [rescale_operator(n, on, apix, cr) for n, on, cr in zip(shape, size, cut)]
    assert rel(apply(ops, x), O.fft_rescale_3d(x, apix, cut, size)) <= 1e-12
    ops = [H.rescale_operator(n, n) for n in shape]
    assert rel(apply(ops, x), O.fft_rescale_3d(x)) <= 1e-12
    # fft_crop wherever the case shrinks every side
    if all(on <= n for n, on in zip(shape, size)):
        ops = [crop_operator(n, on, ax == 2) for ax, (n, on) in enumerate(zip(shape, size))]
        want = O.fft_crop(x.astype(np.float64), size)
        got = apply(ops, x)
        assert got.shape == want.shape and rel(got.real, want) <= 1e-12


@pytest.mark.parametrize("shape,size", O.CROP_CASES_3D + O.CROP_CASES_2D + [((24, 20), (24, 12))])
def test_crop_builder_against_the_oracle(shape, size):
    x = O.blob_volume(shape, seed=7)
    ops = [H.crop_operator(n, on, ax == len(shape) - 1) for ax, (n, on) in enumerate(zip(shape, size))]
    want = O.fft_crop(x.astype(np.float64), size)
    assert rel(apply(ops, x).real, want) <= 1e-12
    for mine, theirs in zip(ops, O.crop_ops(shape, size)):
        assert rel(mine, theirs) <= 1e-12


def test_oracle_operator_forms_agree_with_its_functions():
    """The per-axis forms the float32 floor is computed from are the functions' own, in float64."""
    shape, size = (15, 18, 21), (9, 12, 14)
    x = O.blob_volume(shape, seed=4)
    want, _ = O.fft_resample(x, 1.0, size, output="real")
    assert rel(apply(O.resample_ops(shape, size), x).real * (np.prod(size) / np.prod(shape)), want) <= 1e-12
    floor = O.float32_passes(x, O.resample_ops(shape, size), "real", np.prod(size) / np.prod(shape))
    assert floor.dtype == np.float32 and rel(floor, want) < 2e-6


def test_identity_operators():
    from helicon_amd.fft_resample import _is_identity

    assert _is_identity(H.resample_operator(40, 40)) and _is_identity(H.resample_operator(1, 1))
    assert _is_identity(H.rescale_operator(1, 1)) and _is_identity(H.crop_operator(24, 24, False))
    assert not _is_identity(H.resample_operator(15, 15))     # an odd side keeps a phase factor
    assert not _is_identity(H.resample_operator(40, 72)) and not _is_identity(H.rescale_operator(8, 8))


def test_argument_validation_comes_before_the_library(monkeypatch):
    def no_library():
        raise AssertionError("the library was touched")

    monkeypatch.setattr(_lib, "lib", no_library)
    vol, img = np.zeros((8, 8, 8), np.float32), np.zeros((8, 8), np.float32)
    for bad in (lambda: H.fft_resample(vol, 1.0, (4, 4, 4), output="imag"),
                lambda: H.fft_resample(img, 1.0, (4, 4)),                      # ndim
                lambda: H.fft_resample(vol, 1.0, (4, 4)),                      # one side per axis
                lambda: H.fft_resample(vol, 1.0, (4, 4, 0)),                   # side
                lambda: H.fft_resample(vol, 1.0, (4, 4, 1025)),
                lambda: H.fft_resample(vol, 0.0, (4, 4, 4)),
                lambda: H.fft_resample(vol.astype(np.complex64), 1.0, (4, 4, 4)),
                lambda: H.fft_resample(np.zeros((2, 2, 1025), np.float32), 1.0, (2, 2, 2)),
                lambda: H.fft_rescale(np.zeros(8, np.float32)),
                lambda: H.fft_rescale(vol, output_size=(4, 4)),
                lambda: H.fft_rescale(vol, cutoff_res=(2.0, 2.0)),
                lambda: H.fft_rescale(vol, cutoff_res=(2.0, 2.0, -1.0)),
                lambda: H.fft_rescale(img, output_size=(4.5, 4)),
                lambda: H.fft_crop(np.zeros((2, 2, 2, 2), np.float32), (1, 1, 1, 1)),
                lambda: H.fft_crop(vol, (4, 4)),
                lambda: H.fft_crop(vol, (4, 4, 9)),                            # larger than the input
                lambda: H.fft_crop(vol, (4, 4, 1)),
                lambda: H.crop_operator(8, 9, True),
                lambda: H.rescale_operator(8, 8, 1.0, 0.0),
                lambda: H.resample_operator(0, 8)):
        with pytest.raises(ValueError):
            bad()
    assert H.fft_crop(vol) is vol and H.fft_crop(vol, (8, 8, 8)) is vol and H.fft_crop(img, (8, 8)) is img


# ------------------------------------------------------------------------------------------
# symmetry_search --resample
# ------------------------------------------------------------------------------------------
def _args(argv):
    return SS.add_args(argparse.ArgumentParser()).parse_args(argv)


def test_symmetry_search_resample_with_a_stub_engine_and_resampler(tmp_path):
    from helicon_amd.mrc import write_mrc

    vol = np.random.default_rng(0).random((64, 48, 48)).astype(np.float32)
    write_mrc(tmp_path / "m.mrc", vol, 1.0)
    made, calls = [], []

    def factory(data, apix, **kw):
        made.append(StubEngine(data, apix, **kw))
        return made[-1]

    def resampler(data, apix, new_size, *, output, device):
        calls.append((tuple(data.shape), apix, tuple(new_size), output, device))
        return np.ascontiguousarray(data[::2, ::2, ::2]), round(apix * data.shape[2] / new_size[2], 4)

    common = [str(tmp_path / "m.mrc"), "--twist", "26", "32", "1", "--rise", "4.5", "7.5", "0.5"]
    assert _args(common).resample is None
    plain = SS.run(_args(common), engine_factory=factory, resampler=resampler)
    assert calls == [] and made[-1].shape == (64, 48, 48) and made[-1].apix == 1.0
    assert plain["map"] == dict(path=str(tmp_path / "m.mrc"), shape=[64, 48, 48], apix=1.0)     # what it was
    rep = SS.run(_args([*common, "--resample", "32", "24", "24"]), engine_factory=factory, resampler=resampler)
    json.dumps(rep)
    assert calls == [((64, 48, 48), 1.0, (32, 24, 24), "real", 0)]
    assert made[-1].shape == (32, 24, 24) and made[-1].apix == 2.0 and made[-1].closed
    assert rep["map"] == dict(path=str(tmp_path / "m.mrc"), shape=[32, 24, 24], apix=2.0,
                              resampled_from=dict(shape=[64, 48, 48], apix=1.0))
    assert rep["region"] == dict(rmin=0.0, rmax=11.0, z_fraction=0.5, k_range=[8, 24])          # of the new map
    assert set(rep) == set(plain)
    with pytest.raises(SystemExit, match="even"):
        SS.run(_args([*common, "--resample", "32", "24", "25"]), engine_factory=factory, resampler=resampler)
    with pytest.raises(SystemExit, match="ratios"):
        SS.run(_args([*common, "--resample", "32", "24", "32"]), engine_factory=factory, resampler=resampler)
    with pytest.raises(SystemExit, match="positive"):
        SS.run(_args([*common, "--resample", "32", "24", "0"]), engine_factory=factory, resampler=resampler)
    np.save(tmp_path / "odd.npy", np.zeros((15, 16, 16), np.float32))
    with pytest.raises(SystemExit, match="even"):
        SS.run(_args([str(tmp_path / "odd.npy"), "--apix", "1", *common[1:], "--resample", "8", "8", "8"]), engine_factory=factory,
               resampler=resampler)
    assert len(calls) == 1


def test_module_command_line_arguments():
    from helicon_amd.fft_resample import add_args

    a = add_args(argparse.ArgumentParser()).parse_args(["in.mrc", "out.mrc", "--size", "16", "16", "16"])
    assert (a.input, a.output, a.size, a.kind, a.apix, a.device) == ("in.mrc", "out.mrc", [16, 16, 16], "abs", None, 0)
    a = add_args(argparse.ArgumentParser()).parse_args(["in.mrc", "out.mrc", "--size", "8", "8", "8", "--output", "real", "--apix", "2"])
    assert (a.kind, a.apix) == ("real", 2.0)
    with pytest.raises(SystemExit):
        add_args(argparse.ArgumentParser()).parse_args(["in.mrc", "out.mrc"])
