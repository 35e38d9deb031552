"""The image alignment's float64 yardstick (tests/align_cases.py) checked against itself, the GPU cases' fitness for the
comparison (no bin of a cross-power spectrum near the clamp, few candidates left out by the two exclusion rules), the host
side of helicon_amd.align and the entry points of the built library.  No GPU."""
import re
from pathlib import Path

import numpy as np
import pytest

import align_cases as Y
from helicon_amd import _lib
from helicon_amd import align as A

ROOT = Path(__file__).resolve().parent.parent
ENTRY_POINTS = {"hh_align_chunk", "hh_align_create", "hh_align_destroy", "hh_align_eval", "hh_align_correlation", "hh_align_warp_wrap",
                "hh_align_profile"}


def test_entry_points_in_header_exports_and_library():
    hdr = (ROOT / "include" / "helicon_hip.h").read_text()
    declared = set(re.findall(r"^\s*int\s+(hh_align_\w+)\s*\(", hdr, flags=re.M))
    assert declared == ENTRY_POINTS and ENTRY_POINTS <= set(_lib.EXPORTS)
    L = _lib.lib()
    for name in ENTRY_POINTS:
        assert hasattr(L, name)
    text = (ROOT / "helicon_amd" / "csrc" / "align.inc").read_text()
    assert set(re.findall(r'^extern "C" int (hh_\w+)\(', text, re.M)) == ENTRY_POINTS
    assert 'include "align.inc"' in (ROOT / "helicon_amd" / "csrc" / "helicon_hip.hip").read_text()
    assert L.hh_align_chunk() >= 1 and A.chunk() == L.hh_align_chunk()


def test_package_exports():
    import helicon_amd as H

    assert H.align_images is A.align_images and H.align_images_grid is A.align_images_grid and H.AlignContext is A.AlignContext


@pytest.mark.parametrize("shape", [(12, 15), (14, 16), (15, 12)])
def test_circular_shift_is_recovered_and_wrap_equals_roll(shape):
    """For a shift s in {-1, n // 2, n // 2 + 1} per axis: the moving image rolled by -s is registered by s (by s - n beyond
    the midpoint: the sign convention for even and odd sides), and the wrap warp by an integer shift is np.roll, bit for bit."""
    rng = np.random.default_rng(3)
    a = rng.standard_normal(shape)
    ny, nx = shape
    for sy in (-1, ny // 2, ny // 2 + 1):
        for sx in (-1, nx // 2, nx // 2 + 1):
            b = np.roll(a, (-sy, -sx), axis=(0, 1))
            _, c = Y.cross_power(a, b)
            want = (sy - ny if sy > ny // 2 else sy, sx - nx if sx > nx // 2 else sx)
            assert Y.shift_of(c) == want
            w = Y.warp_wrap(b, Y.shifted(np.eye(3), want))
            assert np.array_equal(w, np.roll(b, want, axis=(0, 1))) and np.array_equal(w, a)


def test_wrap_rule_mixes_last_and_first_column():
    img = np.arange(12, dtype=np.float64).reshape(3, 4)
    h = np.eye(3)
    h[0, 2] = 0.25          # samples column x + 0.25: the last output column lies between column 3 and column 4 = column 0
    w = Y.warp_wrap(img, h)
    assert np.allclose(w[:, 3], 0.75 * img[:, 3] + 0.25 * img[:, 0]) and np.allclose(w[:, 0], 0.75 * img[:, 0] + 0.25 * img[:, 1])
    assert list(Y.coord_map(np.array([-5, -4, -1, 0, 3, 4, 9]), 4)) == [3, 0, 3, 0, 3, 0, 1]


def test_taper_has_no_vanishing_positive_value():
    for ref_shape, mov_shape in Y.CASES:
        for n in set(ref_shape + mov_shape):
            t = Y.taper_profile(n)     # (a side whose n // 2 is a multiple of 10 can put a sample at the slope's very end)
            assert t[t > 0].min() > 1e-3
            assert np.array_equal(t, A.taper_profile(n, 0.8, 0.1))
        assert np.array_equal(Y.tapering_filter(mov_shape), A.generate_tapering_filter(mov_shape))


def test_inverse_matrices_match_the_yardstick():
    for shape in ((33, 47), (48, 64)):
        got = A.inverse_matrices(shape, [1.0, 0.97, 1.06], [0.0, -31.0, 187.0])
        for row, (s, a) in zip(got, [(1.0, 0.0), (0.97, -31.0), (1.06, 187.0)]):
            assert np.allclose(row, Y.inverse_matrix(shape, s, a)[:2].ravel(), rtol=1e-14, atol=1e-12)
    assert np.array_equal(A.inverse_matrices((33, 47), 1.0, 0.0)[0], [1, 0, 0, 0, 1, 0])


@pytest.mark.parametrize("case", range(len(Y.CASES)))
def test_cases_are_fit_for_the_comparison(case):
    """Every bin of every candidate's cross-power spectrum is at least 1e4 times the clamp, and the yardstick alone leaves out
    at most 5 % of the case's candidates by each exclusion rule."""
    yard = Y.case_yardstick(case)
    assert len(yard) == 13 * 4 * 2 * 2
    assert min(e["min_power"] for e in yard) >= 1e4 * Y.CLAMP
    close = sum(e["gap"] <= 4 * Y.TOL_SURFACE for e in yard) / len(yard)
    borderline = sum(e["borderline"] > 0 for e in yard) / len(yard)
    print(f"case {Y.CASES[case]}: gap <= {4 * Y.TOL_SURFACE:.3g} in {close:.3%}, borderline in {borderline:.3%}")
    assert close <= Y.MAX_EXCLUDED and borderline <= Y.MAX_EXCLUDED
    assert not any(np.isnan(e["score"]) for e in yard)


def test_float32_and_float64_agree_on_the_shift():
    ref_work, work, taper, _ = Y.case_planes(0)
    for s, a, pl in Y.candidates()[::9]:
        w = Y.P.warp_affine(work[pl], Y.inverse_matrix(ref_work.shape, s, a))          # float32 planes: float32 arithmetic
        p = np.fft.fft2(ref_work).astype(np.complex64) * np.conj(np.fft.fft2(w).astype(np.complex64))
        c32 = np.fft.ifft2(p / np.maximum(np.abs(p), np.float32(Y.CLAMP)))
        e = Y.evaluate(ref_work, work[pl], taper[pl], s, a)
        if e["gap"] > 4 * Y.TOL_SURFACE:
            assert Y.shift_of(c32) == e["shift"]


def test_yardstick_align_images_scores_what_it_returns():
    ref, mov = Y.make_pair((33, 47), (33, 47))
    for kw in (dict(scale_range=0, angle_range=20), dict(scale_range=0, angle_range=0)):
        (flip, scale, angle, shift, score), trace = Y.align_images(mov, ref, check_polarity=False, **kw)
        ref_work, work, taper, _ = Y.prepare(ref, mov[::-1, :] if flip else mov)
        if kw["angle_range"]:
            e = Y.evaluate(ref_work, work, taper, scale, angle)
            assert e["score"] == score and e["shift"] == tuple(shift) and len(trace) > 4
            assert score == max(t[3]["score"] for t in trace if t[2] == flip)
        else:
            assert (scale, angle, shift) == (1, 0, 0) and not trace


def test_planted_pair_scores_highest_at_the_planted_transform():
    q = Y.PLANTED
    ref, mov = Y.make_pair((48, 64), (48, 64), planted=True)
    ref_work, work, taper, _ = Y.prepare(ref, mov[::-1, :])
    e = Y.evaluate(ref_work, work, taper, q["scale"], q["angle"])
    assert e["shift"] == q["shift"] and e["score"] > 0.6
    assert Y.evaluate(ref_work, work, taper, q["scale"], q["angle"] + 20)["score"] < e["score"] - 0.2


def test_command_line_report(tmp_path):
    ref, mov = Y.make_pair((33, 47), (33, 47))
    np.save(tmp_path / "ref.npy", ref)
    np.save(tmp_path / "mov.npy", mov)
    seen = {}

    def grid_fn(m, r, scales, angles, **kw):
        seen.update(scales=scales, angles=angles, kw=kw)
        return A.AlignBest(True, 1.01, -3.0, np.array([1.0, -2.0]), 0.5), np.zeros((2, 2, len(scales), len(angles)))

    args = A.add_args(__import__("argparse").ArgumentParser()).parse_args(
        [str(tmp_path / "mov.npy"), str(tmp_path / "ref.npy"), "--angle-range", "4", "--angle-step", "2", "--scale-range", "0.02", "--scale-step", "0.01"])
    rep = A.run(args, grid_fn)
    assert np.allclose(seen["angles"], [-4, -2, 0, 2, 4]) and np.allclose(seen["scales"], [0.98, 0.99, 1.0, 1.01, 1.02])
    assert seen["kw"] == dict(check_polarity=True, check_flip=True, refine=False, device=0)
    assert rep["candidates"] == 2 * 2 * 5 * 5 and rep["best"] == dict(flip=True, scale=1.01, angle=-3.0, shift=[1.0, -2.0], score=0.5)
