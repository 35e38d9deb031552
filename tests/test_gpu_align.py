"""Batched image alignment on the device (helicon_amd/align.py, csrc/align.inc) against the float64 yardstick of
tests/align_cases.py.  Five shapes (odd sides; odd asymmetric padding; exactly one tile; just past a tile seam on both axes;
past two tiles in x), 13 angles x 4 scales x 2 polarities on two planes each.  The two bounds (TOL_SURFACE, TOL_SCORE) are four
times the largest differences measured on an MI355X (profiles/align.json); every test prints its figure before it asserts."""
import functools

import numpy as np
import pytest

import align_cases as Y
from helicon_amd import align as A
from helicon_amd.align import AlignContext, align_images, align_images_grid

pytestmark = pytest.mark.gpu

CASE_IDS = ["x".join(map(str, r)) + "_" + "x".join(map(str, m)) for r, m in Y.CASES]


@functools.lru_cache(maxsize=None)
def device_case(case):
    """The device's evaluation of every candidate of a case, computed once."""
    ref_work, work, taper, _ = Y.case_planes(case)
    sc, an, pl = (np.array(v) for v in zip(*Y.candidates()))
    with AlignContext.from_planes(ref_work, work, taper) as ctx:
        return ctx.evaluate(sc, an, pl)


def compare(dev, yard, label, max_excluded=Y.MAX_EXCLUDED):
    """Checks (b) and (c) on parallel lists of device results and yardstick evaluations.  ``max_excluded=None``: the shares left
    out are printed but not bounded — an optimiser's trace starts on the integer lattice (scale 1, angle 0 or 180: every
    pixel's neighbour weights are 0 or 1) and gathers where the shift jumps, so most of its points can be borderline."""
    n = len(yard)
    decided = np.array([e["gap"] > 4 * Y.TOL_SURFACE for e in yard])
    agree = np.array([tuple(int(v) for v in dev.shifts[i]) == tuple(e["shift"]) for i, e in enumerate(yard)])
    clean = agree & np.array([e["borderline"] == 0 for e in yard])
    dscore = np.abs(dev.scores - np.array([e["score"] for e in yard]))
    nm = np.array([e["nmask"] for e in yard])
    worst = float(dscore[clean].max()) if clean.any() else 0.0
    print(f"{label}: {n} candidates, shift left out {1 - decided.mean():.3%}, differs on {np.count_nonzero(decided & ~agree)} decided; "
          f"score left out {1 - clean.mean():.3%}, max |dscore| = {worst:.3e} (bound {Y.TOL_SCORE:.3e}), "
          f"mask counts differ on {np.count_nonzero(clean & (dev.nmask != nm))}")
    if max_excluded is not None:
        assert 1 - decided.mean() <= max_excluded and 1 - clean.mean() <= max_excluded
    assert not (decided & ~agree).any()
    assert np.array_equal(dev.nmask[clean], nm[clean])
    assert worst <= Y.TOL_SCORE
    return decided, clean


@pytest.mark.parametrize("case", range(len(Y.CASES)), ids=CASE_IDS)
def test_correlation_surface(case):
    """(a) the surface c of every candidate, relative to the yardstick's peak; the peak value evaluate() reports is that
    surface's maximum."""
    ref_work, work, taper, _ = Y.case_planes(case)
    yard, dev = Y.case_yardstick(case), device_case(case)
    worst = 0.0
    with AlignContext.from_planes(ref_work, work, taper) as ctx:
        for i, ((s, a, pl), e) in enumerate(zip(Y.candidates(), yard)):
            c = ctx.correlation(s, a, pl)
            assert c.dtype == np.float32 and c.shape == ref_work.shape
            assert np.abs(c).max() == dev.peaks[i]
            worst = max(worst, float(np.abs(c.astype(np.float64) - e["surface"]).max() / e["peak"]))
    print(f"{CASE_IDS[case]}: max |c - yardstick| / peak = {worst:.3e} (bound {Y.TOL_SURFACE:.3e})")
    assert worst <= Y.TOL_SURFACE


@pytest.mark.parametrize("case", range(len(Y.CASES)), ids=CASE_IDS)
def test_shifts_mask_counts_and_scores(case):
    """(b), (c)"""
    compare(device_case(case), Y.case_yardstick(case), CASE_IDS[case])


@pytest.mark.parametrize("case", [0, 1], ids=CASE_IDS[:2])
def test_context_prepares_the_planes_as_the_reference(case):
    ref, mov = Y.make_pair(*Y.CASES[case])
    ref_work, work, taper, padded = Y.case_planes(case)
    with AlignContext(ref, [mov, mov[::-1, :]]) as ctx:
        assert np.array_equal(ctx.ref_work, ref_work) and np.array_equal(ctx.moving_work, work)
        assert np.array_equal(ctx.taper, taper) and np.array_equal(ctx.padded, padded)
        got = ctx.evaluate(Y.SCALES[2], Y.ANGLES[4], [0, 1])
    dev = device_case(case)
    at = [Y.candidates().index((Y.SCALES[2], Y.ANGLES[4], pl)) for pl in (0, 1)]
    assert np.array_equal(got.shifts, dev.shifts[at]) and np.array_equal(got.scores, dev.scores[at])


@pytest.mark.parametrize("case", [0, 1, 4], ids=[CASE_IDS[k] for k in (0, 1, 4)])
def test_aligned_with_an_integer_shift_is_roll(case):
    """(d) bit for bit, for the three resident planes and a caller's plane, shifts inside and beyond a side"""
    ref, mov = Y.make_pair(*Y.CASES[case])
    ny, nx = ref.shape
    other = np.random.default_rng(5).standard_normal(ref.shape).astype(np.float32)
    with AlignContext(ref, [mov, mov[::-1, :]]) as ctx:
        for shift in ((0, 0), (1, 0), (0, -1), (-3, 5), (ny // 2 + 1, -(nx // 2) - 1), (ny + 2, -nx - 3)):
            for m in (0, 1):
                for which, src in (("image", ctx.padded[m]), ("work", ctx.moving_work[m]), ("taper", ctx.taper[m]), (other, other)):
                    got = ctx.aligned(1, 0, shift, m, which)
                    assert got.dtype == np.float32 and np.array_equal(got, np.roll(src, shift, axis=(0, 1))), (shift, m)
    print(f"{CASE_IDS[case]}: aligned(1, 0, integer shift) == np.roll on 6 shifts x 2 planes x 4 sources")


def test_aligned_matches_the_yardstick_wrap_warp():
    ref, mov = Y.make_pair(*Y.CASES[1])
    with AlignContext(ref, [mov]) as ctx:
        got = ctx.aligned(1.03, 187.0, (3, -5), 0, "image")
        want = Y.aligned(ctx.padded[0], 1.03, 187.0, (3, -5))
    err = float(np.abs(got - want).max() / np.abs(want).max())
    print(f"wrap warp: max |device - yardstick| / max = {err:.3e}")
    assert err <= 1e-4     # float32 coordinates of magnitude < 2^7 (ulp 8e-6) on an image whose pixel-to-pixel change is its range


@pytest.mark.parametrize("shape", [(16, 24), (15, 23), (64, 66), (65, 31)])
def test_engineered_circular_shifts(shape):
    """(e) a circular shift of the reference by -1, n // 2, n // 2 + 1 per axis returns exactly that shift, score 1 to 1e-12"""
    ny, nx = shape
    ref = np.random.default_rng(9).standard_normal(shape).astype(np.float32)
    shifts = [(sy, sx) for sy in (-1, ny // 2, ny // 2 + 1) for sx in (-1, nx // 2, nx // 2 + 1)]
    moving = np.stack([np.roll(ref, (-sy, -sx), axis=(0, 1)) for sy, sx in shifts])
    with AlignContext.from_planes(ref, moving, np.ones_like(moving)) as ctx:
        r = ctx.evaluate(1.0, 0.0, np.arange(len(shifts)))
    want = np.array([(sy - ny if sy > ny // 2 else sy, sx - nx if sx > nx // 2 else sx) for sy, sx in shifts])
    print(f"{shape}: shifts {r.shifts.tolist()}, max |score - 1| = {np.abs(r.scores - 1).max():.3e}, min peak {r.peaks.min():.6f}")
    assert np.array_equal(r.shifts, want)
    assert np.abs(r.scores - 1).max() <= 1e-12 and (r.nmask == ny * nx).all()


def test_zero_plane_in_a_batch():
    """(f)"""
    ref_work, work, taper, _ = Y.case_planes(0)
    planes = np.stack([work[0], np.zeros_like(work[0]), work[1]])
    tapers = np.stack([taper[0], taper[0], taper[1]])
    with AlignContext.from_planes(ref_work, planes, tapers) as ctx:
        r = ctx.evaluate([1.0, 1.03, 1.0, 0.97, 1.0], [0.0, 14.0, -6.0, 9.0, 180.0], [0, 1, 2, 1, 0])
    print(f"zero plane: shifts {r.shifts.tolist()}, scores {r.scores.tolist()}, peaks {r.peaks.tolist()}")
    for i in (1, 3):
        assert tuple(r.shifts[i]) == (0, 0) and r.scores[i] == 0 and r.peaks[i] == 0
    assert np.isfinite(r.scores).all() and (r.scores[[0, 2, 4]] != 0).all()


def test_chunk_seam_and_batch_independence():
    """(g) hh_align_chunk() + 1 candidates at (16, 24), bit for bit the same singly, and in another order"""
    n = A.chunk() + 1
    ref, mov = Y.make_pair((16, 24), (16, 24))
    rng = np.random.default_rng(2)
    sc, an, pl = rng.uniform(0.95, 1.05, n), rng.uniform(-180, 180, n), rng.integers(0, 2, n)
    with AlignContext(ref, [mov, mov[::-1, :]]) as ctx:
        batch = ctx.evaluate(sc, an, pl)
        order = rng.permutation(n)
        mixed = ctx.evaluate(sc[order], an[order], pl[order])
        single = [ctx.evaluate(sc[i], an[i], pl[i]) for i in range(n)]
    for k, name in enumerate(A.AlignEval._fields):
        one = np.concatenate([s[k] for s in single])
        assert np.array_equal(batch[k], one, equal_nan=True), name
        assert np.array_equal(batch[k][order], mixed[k], equal_nan=True), name
    print(f"{n} candidates: the batch, a permutation of it and {n} single evaluations are bit-identical")


def test_two_runs_are_identical():
    """(h)"""
    ref_work, work, taper, _ = Y.case_planes(3)
    sc, an, pl = (np.array(v) for v in zip(*Y.candidates()))
    with AlignContext.from_planes(ref_work, work, taper) as ctx:
        again = ctx.evaluate(sc, an, pl)
    first = device_case(3)
    for k, name in enumerate(A.AlignEval._fields):
        assert np.array_equal(first[k], again[k], equal_nan=True), name
    print("two runs (two contexts) of 208 candidates at (65, 82) are bit-identical")


@pytest.mark.parametrize("scale_range,angle_range,polarity,flip", [(0, 20, True, True), (0, 20, False, False), (0.05, 20, False, True),
                                                                   (0.05, 20, True, False)])
def test_align_images(scale_range, angle_range, polarity, flip):
    """(i) against the yardstick's align_images; optimiser trajectories are not compared"""
    ref, mov = Y.make_pair(*Y.CASES[1])
    want, trace = Y.align_images(mov, ref, scale_range, angle_range, check_polarity=polarity, check_flip=flip)
    got = align_images(mov, ref, scale_range, angle_range, check_polarity=polarity, check_flip=flip)
    assert len(got) == len(want) == (5 if flip else 4)
    flipped = bool(got[0]) if flip else False
    scale, angle, shift, score = got[-4:]
    ref_work, work, taper, _ = Y.prepare(ref, mov[::-1, :] if flipped else mov)
    e = Y.evaluate(ref_work, work, taper, scale, angle)
    print(f"align_images{(scale_range, angle_range, polarity, flip)}: device {flipped, float(scale), float(angle), tuple(shift), float(score)}; "
          f"yardstick there: shift {e['shift']}, score {e['score']:.9f}, gap {e['gap']:.3e}, borderline {e['borderline']}; "
          f"yardstick's own optimum {float(want[-1]):.9f}")
    if e["gap"] > 4 * Y.TOL_SURFACE:
        assert tuple(shift) == e["shift"]
    if tuple(shift) == e["shift"] and e["borderline"] == 0:
        assert abs(score - e["score"]) <= Y.TOL_SCORE
    assert score >= want[-1] - Y.TOL_SCORE
    with AlignContext(ref, [mov, mov[::-1, :]]) as ctx:
        dev = ctx.evaluate([t[0] for t in trace], [t[1] for t in trace], [int(t[2]) for t in trace])
    compare(dev, [t[3] for t in trace], f"trace of {len(trace)} evaluations", max_excluded=None)


def test_align_images_with_both_ranges_zero_and_the_aligned_image():
    ref, mov = Y.make_pair(*Y.CASES[1])
    want, _ = Y.align_images(mov, ref, 0, 0, check_flip=True)
    got = align_images(mov, ref, 0, 0, check_flip=True)
    print(f"both ranges 0: device {got}, yardstick {want}")
    assert got[:4] == want[:4] == (bool(want[0]), 1, 0, 0) and abs(got[4] - want[4]) <= 1e-12
    out = align_images(mov, ref, 0, 20, check_polarity=False, check_flip=False, return_aligned_moving_image=True)
    assert len(out) == 5 and out[4].shape == ref.shape
    padded = Y.prepare(ref, mov)[3]
    err = float(np.abs(out[4] - Y.aligned(padded, out[0], out[1], out[2])).max() / np.abs(padded).max())
    print(f"aligned image: max |device - yardstick| / max = {err:.3e}")
    assert err <= 1e-4     # as test_aligned_matches_the_yardstick_wrap_warp


@pytest.mark.parametrize("refine", [False, True])
def test_grid_recovers_a_planted_transform(refine):
    """(j) flip, 180 + 7 degrees, scale 1.03, shift (3, -5), to the grid's resolution"""
    q = Y.PLANTED
    ref, mov = Y.make_pair((48, 64), (48, 64), planted=True)
    angles, scales = np.arange(-10.0, 11.0, 1.0), np.array(Y.SCALES)
    best, scores = align_images_grid(mov, ref, scales, angles, refine=refine)
    print(f"planted {q}: best {best}, refine = {refine}")
    assert scores.shape == (2, 2, 4, 21) and np.isfinite(scores).all()
    assert best.flip is True and abs(best.angle - q["angle"]) <= 1.0 and abs(best.scale - q["scale"]) <= 0.03 + 1e-12
    assert np.abs(np.asarray(best.shift) - q["shift"]).max() <= 1
    assert best.score >= np.nanmax(scores) and best.score > 0.6
    if not refine:
        assert best.score == scores.max() and (best.angle, best.scale) == (q["angle"], q["scale"]) and tuple(best.shift) == q["shift"]
        many, all_scores = align_images_grid([mov, mov[::-1, :]], ref, scales, angles)
        assert all_scores.shape == (2, 2, 2, 4, 21) and np.array_equal(all_scores[0], scores)
        assert (many[0].flip, many[0].scale, many[0].angle, many[0].score) == (best.flip, best.scale, best.angle, best.score)
        assert many[1].flip is False and many[1].score == best.score and tuple(many[1].shift) == tuple(best.shift)


def test_command_line(tmp_path, capsys):
    import json

    from helicon_amd.mrc import read_mrc, write_mrc

    q = Y.PLANTED
    ref, mov = Y.make_pair((48, 64), (48, 64), planted=True)
    write_mrc(tmp_path / "ref.mrc", ref)
    write_mrc(tmp_path / "mov.mrc", mov)
    assert A.main([str(tmp_path / "mov.mrc"), str(tmp_path / "ref.mrc"), "--angle-range", "8", "--angle-step", "1", "--scale-range", "0.03",
                   "--scale-step", "0.03", "--out", str(tmp_path / "aligned.mrc")]) == 0
    rep = json.loads(capsys.readouterr().out)
    print(f"command line: {rep['best']}, {rep['candidates']} candidates")
    assert rep["candidates"] == 2 * 2 * 3 * 17
    assert rep["best"]["flip"] is True and rep["best"]["angle"] == q["angle"] and abs(rep["best"]["scale"] - q["scale"]) < 1e-12
    assert rep["best"]["shift"] == list(q["shift"])
    with AlignContext(ref, [mov[::-1, :]]) as ctx:
        want = ctx.aligned(rep["best"]["scale"], rep["best"]["angle"], rep["best"]["shift"], 0, "image")
    assert np.array_equal(np.asarray(read_mrc(tmp_path / "aligned.mrc")[0])[0], want)
