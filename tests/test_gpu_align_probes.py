"""The stages of the batched image alignment around its transforms (csrc/align.inc: k_align_warp, k_align_warp_wrap, the
arg-max epilogue of k_align_c2r, k_align_score, k_align_finish) against tests/align_probes.py, BIT FOR BIT and with no pixel and
no candidate left out; only the score carries a bound, the first-order one of the six-moment formula, worked out per candidate
from the restated planes.  Everything goes through AlignContext.from_planes, evaluate_matrices, correlation and aligned.

  (a) first warp    a second context whose moving planes are oracle.prep.warp_affine of every candidate, evaluated at the
                    identity (which copies a finite plane exactly), gives the same surfaces, peaks and shifts
  (b) arg-max       evaluate's shift (one launch for all candidates) is align_cases.shift_of the surface correlation() returns
                    (one candidate per launch): the first arg-max of |c| in C order, the midpoint rule; the peak is its maximum
  (c) wrap warp     aligned() is warp_wrap_f32 on every pixel: the prepared plane, its taper, a caller's plane; the device's own
                    shift and three fixed ones
  (d) mask, score   with the device's own shift, nmask is the restatement's on every candidate; the score lies within
                    8 nmask 2^-53 max(kappa_a, kappa_b) of align_cases.pearson, and is exactly NaN / 0 where that is exact
  (e) range table   the planes in reversed order, indices remapped: bit-identical
  (f) determinism   the seam probes as one call, permuted and one candidate at a time: bit-identical

Every test prints its figure before it asserts.  On an MI355X (profiles/align.json, "probes"): 885 candidates, 601 surfaces,
4,452 wrap warps (2.0 M pixels) and every mask count without one difference; 15 tied maxima resolved as np.argmax does; the
scores use at most 0.123 of their allowance (at (2, 2); below 0.01 from (5, 7) up); 80 tests in 2.5 s."""
import functools

import numpy as np
import pytest

from oracle import prep as P
import align_cases as Y
import align_probes as Q
from helicon_amd import align as A
from helicon_amd.align import AlignContext

pytestmark = pytest.mark.gpu

NAMES = [p.name for p in Q.PROBES]
FIELDS = A.AlignEval._fields


@functools.lru_cache(maxsize=None)
def matrices(name):
    """``[n, 6]`` float64 of the probe's candidates; a (scale, angle) candidate's row is what ``correlation`` and ``aligned``
    compose for it themselves (the probe's own composition restates that one: asserted)."""
    cands = Q.candidates(name)
    inv = np.array([c.inv for c in cands], dtype=np.float64)
    shape = Q.BY_NAME[name].shape
    for k, c in enumerate(cands):
        if c.scale is not None:
            assert np.array_equal(A.inverse_matrices(shape, c.scale, c.angle)[0], inv[k]), (name, c.tag)
    inv.setflags(write=False)
    return inv


def context(name, reverse=False):
    ref, mov, tap = Q.planes(name)
    return AlignContext.from_planes(ref, mov[::-1] if reverse else mov, tap[::-1] if reverse else tap)


@functools.lru_cache(maxsize=None)
def device_eval(name):
    """The device's evaluation of every candidate of a probe in one call, computed once."""
    assert A.chunk() == Q.CHUNK
    with context(name) as ctx:
        return ctx.evaluate_matrices(matrices(name), [c.plane for c in Q.candidates(name)])


def same(a, b):
    return all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a, b))


@pytest.mark.parametrize("name", NAMES)
def test_first_warp_by_two_contexts(name):
    """(a)"""
    ref, mov, _ = Q.planes(name)
    cands, inv, got = Q.candidates(name), matrices(name), device_eval(name)
    warped = np.stack([P.warp_affine(mov[c.plane], Q.full3(inv[k])) for k, c in enumerate(cands)])
    assert warped.dtype == np.float32
    surfaces = pixels = 0
    with context(name) as a, AlignContext.from_planes(ref, warped, np.ones_like(warped)) as b:
        want = b.evaluate_matrices(np.tile(np.asarray(Q.IDENTITY6), (len(cands), 1)), np.arange(len(cands)))
        bad = []
        for k, c in enumerate(cands):
            if c.scale is None:
                continue
            ca, cb = a.correlation(c.scale, c.angle, c.plane), b.correlation(1.0, 0.0, k)
            surfaces += 1
            pixels += int((ca != cb).sum())
            if not np.array_equal(ca, cb):
                bad.append(c.tag)
    peaks, shifts = int((got.peaks != want.peaks).sum()), int((got.shifts != want.shifts).any(axis=1).sum())
    print(f"{name}: {len(cands)} candidates: peaks differ on {peaks}, shifts on {shifts}; {surfaces} surfaces, {pixels} pixels differ {bad[:4]}")
    assert peaks == 0 and shifts == 0 and pixels == 0


@pytest.mark.parametrize("name", NAMES)
def test_argmax_against_the_device_surface(name):
    """(b)"""
    shape = Q.BY_NAME[name].shape
    cands, got = Q.candidates(name), device_eval(name)
    bad, n, ties = [], 0, 0
    with context(name) as ctx:
        for k, c in enumerate(cands):
            if c.scale is None:
                continue
            s = np.abs(ctx.correlation(c.scale, c.angle, c.plane))
            n += 1
            ties += int((s == s.max()).sum() > 1)
            ok = (tuple(int(v) for v in got.shifts[k]) == Y.shift_of(s) and Q.flat_index(got.shifts[k], shape) == int(np.argmax(s))
                  and got.peaks[k] == s.max())
            if not ok:
                bad.append((c.tag, tuple(got.shifts[k]), Y.shift_of(s), float(got.peaks[k]), float(s.max())))
    print(f"{name}: {n} surfaces (one candidate per launch) against one evaluation of {len(cands)}: {len(bad)} differ {bad[:3]}; "
          f"{ties} surfaces with a tied maximum")
    assert n > 0 and not bad


def fixed_shifts(shape):
    ny, nx = shape
    return ((0, 0), (1, -1), (ny + 2, -nx - 3))


@pytest.mark.parametrize("name", NAMES)
def test_wrap_warp_every_pixel(name):
    """(c)"""
    shape = Q.BY_NAME[name].shape
    ref, mov, tap = Q.planes(name)
    caller = Q.caller_plane(name)
    cands, got = Q.candidates(name), device_eval(name)
    calls = pixels = 0
    bad = []
    with context(name) as ctx:
        seen = 0
        for k, c in enumerate(cands):
            if c.scale is None:
                continue
            own = tuple(int(v) for v in got.shifts[k])
            sources = (("work", mov[c.plane]), ("taper", tap[c.plane]), (caller, caller))
            todo = [(own, s) for s in sources]
            if seen < 16:
                todo += [(sh, s) for sh in fixed_shifts(shape) for s in sources]
            else:
                todo.append((fixed_shifts(shape)[seen % 3], sources[seen % 3]))
            seen += 1
            for shift, (which, src) in todo:
                out = ctx.aligned(c.scale, c.angle, shift, c.plane, which)
                want = Q.warp_wrap_f32(src, c.inv, shift)
                calls += 1
                d = int((out != want).sum())
                pixels += d
                if d or out.dtype != np.float32:
                    bad.append((c.tag, shift, which if isinstance(which, str) else "plane", d))
    print(f"{name}: {calls} wrap warps of {shape[0] * shape[1]} pixels: {pixels} pixels differ from the float32 restatement {bad[:4]}")
    assert calls > 0 and not bad


@pytest.mark.parametrize("name", NAMES)
def test_mask_counts_and_scores_nobody_left_out(name):
    """(d)"""
    cands, got = Q.candidates(name), device_eval(name)
    wrong_n, wrong_exact, over, used, exact = [], [], [], 0.0, 0
    for k, c in enumerate(cands):
        shift = tuple(int(v) for v in got.shifts[k])
        r = Q.restate(name, c, shift)
        if got.nmask[k] != r["nmask"]:
            wrong_n.append((c.tag, int(got.nmask[k]), r["nmask"]))
        if not Q.first_warp(name, c).any():                  # a zero plane, or a warp that falls wholly outside
            if shift != (0, 0) or got.peaks[k] != 0:
                wrong_exact.append((c.tag, shift, float(got.peaks[k])))
        if r["allowance"] == 0.0:                            # NaN on an empty mask, 0 on a constant or zero plane
            exact += 1
            if not (np.isnan(got.scores[k]) if np.isnan(r["score"]) else got.scores[k] == r["score"] == 0.0):
                wrong_exact.append((c.tag, float(got.scores[k]), r["score"]))
            continue
        d = abs(float(got.scores[k]) - r["score"])
        used = max(used, d / r["allowance"])
        if not d <= r["allowance"]:
            over.append((c.tag, d, r["allowance"], r["nmask"], r["kappa"]))
    print(f"{name}: {len(cands)} candidates: nmask differs on {len(wrong_n)} {wrong_n[:3]}; {exact} exact scores (NaN / 0), {len(wrong_exact)} wrong "
          f"{wrong_exact[:3]}; largest share of the score allowance used {used:.3f}; over it: {over[:3]}")
    assert not wrong_n and not wrong_exact and not over


@pytest.mark.parametrize("name", Q.RANGE_PROBES)
def test_range_table_with_the_planes_reversed(name):
    """(e)"""
    cands, inv, got = Q.candidates(name), matrices(name), device_eval(name)
    M = Q.BY_NAME[name].n_planes
    n = 0
    with context(name) as fwd, context(name, reverse=True) as rev:
        again = rev.evaluate_matrices(inv, [M - 1 - c.plane for c in cands])
        warps = True
        for k, c in enumerate(cands):
            if c.scale is None:
                continue
            shift = got.shifts[k]
            for which in ("work", "taper"):
                n += 1
                warps &= np.array_equal(fwd.aligned(c.scale, c.angle, shift, c.plane, which), rev.aligned(c.scale, c.angle, shift, M - 1 - c.plane, which))
            warps &= np.array_equal(fwd.correlation(c.scale, c.angle, c.plane), rev.correlation(c.scale, c.angle, M - 1 - c.plane))
    differ = [f for f, x, y in zip(FIELDS, got, again) if not np.array_equal(x, y, equal_nan=True)]
    print(f"{name}: {len(cands)} candidates with the {M} planes reversed: fields that differ {differ}; {n} wrap warps and {n // 2} surfaces identical: {bool(warps)}")
    assert not differ and warps


@pytest.mark.parametrize("name", Q.SEAM_PROBES)
def test_seam_determinism(name):
    """(f)"""
    cands, inv = Q.candidates(name), matrices(name)
    idx = np.array([c.plane for c in cands])
    n = len(cands)
    order = np.random.default_rng(3).permutation(n)
    with context(name) as ctx:
        batch = ctx.evaluate_matrices(inv, idx)
        mixed = ctx.evaluate_matrices(inv[order], idx[order])
        single = [ctx.evaluate_matrices(inv[k:k + 1], idx[k:k + 1]) for k in range(n)]
    one = [np.concatenate([s[f] for s in single]) for f in range(len(FIELDS))]
    ok = same(batch, one), same([v[order] for v in batch], mixed), same(batch, device_eval(name))
    print(f"{name}: {n} candidates (chunks of {Q.CHUNK}): the batch equals {n} single evaluations: {ok[0]}, a permutation of it: {ok[1]}, "
          f"another context: {ok[2]}")
    assert all(ok)
