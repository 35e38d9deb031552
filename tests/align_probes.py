"""Shared by tests/test_align_probes_host.py and tests/test_gpu_align_probes.py: the probe table of the batched image alignment
(csrc/align.inc, helicon_amd/align.py), the float32 restatement of each stage around the transforms, the census of the rules
the probes reach and the wrong-rule variants the host test uses to show that an exact comparison would notice a defect.  CPU
only: nothing here imports the device package.

Every stage of one evaluation except the transforms is plain IEEE arithmetic in a fixed order, contraction off, so NumPy states
it BIT FOR BIT:

  first warp   k_align_warp: oracle.prep.warp_affine(float32 plane, 3 x 3 inverse), unchanged (warp_constant_f32 below is the
               same thing with its rules exposed; the host test asserts the two agree bit for bit)
  second warp  k_align_warp_wrap / k_align_score: warp_wrap_f32 — al_shifted (the translation column moved in float64, then the
               six entries cast), al_coords (c = h0 x + h1 y + h2 in float32, left to right), al_bilinear<true> (corners at
               floor / ceil, each through align_cases.coord_map; dr = r - float32(minr); the horizontal mixes in float32, the
               vertical mix in float64, then the cast), al_clip (np.clip to the plane's own range, skipped on a NaN range)
  mask, score  score_from_planes: align_cases.pearson in float64 on warped taper > 0; the device's six-moment formula differs
               from this two-pass one by at most 8 n 2^-53 max(kappa_a, kappa_b), kappa = sum x^2 / (n var x)
  shift        align_cases.shift_of on the device's own surface (the first arg-max of |c| in C order, the midpoint rule)

A probe is a frozen record: name, the rule it reaches, shape, the recipe of its planes (seeded from the name) and its own
candidates; ``planes(probe)`` and ``candidates(probe)`` give the arrays and the full list of (plane index, inverse matrix[,
scale, angle]).  Every probe except the largest sides also carries the FAR AND ODD matrices.  All planes are finite."""
import functools
import zlib
from collections import namedtuple
from dataclasses import dataclass

import numpy as np

import align_cases as Y

F32, F64 = np.float32, np.float64
CHUNK = 64                 # hh_align_chunk(): the GPU test asserts it
KAPPA_MAX = 1e4
U = 2.0 ** -53

Cand = namedtuple("Cand", "plane inv scale angle tag")      # inv: 6 float64, the first two rows of the unshifted inverse


# ------------------------------------------------------------------------------------------------------------ matrices
def _affine(scale, rotation, t):
    return np.array([[scale * np.cos(rotation), -scale * np.sin(rotation), t[0]],
                     [scale * np.sin(rotation), scale * np.cos(rotation), t[1]],
                     [0.0, 0.0, 1.0]])


def inverse_matrix6(shape, scale, angle):
    """The six entries ``AlignContext.evaluate`` sends for (scale, angle in degrees), composed as the package composes them
    (to the centre shape / 2, rotate / scale, back; float64; np.linalg.inv)."""
    s, r = np.atleast_1d(np.asarray(scale, dtype=F64)), np.deg2rad(np.atleast_1d(np.asarray(angle, dtype=F64)))
    cy, cx = shape[0] / 2.0, shape[1] / 2.0
    centre = np.zeros((s.size, 3, 3))
    centre[:, 0, 0], centre[:, 0, 1] = s * np.cos(r), -s * np.sin(r)
    centre[:, 1, 0], centre[:, 1, 1] = s * np.sin(r), s * np.cos(r)
    centre[:, 2, 2] = 1.0
    m = _affine(1.0, 0.0, (cx, cy)) @ (centre @ _affine(1.0, 0.0, (-cx, -cy)))
    return np.ascontiguousarray(np.linalg.inv(m)[:, :2, :].reshape(-1, 6))[0]


def full3(inv6):
    return np.vstack([np.asarray(inv6, dtype=F64).reshape(2, 3), [0.0, 0.0, 1.0]])


IDENTITY6 = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0)
HAIR = 2.0 ** -30          # a translation float32 drops and float64 keeps: the mask decision the two make differently


def far_and_odd(shape, n_planes):
    """Identity; quarter and half turns with exact integer entries; half-, quarter- and hair-pixel translations; translations
    of +-3.5 and +-40 sides (the first warp falls wholly outside, the wrap indices lie many periods away); scale 0.5 and 2; a
    shear; a reflection; ordinary (scale, angle) pairs, among them the right angles with cos 90 deg = 6e-17."""
    ny, nx = shape
    side = min(shape) - 1
    out = [Cand(0, tuple(inverse_matrix6(shape, 1.0, 0.0)), 1.0, 0.0, "identity")]       # plane 0: the reference is its roll
    raw = [("quarter turn", (0.0, -1.0, side, 1.0, 0.0, 0.0)), ("quarter turn back", (0.0, 1.0, float(nx // 2 - ny // 2), -1.0, 0.0, float(ny // 2 + nx // 2))),
           ("half turn", (-1.0, 0.0, nx - 1.0, 0.0, -1.0, ny - 1.0)),
           ("half pixel", (1.0, 0.0, 0.5, 0.0, 1.0, -0.5)), ("quarter pixel", (1.0, 0.0, -0.25, 0.0, 1.0, 0.75)),
           ("hair", (1.0, 0.0, 3.0 + HAIR, 0.0, 1.0, -2.0 - HAIR)), ("hair back", (1.0, 0.0, -1.0 - HAIR, 0.0, 1.0, 1.0 + HAIR)),
           ("3.5 sides", (1.0, 0.0, 3.5 * nx, 0.0, 1.0, -3.5 * ny)), ("-3.5 sides", (1.0, 0.0, -3.5 * nx, 0.0, 1.0, 3.5 * ny)),
           ("40 sides", (1.0, 0.0, 40.0 * nx + 0.3, 0.0, 1.0, -40.0 * ny - 0.6)), ("-40 sides", (1.0, 0.0, -40.0 * nx - 0.3, 0.0, 1.0, 40.0 * ny + 0.6)),
           ("shear", (1.0, 0.3, -1.0, 0.1, 1.0, 0.5)), ("reflection", (-1.0, 0.0, nx - 1.5, 0.0, 1.0, 0.25))]
    turned = inverse_matrix6(shape, 1.03, 37.3)
    turned[2] += 40.0 * nx
    turned[5] -= 40.0 * ny
    raw.append(("turned, 40 sides", tuple(turned)))
    for k, (tag, m) in enumerate(raw):
        out.append(Cand((k + 1) % n_planes, tuple(float(v) for v in m), None, None, tag))
    pairs = [(0.5, 0.0), (2.0, 0.0), (1.0, 90.0), (1.0, 180.0), (1.03, 37.3), (0.97, -121.9), (1.0, 7.0), (1.06, -14.5)]
    for k, (s, a) in enumerate(pairs):
        out.append(Cand(k % n_planes, tuple(inverse_matrix6(shape, s, a)), s, a, f"scale {s}, angle {a}"))
    return out


# ------------------------------------------------------------------------------------------------------------ the table
@dataclass(frozen=True)
class Probe:
    name: str
    rule: str                  # "kernel: what the probe reaches"
    shape: tuple
    n_planes: int
    recipe: str                # "plain", "ranges" or "tapers"
    own: tuple                 # ("pairs", ((scale, angle), ...)) | ("random", count) | ("few",)
    far: bool = True
    degenerate: bool = False   # holds candidates whose masked plane is constant, zero or empty (listed by the host test)


def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def _sname(shape):
    return "x".join(str(int(v)) for v in shape)


def _table():
    out = []
    pairs = ((1.0, 0.5), (1.02, -3.0), (0.98, 11.0))
    for shape in ((6, 257), (5, 258), (8, 256), (3, 300)):
        out.append(Probe(f"second_x_block/{_sname(shape)}", "k_align_warp, k_align_warp_wrap: blockIdx.x = 1; ncol 129 / 130 / 151, a one-column last tile",
                         shape, 2, "plain", ("pairs", pairs)))
    for shape in ((257, 6), (300, 3)):
        out.append(Probe(f"tall/{_sname(shape)}", "rows past 256, ncol 4 and 2, many row tiles per candidate", shape, 2, "plain", ("pairs", pairs)))
    for shape in ((2, 2), (2, 3), (3, 2), (5, 7), (7, 4)):
        out.append(Probe(f"smallest_sides/{_sname(shape)}", "k_align_c2r: a wavefront spans 5 ... 16 candidates (per-lane atomicMax); ncol = 2",
                         shape, 3, "plain", ("random", 24), degenerate=True))
    for shape in ((2, 1024), (1024, 2)):
        out.append(Probe(f"largest_sides/{_sname(shape)}", "the maximum side on each axis", shape, 2, "plain", ("few",), far=False))
    out.append(Probe("range_rules/12x20", "al_clip: preserve-zero and clip up / down on planes of disjoint ranges; range rows 2 m",
                     (12, 20), 5, "ranges", ("pairs", ((1.03, 37.3), (1.0, 0.0), (0.97, -8.0))), degenerate=True))
    out.append(Probe("taper_rules/12x20", "k_align_score: range rows 2 (M + m); an empty mask; a taper of both signs",
                     (12, 20), 5, "tapers", ("pairs", ((1.03, 37.3), (1.0, 0.0), (0.97, -8.0))), degenerate=True))
    for shape in ((9, 14), (16, 24)):
        out.append(Probe(f"far_and_odd/{_sname(shape)}", "al_coords, al_wrap, al_bilinear: far, exact and odd matrices", shape, 3, "plain", ("few",)))
    for shape in ((16, 24), (5, 7)):
        out.append(Probe(f"seam/{_sname(shape)}", "hh_align_eval: the chunk seam with a changing plane index", shape, 3, "plain", ("random", 2 * CHUNK + 1)))
    return tuple(out)


PROBES = _table()
BY_NAME = {p.name: p for p in PROBES}
assert len(BY_NAME) == len(PROBES)
RANGE_PROBES = ("range_rules/12x20", "taper_rules/12x20")
SEAM_PROBES = tuple(p.name for p in PROBES if p.name.startswith("seam/"))


def _soft_taper(rng, shape):
    """Values in [0, 0.7], about three in ten exactly 0, zeros beside positive pixels."""
    return np.maximum(rng.random(shape) - 0.3, 0.0).astype(F32)


@functools.lru_cache(maxsize=None)
def planes(name):
    """``(ref [ny, nx], moving [M, ny, nx], taper [M, ny, nx])``, float32, read-only.  The reference is plane 0 rolled by half a
    side on each axis: the identity candidate's arg-max sits exactly on the midpoint of both axes."""
    p = BY_NAME[name]
    rng = _rng(name)
    shape, M = p.shape, p.n_planes
    small = min(shape) < 5
    if p.recipe == "ranges":
        mov = [5.0 + 4.0 * rng.random(shape), -9.0 + 4.0 * rng.random(shape), 3.0 * rng.random(shape) - 1.0, np.full(shape, 3.0), np.zeros(shape)]
        tap = [Y.tapering_filter(shape), _soft_taper(rng, shape), Y.tapering_filter(shape), _soft_taper(rng, shape), Y.tapering_filter(shape)]
    elif p.recipe == "tapers":
        mov = [3.0 * rng.random(shape) - 1.0 + 2.0 * m for m in range(M)]
        both = np.where(np.arange(shape[1])[None, :] < shape[1] // 2, -4.0 + rng.random(shape), 3.0 + rng.random(shape))
        nonpos = np.where(rng.random(shape) < 0.2, 0.0, -2.0 + rng.random(shape))
        tap = [0.5 + 0.5 * rng.random(shape), nonpos, both, 2.0 + rng.random(shape), Y.tapering_filter(shape)]
    else:
        mov = [3.0 * rng.random(shape) - 1.0 + 0.5 * m for m in range(M)]
        if small:
            tap = [0.2 + 0.8 * rng.random(shape) for _ in range(M)]
            tap[-1].flat[rng.integers(tap[-1].size)] = 0.0
        else:
            tap = [Y.tapering_filter(shape) if m % 2 == 0 else _soft_taper(rng, shape) for m in range(M)]
    mov, tap = np.stack(mov).astype(F32), np.stack(tap).astype(F32)
    ref = np.roll(mov[0], (shape[0] // 2, shape[1] // 2), axis=(0, 1)).copy()
    for v in (ref, mov, tap):
        v.setflags(write=False)
    return ref, mov, tap


@functools.lru_cache(maxsize=None)
def caller_plane(name):
    """A plane that is not in the context (the ``which`` = plane route of ``aligned``): its own range, strictly positive."""
    v = (10.0 + 2.0 * _rng(name + "/caller").random(BY_NAME[name].shape)).astype(F32)
    v.setflags(write=False)
    return v


@functools.lru_cache(maxsize=None)
def candidates(name):
    p = BY_NAME[name]
    rng = _rng(name + "/candidates")
    M = p.n_planes
    out = []
    if p.own[0] == "pairs":
        for m in range(M):
            for s, a in p.own[1]:
                out.append(Cand(m, tuple(inverse_matrix6(p.shape, s, a)), s, a, f"plane {m}, scale {s}, angle {a}"))
        for m in range(M):      # a border of half-outside mixes on every side: clipped up (down) where 0 lies outside the range
            out.append(Cand(m, (1.0, 0.0, 2.5, 0.0, 1.0, 2.5), None, None, f"plane {m}, 2.5 pixels"))
            out.append(Cand(m, (1.0, 0.0, -2.5, 0.0, 1.0, -1.5), None, None, f"plane {m}, -2.5 pixels"))
    elif p.own[0] == "random":
        for k in range(p.own[1]):
            s, a, m = float(rng.uniform(0.9, 1.1)), float(rng.uniform(-180.0, 180.0)), int(rng.integers(M))
            out.append(Cand(m, tuple(inverse_matrix6(p.shape, s, a)), s, a, f"random {k}"))
    elif not p.far:
        out = [Cand(0, tuple(inverse_matrix6(p.shape, 1.0, 0.0)), 1.0, 0.0, "identity"),
               Cand(1, tuple(inverse_matrix6(p.shape, 1.0, 0.2)), 1.0, 0.2, "scale 1, angle 0.2"),
               Cand(1, (1.0, 0.0, 0.5, 0.0, 1.0, -0.5), None, None, "half pixel")]
    if p.far:
        out += far_and_odd(p.shape, M)
    return tuple(out)


# -------------------------------------------------------------------------------------------------------- the restatements
def wrap_index(i, dim, rule="periodic"):
    if rule == "periodic":
        return Y.coord_map(i, dim)
    q = np.mod(np.asarray(i, dtype=np.int64), 2 * dim)          # (wrong rule) reflection about the edges
    return np.where(q >= dim, 2 * dim - 1 - q, q)


def shifted6(inv6, shift, *, swapped=False, added=False):
    """al_shifted: the translation column in float64.  ``swapped`` / ``added``: wrong rules."""
    sy, sx = float(shift[0]), float(shift[1])
    if swapped:
        sy, sx = sx, sy
    h = np.array(inv6, dtype=F64)
    a, b = h[0] * sx + h[1] * sy, h[3] * sx + h[4] * sy
    h[2], h[5] = (h[2] + a, h[5] + b) if added else (h[2] - a, h[5] - b)
    return h


def coordinates(shape, h, coords="f32"):
    """al_coords: (c, r) float32.  ``coords="f64"`` (wrong rule): formed in float64 from the uncast matrix, then cast."""
    T = F32 if coords == "f32" else F64
    H = np.asarray(h, dtype=F64).astype(T)
    y, x = np.meshgrid(np.arange(shape[0]), np.arange(shape[1]), indexing="ij")
    x, y = x.astype(T), y.astype(T)
    with np.errstate(all="ignore"):
        c = H[0] * x + H[1] * y + H[2]
        r = H[3] * x + H[4] * y + H[5]
    return c.astype(F32), r.astype(F32)


Sample = namedtuple("Sample", "value minr maxr minc maxc")


def bilinear(image, c, r, *, wrap, ceil_rule="ceil", wrap_rule="periodic"):
    """al_bilinear<wrap>: the unclipped float32 value and the four corner indices before any mapping."""
    img = np.asarray(image, dtype=F32)
    rows, cols = img.shape
    minr, minc = np.floor(r).astype(np.int64), np.floor(c).astype(np.int64)
    maxr, maxc = (np.ceil(r).astype(np.int64), np.ceil(c).astype(np.int64)) if ceil_rule == "ceil" else (minr + 1, minc + 1)
    dr, dc = r - minr.astype(F32), c - minc.astype(F32)

    def pixel(rr, cc):
        if wrap:
            return img[wrap_index(rr, rows, wrap_rule), wrap_index(cc, cols, wrap_rule)]
        inside = (rr >= 0) & (rr < rows) & (cc >= 0) & (cc < cols)
        out = np.zeros(rr.shape, dtype=F32)
        out[inside] = img[rr[inside], cc[inside]]
        return out

    one = F32(1)
    with np.errstate(all="ignore"):
        top = ((one - dc) * pixel(minr, minc) + dc * pixel(minr, maxc)).astype(F64)
        bottom = ((one - dc) * pixel(maxr, minc) + dc * pixel(maxr, maxc)).astype(F64)
        value = ((one - dr).astype(F64) * top + dr.astype(F64) * bottom).astype(F32)
    return Sample(value, minr, maxr, minc, maxc)


def clip_f32(v, lo, hi, preserve_zero):
    """al_clip: a NaN range leaves v alone; an exact 0 stays where ``preserve_zero``; else the clamp."""
    if np.isnan(lo) or np.isnan(hi):
        return v
    out = np.clip(v, F32(lo), F32(hi))
    if preserve_zero:
        out[v == 0] = 0
    return out


def plane_range(plane):
    return np.asarray(plane).min(), np.asarray(plane).max()


def warp_wrap_f32(plane, inv6, shift, *, range_of=None, ceil_rule="ceil", wrap_rule="periodic", swapped=False, added=False,
                  coords="f32", preserve_zero=False):
    """The second warp (mode "wrap") of a float32 plane, bit for bit.  ``range_of``: the plane whose (min, max) the clip takes
    (default: the plane's own).  Every other keyword selects a WRONG rule."""
    img = np.asarray(plane, dtype=F32)
    c, r = coordinates(img.shape, shifted6(inv6, shift, swapped=swapped, added=added), coords)
    v = bilinear(img, c, r, wrap=True, ceil_rule=ceil_rule, wrap_rule=wrap_rule).value
    lo, hi = plane_range(img if range_of is None else range_of)
    return clip_f32(v, lo, hi, preserve_zero)


def warp_constant_f32(plane, inv6, *, range_of=None, preserve="rule", ceil_rule="ceil", coords="f32"):
    """The first warp (mode "constant", cval 0) with its rules exposed; the defaults are oracle.prep.warp_affine bit for bit."""
    img = np.asarray(plane, dtype=F32)
    c, r = coordinates(img.shape, inv6, coords)
    v = bilinear(img, c, r, wrap=False, ceil_rule=ceil_rule).value
    lo, hi = plane_range(img if range_of is None else range_of)
    keep = {"rule": not (lo <= 0.0 <= hi), "never": False, "always": True}[preserve]
    return clip_f32(v, lo, hi, keep)


def kappa(x):
    """sum x^2 / (n var x) = sum x^2 / sum (x - mean)^2 of a float64 vector: the condition of the one-pass variance."""
    if x.size == 0:
        return float("nan")
    dev = float(np.sum((x - np.mean(x)) ** 2))
    return float("inf") if dev == 0 else float(np.sum(x * x)) / dev


def score_from_planes(ref, warped, warped_taper):
    """``(score, nmask, (kappa_a, kappa_b))``: align_cases.pearson in float64 on ``warped_taper > 0``; NaN on an empty mask."""
    mask = np.asarray(warped_taper) > 0
    n = int(mask.sum())
    if n == 0:
        return float("nan"), 0, (float("nan"), float("nan"))
    a, b = np.asarray(ref)[mask].astype(F64), np.asarray(warped)[mask].astype(F64)
    return Y.pearson(a, b), n, (kappa(a), kappa(b))


def score_allowance(nmask, kappas):
    """The first-order bound of the six-moment formula against the two-pass one; 0 where the comparison is exact (an empty mask;
    a masked plane that is constant, whose deviations and moments are exact)."""
    k = max(kappas) if nmask else float("inf")
    return 0.0 if not np.isfinite(k) else 8.0 * nmask * U * k


def midpoint_shift(index, shape, rule=">"):
    """phase_cross_correlation's shift of an arg-max index.  ``rule=">="``: wrong."""
    return tuple(int(i - n) if (i > n // 2 if rule == ">" else i >= n // 2) else int(i) for i, n in zip(index, shape))


def flat_index(shift, shape):
    return (int(shift[0]) % shape[0]) * shape[1] + int(shift[1]) % shape[1]


def first_warp(name, cand, **variant):
    """The first warp of a candidate.  ``image_row="plane0"`` (wrong rule): the clip takes plane 0's range."""
    _, mov, _ = planes(name)
    row = variant.pop("image_row", "own")
    return warp_constant_f32(mov[cand.plane], cand.inv, range_of=mov[0] if row == "plane0" else None, **variant)


def host_index(name, cand, **variant):
    """The arg-max index of the float64 phase correlation of the reference with the (float32) first warp: the host's stand-in
    for the device's key where a census or a variant needs a shift."""
    ref, _, _ = planes(name)
    _, c = Y.cross_power(ref, first_warp(name, cand, **variant))
    a = np.abs(c)
    return tuple(int(v) for v in np.unravel_index(int(np.argmax(a)), a.shape))


@functools.lru_cache(maxsize=None)
def host_indices(name):
    """host_index of every candidate of a probe, computed once."""
    return tuple(host_index(name, cand) for cand in candidates(name))


def restate(name, cand, shift, *, taper_row="taper", image_row="own", **variant):
    """The score pass of one candidate at ``shift``: dict(warped, warped_taper, score, nmask, kappa, allowance).  ``taper_row =
    "image"`` / ``image_row = "plane0"`` (wrong rules): the range row 2 m for the taper, row 0 for the image."""
    ref, mov, tap = planes(name)
    m = cand.plane
    wt = warp_wrap_f32(tap[m], cand.inv, shift, range_of=mov[m] if taper_row == "image" else None, **variant)
    wm = warp_wrap_f32(mov[m], cand.inv, shift, range_of=mov[0] if image_row == "plane0" else None, **variant)
    score, n, kap = score_from_planes(ref, wm, wt)
    return dict(warped=wm, warped_taper=wt, score=score, nmask=n, kappa=kap, allowance=score_allowance(n, kap))


def degenerate_reason(name, cand, r):
    """None, or why the reference's score of a candidate is exact: ``(reason, value)``."""
    _, mov, _ = planes(name)
    if r["nmask"] == 0:
        return "empty mask", float("nan")
    if not mov[cand.plane].any():
        return "zero plane", 0.0
    if not np.isfinite(max(r["kappa"])):
        return "constant plane", 0.0
    return None


# ------------------------------------------------------------------------------------------------------------- the census
CENSUS_RULES = ("corner above", "corner below", "corner left", "corner right", "wrapped row < 0", "wrapped row > ny - 1",
                "wrapped column < 0", "wrapped column > nx - 1", "two periods away", "preserved zero", "clipped up", "clipped down",
                "warp wholly outside", "float64 decides the mask differently")


def census(name):
    """Pixels of the probe's candidates on which each named rule acts (the second warp at the host's shift)."""
    ref, mov, tap = planes(name)
    rows, cols = ref.shape
    n = dict.fromkeys(CENSUS_RULES, 0)
    for cand, idx in zip(candidates(name), host_indices(name)):
        img = mov[cand.plane]
        s = bilinear(img, *coordinates(img.shape, cand.inv), wrap=False)
        inside = lambda rr, cc: (rr >= 0) & (rr < rows) & (cc >= 0) & (cc < cols)
        some = inside(s.minr, s.minc) | inside(s.minr, s.maxc) | inside(s.maxr, s.minc) | inside(s.maxr, s.maxc)
        n["corner above"] += int((some & (s.minr < 0)).sum())
        n["corner below"] += int((some & (s.maxr >= rows)).sum())
        n["corner left"] += int((some & (s.minc < 0)).sum())
        n["corner right"] += int((some & (s.maxc >= cols)).sum())
        n["warp wholly outside"] += int(not some.any())
        lo, hi = plane_range(img)
        out = first_warp(name, cand)
        if not lo <= 0.0 <= hi:
            n["preserved zero"] += int((out == 0).sum())
            n["clipped up"] += int(((s.value != 0) & (s.value < lo)).sum())
            n["clipped down"] += int(((s.value != 0) & (s.value > hi)).sum())
        shift = midpoint_shift(idx, ref.shape)
        h = shifted6(cand.inv, shift)
        w = bilinear(tap[cand.plane], *coordinates(ref.shape, h), wrap=True)
        n["wrapped row < 0"] += int((w.minr < 0).sum())
        n["wrapped row > ny - 1"] += int((w.maxr > rows - 1).sum())
        n["wrapped column < 0"] += int((w.minc < 0).sum())
        n["wrapped column > nx - 1"] += int((w.maxc > cols - 1).sum())
        n["two periods away"] += int(((w.minr < -rows) | (w.maxr >= 2 * rows) | (w.minc < -cols) | (w.maxc >= 2 * cols)).sum())
        f32 = warp_wrap_f32(tap[cand.plane], cand.inv, shift) > 0
        f64 = Y.warp_wrap(tap[cand.plane], full3(h)) > 0
        n["float64 decides the mask differently"] += int((f32 != f64).sum())
    return n


# ---------------------------------------------------------------------------------------------------- the wrong-rule variants
@dataclass(frozen=True)
class Variant:
    rule: str              # the one rule of align.inc changed
    stage: str             # "wrap" (keywords of warp_wrap_f32 / restate), "first" (of first_warp) or "shift"
    kw: tuple              # the keywords, as items
    finite_blind: str = ""  # why no finite (normal) plane can show it, where that is so; else ""
    probes: tuple = ("far_and_odd/9x14", "range_rules/12x20", "taper_rules/12x20")     # at least one of these must be bitten


VARIANTS = {
    "maxr = minr + 1 for ceil": Variant("al_bilinear corners", "wrap", (("ceil_rule", "floor+1"),),
                                        "at an integer coordinate the other corner carries weight 0 exactly, and 0 * finite = 0"),
    "wrap by reflection": Variant("al_wrap", "wrap", (("wrap_rule", "reflect"),)),
    "shift applied as (sx, sy)": Variant("al_shifted argument order", "wrap", (("swapped", True),)),
    "shift added": Variant("al_shifted sign", "wrap", (("added", True),)),
    "midpoint with >=": Variant("al_key_shift", "shift", (("rule", ">="),)),
    "clip without the preserve-zero rule": Variant("k_align_warp: al_clip(..., !(lo <= 0 && 0 <= hi))", "first", (("preserve", "never"),)),
    "clip always preserving zeros": Variant("k_align_warp_wrap / k_align_score: al_clip(..., false)", "wrap", (("preserve_zero", True),),
                                            "a mix of values on one side of 0 is itself there unless a product underflows: no exact 0 to keep"),
    "taper's range row 2 m": Variant("k_align_score tlo / thi", "wrap", (("taper_row", "image"),)),
    "image's range row from plane 0": Variant("k_align_warp / k_align_score range[2 m]", "wrap", (("image_row", "plane0"),)),
    "coordinates in float64": Variant("al_coords", "wrap", (("coords", "f64"),)),
}


def variant_bites(vname, name):
    """The exact items of a probe that the variant changes: a list of short strings (empty: the probe cannot tell)."""
    v = VARIANTS[vname]
    kw = dict(v.kw)
    ref, mov, tap = planes(name)
    out = []
    for k, (cand, idx) in enumerate(zip(candidates(name), host_indices(name))):
        shift = midpoint_shift(idx, ref.shape)
        if v.stage == "shift":
            wrong = midpoint_shift(idx, ref.shape, **kw)
            if wrong != shift:
                out.append(f"candidate {k} ({cand.tag}): shift {shift} -> {wrong}")
            continue
        if v.stage == "first":
            a, b = first_warp(name, cand), first_warp(name, cand, **kw)
            if not np.array_equal(a, b):
                out.append(f"candidate {k} ({cand.tag}): {int((a != b).sum())} pixels of the first warp")
            continue
        if "image_row" in kw:
            a, b = first_warp(name, cand), first_warp(name, cand, **kw)
            if not np.array_equal(a, b):
                out.append(f"candidate {k} ({cand.tag}): {int((a != b).sum())} pixels of the first warp")
        good, bad = restate(name, cand, shift), restate(name, cand, shift, **kw)
        for key, what in (("warped", "pixels of the second warp"), ("warped_taper", "pixels of the warped taper")):
            d = int((good[key] != bad[key]).sum())
            if d:
                out.append(f"candidate {k} ({cand.tag}): {d} {what}")
        if good["nmask"] != bad["nmask"]:
            out.append(f"candidate {k} ({cand.tag}): nmask {good['nmask']} -> {bad['nmask']}")
    return out
