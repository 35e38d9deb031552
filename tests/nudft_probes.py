"""Probes of the non-uniform DFT (csrc/nudft.inc, hh_nudft2d2) whose expectations are CLOSED FORMS, not sums: deltas, constants,
full rows and full columns, and their sums by linearity, at every side from 1 to 130, on and just before every compiled-in seam
(NU_T = 64 rows, NU_K = 32 columns a slice, NU_KS = 128 columns a stage), at the compiled limit of 16384, and in stacks that
reach every images-per-workgroup form.  NumPy only; nothing of the package is imported here.

    delta h at (a0, c0)     F = h exp(-i (x (a0 - ny // 2) + y (c0 - nx // 2)))
    constant m              F = m D(x, ny) D(y, nx),  D(t, n) = exp(-i t (-(n // 2) + (n - 1) / 2)) sin(n t / 2) / sin(t / 2),
                            D = n where sin(t / 2) = 0
    full row a0 of value v  F = v exp(-i x (a0 - ny // 2)) D(y, nx);  a full column likewise with D(x, ny)
    unit noise (+ offset)   the one part that is summed: pixel_size_cases.yardstick

The one bound, per image and point, for the complex and the abs output alike (``allowance``)::

    |got - want| <= B sum |f - mean| + 2^-23 |want| + ny nx (ny + nx) 2^-53 |mean|

B is pixel_size_cases.B; for a delta, whose sum |f - mean| is 2 h (1 - 1 / (ny nx)), it is a phase check to 6e-6 radians.  The
second term is complex64's own rounding of the result, the third a pessimistic float64 bound on the two axis sums of the mean's
term.  No tolerance here comes from device output.

``model`` is the direct sum as the kernel lays it out (mean removed and rounded once, the mean's term apart, launches of
``CHUNK`` points and images, ``ipw`` images a workgroup) with one switch per WRONG rule; tests/test_nudft_probes_host.py shows
that each of them breaks the bound on a named probe."""
import functools
from typing import NamedTuple

import numpy as np

import pixel_size_cases as Y

CHUNK = 32768                  # hh_nudft_chunk(); the GPU test asserts it
NU_T, NU_K, NU_KS = 64, 32, 128
MAX_SIDE = 16384
N_POINTS = 65
ACC_ROWS = (3, 4, 7, 8, 12)    # the lane map 4 h + {0..3, 8..11, ...}: the last and first row of a lane's run, and a run apart
CONSTANT, LIMIT_CONSTANT, ROW_VALUE, COL_VALUE, NOISE_OFFSET = 1000.25, 0.5, 1.0, 0.5, 1000.25

RULES = {
    "centre": "index k of a side n stands at k - n // 2",
    "pairing": "x goes with the first image axis",
    "sign": "the exponent is negative",
    "phase_reduction": "a phase is reduced in float64 before its sine and cosine",
    "row_tail": "rows past ny of the last 64-row tile add nothing",
    "col_tail": "columns past nx of the last 128-column stage add nothing",
    "stage_seam": "column 128 s is the first of stage s",
    "slice_base": "a slice's base phase is that of its first column",
    "acc_rows": "register i of lane (r, h) is accumulator row (i & 3) + 8 (i >> 2) + 4 h",
    "mean_term": "the mean's separable term is added",
    "mean_centre": "the mean's term is centred at n // 2",
    "ragged_group": "the last, shorter group of images runs",
    "image_turn": "every image of a workgroup's turn gets its own sum",
    "ring_index": "the ring maximum groups by the call's point index",
}
WRONG = {   # switch of ``model`` -> (the rule it breaks, what it does instead)
    "centre": ("centre", "centre (n - 1) // 2"),
    "pairing": ("pairing", "x paired with the columns"),
    "sign": ("sign", "sign +"),
    "f32phase": ("phase_reduction", "float32 unreduced phases"),
    "row_pad": ("row_tail", "rows past ny repeat the last row to the end of their 64-row tile"),
    "col_pad": ("col_tail", "columns past nx repeat the last column to the end of their 128-column stage"),
    "stage_first": ("stage_seam", "the first column of a stage is taken from the column before it"),
    "slice_late": ("slice_base", "a slice's base phase (after the first) is taken one column late"),
    "acc_swap": ("acc_rows", "accumulator rows 4-7 and 8-11 are swapped"),
    "no_mean": ("mean_term", "the mean's term is left out"),
    "mean_off_centre": ("mean_centre", "the mean's term is centred at (n - 1) // 2"),
    "skip_ragged": ("ragged_group", "the last ragged image group is skipped"),
    "prev_image": ("image_turn", "an image after the first of its group returns the sum of the one before it"),
    "ring_local": ("ring_index", "the ring maximum is grouped by the launch-local point index"),
}


# ---------------------------------------------------------------------------------------------------------------- closed forms

def dirichlet(t, n):
    """complex128: sum_{k < n} exp(-i t (k - n // 2)).  The indices are whole numbers, so t is taken modulo 2 pi first: next to
    a multiple of 2 pi the quotient of the two sines would otherwise be that of their rounding errors."""
    t = np.asarray(t, dtype=np.float64)
    t = t - 2 * np.pi * np.rint(t / (2 * np.pi))
    s = np.sin(t / 2)
    flat = s == 0
    ratio = np.where(flat, float(n), np.sin(n * t / 2) / np.where(flat, 1.0, s))
    return np.exp(-1j * t * (-(n // 2) + (n - 1) / 2)) * ratio


def _noise(shape, seed, offset):
    rng = np.random.default_rng([Y.SEED, shape[0], shape[1], seed])
    return (offset + rng.standard_normal(shape)).astype(np.float32)


def part_image(part, shape):
    """float64 [ny, nx] of one part: ("delta", a0, c0, h), ("const", m), ("row", a0, v), ("col", c0, v), ("noise", seed, offset)."""
    out = np.zeros(shape, np.float64)
    kind = part[0]
    if kind == "delta":
        out[part[1], part[2]] = part[3]
    elif kind == "const":
        out[:] = part[1]
    elif kind == "row":
        out[part[1], :] = part[2]
    elif kind == "col":
        out[:, part[1]] = part[2]
    elif kind == "noise":
        out[:] = _noise(shape, part[1], part[2])
    else:
        raise ValueError(kind)
    return out


def part_expect(part, shape, x, y):
    """complex128 [P] of one part with a closed form."""
    ny, nx = shape
    kind = part[0]
    if kind == "delta":
        return part[3] * np.exp(-1j * (x * (part[1] - ny // 2) + y * (part[2] - nx // 2)))
    if kind == "const":
        return part[1] * dirichlet(x, ny) * dirichlet(y, nx)
    if kind == "row":
        return part[2] * np.exp(-1j * x * (part[1] - ny // 2)) * dirichlet(y, nx)
    if kind == "col":
        return part[2] * np.exp(-1j * y * (part[1] - nx // 2)) * dirichlet(x, ny)
    raise ValueError(kind)      # noise has no closed form: expect() sums the whole image


class Probe(NamedTuple):
    label: str
    family: str
    shape: tuple          # (ny, nx)
    parts: tuple          # per image: a tuple of parts; the image is their sum
    n_pts: int
    rules: tuple          # names of RULES it reaches
    ipw: tuple = (1,)     # images per workgroup of each point launch, by the formula of nudft.inc
    pick: tuple = None    # the point indices compared (the 17-image case alone), fixed here
    ring_group: int = 0   # a ring-maximum group of its own, beyond 1 and n_pts


def images(probe):
    """float32 [B, ny, nx], read-only."""
    return _images(probe.label)


def points(probe):
    """(x, y) float64 [n_pts]: pixel_size_cases.points; the ring probe's last point is the origin again."""
    return _points(probe.label)


def expect(probe, idx=None):
    """complex128 [B, P] (or [B, len(idx)]): the closed forms at the probe's points."""
    x, y = points(probe)
    if idx is not None:
        x, y = x[idx], y[idx]
    ny, nx = probe.shape
    lone = [p for p in probe.parts if len(p) == 1 and p[0][0] == "delta"]
    if len(lone) == len(probe.parts) and len(lone) > 64:      # a long stack of single deltas, at once
        a = np.array([p[0][1] for p in lone], np.float64) - ny // 2
        c = np.array([p[0][2] for p in lone], np.float64) - nx // 2
        h = np.array([p[0][3] for p in lone], np.float64)
        return h[:, None] * np.exp(-1j * (a[:, None] * x[None, :] + c[:, None] * y[None, :]))
    out = np.zeros((len(probe.parts), x.size), np.complex128)
    for b, parts in enumerate(probe.parts):
        if any(part[0] == "noise" for part in parts):         # summed, and of the float32 image as it is handed over
            out[b] = Y.yardstick(x, y, images(probe)[b])
            continue
        for part in parts:
            out[b] += part_expect(part, probe.shape, x, y)
    return out


def allowance(f, want):
    """float64 [B, P]: the bound of this module's docstring for a stack ``f`` [B, ny, nx] and its expectation [B, P]."""
    f = np.asarray(f, dtype=np.float64)
    ny, nx = f.shape[-2:]
    mean = f.mean(axis=(-2, -1))
    s = np.abs(f - mean[:, None, None]).sum(axis=(-2, -1))
    return Y.B * s[:, None] + 2.0 ** -23 * np.abs(want) + ny * nx * (ny + nx) * 2.0 ** -53 * np.abs(mean)[:, None]


def share(got, want, lim):
    """The largest used share of the allowance; an error of 0 against an allowance of 0 uses none of it."""
    err = np.abs(np.asarray(got) - want)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(err == 0, 0.0, err / lim)
    return float(q.max())


def ring_of(mag, group, local=False, chunk=CHUNK):
    """[group]: the maximum over images and over the points p with p % group == r of ``mag`` [B, P] (``local``: the wrong
    rule, p taken within its launch)."""
    p = np.arange(mag.shape[1])
    r = (p % chunk if local else p) % group
    out = np.zeros(group, mag.dtype)
    np.maximum.at(out, r, mag.max(axis=0))
    return out


def ring_allowance(lim, group):
    """[group]: the maximum is 1-Lipschitz, so a ring value moves by at most the largest allowance of its points."""
    return ring_of(lim, group)


# ------------------------------------------------------------------------------------------------------------ launch geometry

def ipw_of(n_img, n_pts):
    """Images a workgroup takes in turn in a launch of ``n_img`` images and ``n_pts`` points: nudft.inc's
    ``min(8, max(1, nb * tiles / 4096))`` with tiles = ceil(np / 64)."""
    tiles = (n_pts + NU_T - 1) // NU_T
    return int(min(8, max(1, n_img * tiles // 4096)))


def launches(n_img, n_pts, chunk=CHUNK):
    """[(p0, np, b0, nb, ipw)] of a call, in the order hh_nudft2d2 launches them."""
    out = []
    for p0 in range(0, n_pts, chunk):
        np_ = min(chunk, n_pts - p0)
        for b0 in range(0, n_img, chunk):
            nb = min(chunk, n_img - b0)
            out.append((p0, np_, b0, nb, ipw_of(nb, np_)))
    return out


def group_edges(n_img, n_pts):
    """Image indices on both sides of the first, a middle and the last workgroup boundary of the first launch, with the first
    and the last image: the sample that is transformed alone."""
    _, _, _, nb, ipw = launches(n_img, n_pts)[0]
    groups = (nb + ipw - 1) // ipw
    pick = {0, n_img - 1}
    for g in {1, groups // 2, groups - 1}:
        if 0 < g < groups:
            pick |= {g * ipw - 1, g * ipw}
    return sorted(b for b in pick if 0 <= b < n_img)


# ------------------------------------------------------------------------------------------------------------------ the model

def model(x, y, f, wrong=None, n_pts_call=None, idx=None, chunk=CHUNK, col_phase=None):
    """complex128 [B, P]: the direct sum in the kernel's layout.  ``wrong``: a key of WRONG (``ring_local`` changes nothing
    here, see ring_of).  ``idx``: the indices, within a call of ``n_pts_call`` points, that ``x`` and ``y`` are; the image-group
    rules need them.  ``col_phase`` = (column, radians): a phase error on one column, for the record of what noise hides."""
    assert wrong is None or wrong in WRONG
    f = np.asarray(f, dtype=np.float32)
    x = np.asarray(x, dtype=np.float64).reshape(-1)
    y = np.asarray(y, dtype=np.float64).reshape(-1)
    n_img, ny, nx = f.shape
    mean = f.astype(np.float64).mean(axis=(1, 2))
    g = (f.astype(np.float64) - mean[:, None, None]).astype(np.float32).astype(np.float64)
    if wrong == "stage_first":
        first = np.arange(NU_KS, nx, NU_KS)
        g[:, :, first] = g[:, :, first - 1]
    if wrong == "row_pad" and ny % NU_T:
        g = np.concatenate([g, np.repeat(g[:, -1:, :], NU_T - ny % NU_T, axis=1)], axis=1)
    if wrong == "col_pad" and nx % NU_KS:
        g = np.concatenate([g, np.repeat(g[:, :, -1:], NU_KS - nx % NU_KS, axis=2)], axis=2)
    rows, cols = np.arange(g.shape[1]), np.arange(g.shape[2])
    off = (lambda n: (n - 1) // 2) if wrong == "centre" else (lambda n: n // 2)
    kr, kc = rows - off(ny), cols - off(nx)
    if wrong == "slice_late":
        kc = np.where(cols >= NU_K, kc + 1, kc)
    if wrong == "acc_swap":
        r = rows % 32
        kr = kr + np.where((r >= 4) & (r < 8), 4, np.where((r >= 8) & (r < 12), -4, 0))
    tr, tc = (y, x) if wrong == "pairing" else (x, y)
    sign = 1j if wrong == "sign" else -1j

    def unit(t, k):
        if wrong == "f32phase":
            return np.exp(sign * (t.astype(np.float32)[:, None] * k.astype(np.float32)[None, :]).astype(np.float64))
        return np.exp(sign * np.outer(t, k))

    ex, ey = unit(tr, kr), unit(tc, kc)
    if col_phase is not None:
        ey[:, col_phase[0]] *= np.exp(1j * col_phase[1])
    out = ((g @ ey.T) * ex.T[None]).sum(axis=1)
    if wrong != "no_mean":
        moff = (lambda n: (n - 1) // 2) if wrong in ("centre", "mean_off_centre") else (lambda n: n // 2)
        axis = unit(tr, np.arange(ny) - moff(ny)).sum(axis=1) * unit(tc, np.arange(nx) - moff(nx)).sum(axis=1)
        out = out + mean[:, None] * axis[None, :]
    if wrong in ("skip_ragged", "prev_image"):
        idx = np.arange(x.size) if idx is None else np.asarray(idx)
        right = out.copy()
        for p0, np_, b0, nb, ipw in launches(n_img, x.size if n_pts_call is None else n_pts_call, chunk):
            cols_ = np.nonzero((idx >= p0) & (idx < p0 + np_))[0]
            b = np.arange(b0, b0 + nb)
            if wrong == "skip_ragged" and nb % ipw:
                out[np.ix_(b[nb - nb % ipw:], cols_)] = 0
            if wrong == "prev_image":
                late = b[(b - b0) % ipw != 0]
                out[np.ix_(late, cols_)] = right[np.ix_(late - 1, cols_)]
    return out


# -------------------------------------------------------------------------------------------------------------- the probe list

def seam_rows(ny):
    return sorted({r for k in range(1, ny // NU_T + 1) for r in (NU_T * k - 1, NU_T * k) if r < ny})


def seam_cols(nx):
    return sorted({c for c in (NU_K - 1, NU_K) if c < nx} | {c for k in range(1, nx // NU_KS + 1) for c in (NU_KS * k - 1, NU_KS * k) if c < nx})


def _side_rules(ny, nx, limit=False):
    names = ["centre", "pairing", "sign", "mean_term", "mean_centre"]
    names += ["row_tail"] if ny % NU_T else []
    names += ["col_tail"] if nx % NU_KS else []
    names += ["stage_seam"] if nx > NU_KS else []
    names += ["slice_base"] if nx > NU_K else []
    names += ["acc_rows"] if ny > 4 else []
    names += ["phase_reduction"] if limit else []
    return tuple(names)


def _delta_stack(positions):
    """One delta an image, heights 1, 2, 3, ...; positions without repeats, in order."""
    seen = []
    for pos in positions:
        if pos not in seen:
            seen.append(pos)
    return [(("delta", a, c, float(k + 1)),) for k, (a, c) in enumerate(seen)]


def _tail_images(ny, nx, constant=CONSTANT):
    return [(("const", constant),), (("row", ny - 1, ROW_VALUE),), (("col", nx - 1, COL_VALUE),), (("noise", 0, NOISE_OFFSET),)]


def _side_probe(family, ny, nx):
    pos = [(0, 0), (0, nx - 1), (ny - 1, 0), (ny - 1, nx - 1)]
    pos += [(r, min(1, nx - 1)) for r in seam_rows(ny)]
    pos += [(min(1, ny - 1), c) for c in seam_cols(nx)]
    pos += [(r, r % nx) for r in ACC_ROWS if r < ny]
    return Probe(f"{family} {ny}x{nx}", family, (ny, nx), tuple(_delta_stack(pos) + _tail_images(ny, nx)), N_POINTS, _side_rules(ny, nx))


def _cross_probe(ny, nx):
    pos = [(r, c) for r in sorted({0, ny - 1, *seam_rows(ny)}) for c in sorted({0, nx - 1, *seam_cols(nx)})]
    return Probe(f"cross {ny}x{nx}", "cross", (ny, nx), tuple(_delta_stack(pos) + _tail_images(ny, nx)), N_POINTS, _side_rules(ny, nx))


def _limit_probe(ny, nx):
    along = (0, 8191, 8192, 8193, MAX_SIDE - 1)
    pos = [(k, j % nx) for j, k in enumerate(along)] if ny == MAX_SIDE else [(j % ny, k) for j, k in enumerate(along)]
    parts = _delta_stack(pos) + [(("const", LIMIT_CONSTANT),)]
    return Probe(f"limit {ny}x{nx}", "limit", (ny, nx), tuple(parts), N_POINTS, _side_rules(ny, nx, limit=True))


def _stack_probe(label, n_img, n_pts, shape, want_ipw, extra=(), ring_group=0):
    ny, nx = shape
    parts = tuple((("delta", (b // nx) % ny, b % nx, 1.0 + b / 4),) for b in range(n_img))
    if ring_group:   # |F| of a single delta is flat: a constant under it peaks |F| at the origin, which the last point repeats
        parts = tuple(p + (("const", 0.5),) for p in parts)
    ipw = tuple(dict.fromkeys(l[4] for l in launches(n_img, n_pts)))
    assert ipw[0] == want_ipw, (label, ipw)
    return Probe(label, "ipw", shape, parts, n_pts, ("image_turn",) + tuple(extra), ipw, None, ring_group)


def _carry_probe():
    """17 images of 65 x 129 at CHUNK points: two row tiles and two stages an image, two images a workgroup, the last group
    ragged.  Noise plus a delta that walks the seams, so that what one image leaves behind (the prefetched stage, the slice
    base, the partial sums in LDS) would show in the next.  Compared at about 500 point indices, fixed here."""
    ny, nx, n_img, n_pts = 65, 129, 17, CHUNK
    where = [(r, c) for r in (0, 63, 64) for c in (0, 31, 32, 127, 128)] + [(64, 1), (1, 128)]
    parts = tuple((("noise", b + 1, 0.0), ("delta", *where[b], 8.0 + b)) for b in range(n_img))
    tiles = n_pts // NU_T
    edge = [t * NU_T + k for t in (0, 1, tiles - 1) for k in (0, NU_T - 1)]
    pick = tuple(sorted(set(edge) | set(range(0, n_pts, 67))))
    ipw = tuple(dict.fromkeys(l[4] for l in launches(n_img, n_pts)))
    assert ipw == (2,) and n_img % 2 == 1 and 480 <= len(pick) <= 520
    rules = ("image_turn", "ragged_group") + _side_rules(ny, nx)
    return Probe(f"ipw 2 ragged, {n_img} of {ny}x{nx}, {n_pts} points", "ipw", (ny, nx), parts, n_pts, rules, ipw, pick)


@functools.lru_cache(maxsize=None)
def probes():
    out = [_side_probe("rows", ny, 3) for ny in range(1, 131)]
    out += [_side_probe("columns", 3, nx) for nx in range(1, 131)]
    out += [_side_probe("seams", 2, nx) for nx in (255, 256, 257, 383, 385)]
    out += [_side_probe("seams", ny, 2) for ny in (127, 128, 129, 191, 192, 193)]
    out += [_cross_probe(65, 129), _cross_probe(129, 65)]
    out += [_limit_probe(MAX_SIDE, 3), _limit_probe(3, MAX_SIDE)]
    out += [
        _stack_probe("ipw 2 exact, 8192 of 2x3, 64 points", 8192, 64, (2, 3), 2),
        _stack_probe("ipw 2 ragged, 8193 of 2x3, 64 points", 8193, 64, (2, 3), 2, ["ragged_group"]),
        _stack_probe("ipw 3, 12288 of 2x3, 64 points", 12288, 64, (2, 3), 3),
        # one point tile reaches ipw 8 only with CHUNK images, which 8 divides: 32763 images give 7 of 4680 turns and 3 over
        _stack_probe("ipw 7 ragged, 32763 of 1x1, 64 points", 32763, 64, (1, 1), 7, ["ragged_group"]),
        _stack_probe("ipw 8 ragged, 16387 of 1x1, 65 points", 16387, 65, (1, 1), 8, ["ragged_group"]),
        _stack_probe("ipw 2 ragged, 4097 of 2x3, 65 points", 4097, 65, (2, 3), 2, ["ragged_group"]),
        _carry_probe(),
        _stack_probe(f"ring 7, ipw 2 ragged, 17 of 2x3, {CHUNK + 1} points", 17, CHUNK + 1, (2, 3), 2,
                     ["ragged_group", "ring_index", "mean_term"], ring_group=7),
    ]
    assert len({p.label for p in out}) == len(out)
    return tuple(out)


def by_label(label):
    return next(p for p in probes() if p.label == label)


def families():
    return tuple(dict.fromkeys(p.family for p in probes()))


@functools.lru_cache(maxsize=8)
def _images(label):
    probe = by_label(label)
    ny, nx = probe.shape
    lone = all(len(p) == 1 and p[0][0] == "delta" for p in probe.parts)
    if lone:
        out = np.zeros((len(probe.parts), ny, nx), np.float64)
        b = np.arange(len(probe.parts))
        out[b, [p[0][1] for p in probe.parts], [p[0][2] for p in probe.parts]] = [p[0][3] for p in probe.parts]
    else:
        out = np.stack([sum(part_image(part, probe.shape) for part in parts) for parts in probe.parts])
    f = out.astype(np.float32)
    closed = [b for b, parts in enumerate(probe.parts) if all(part[0] != "noise" for part in parts)]
    assert np.array_equal(f[closed].astype(np.float64), out[closed])      # every closed-form value is one float32 holds
    f.setflags(write=False)
    return f


@functools.lru_cache(maxsize=8)
def _points(label):
    probe = by_label(label)
    x, y = Y.points(probe.n_pts)
    if probe.ring_group:
        x[-1] = y[-1] = 0.0
    x.setflags(write=False)
    y.setflags(write=False)
    return x, y
