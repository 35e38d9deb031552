"""Shared by tests/test_reduction_probes_host.py and tests/test_gpu_reduction_probes.py: the probe table of the score,
arg-max and threshold reductions (k_pair_sums behind pearson / cosine, k_argmax_rows and its host twin hh_argmax, k_array_max /
k_threshold behind hh_threshold_data, all in csrc/helicon_hip.hip), each probe's reference, the comparison both tests apply, and
the wrong-rule variants the host test uses to show that a comparison would notice a defect.  CPU only: nothing here imports the
device package.

A probe names the kernel and rule it aims at (``rule``), its input (``inputs()``, seeded by the probe's name) and the call
(``kind`` + ``args``).

kind             call on the device                                                   reference
pearson          helicon_amd.cross_correlation_coefficient(a, b)                      pair_yardstick: math.fsum of float64 terms
cosine           helicon_amd.cosine_similarity(a, b)                                  pair_yardstick
argmax           hh_argmax_device(scores [rows][ld], rows, n, ld) -> d_index/h_index  argmax_numpy, row by row
argmax_host      hh_argmax(row, n), one row at a time (host code: runs anywhere)      argmax_numpy
argmax_refusal   hh_argmax_device with a bad argument, then a good call               ("refused", argmax_numpy of the good call)
threshold        SweepEngine.threshold_data(data, thresh_fraction / thresh_value)     threshold_numpy: float32 NumPy

The decomposition the kernels use, which the seams below are read from: wavefronts of 64 lanes; k_pair_sums, k_array_max and
k_threshold run min(1024, ceil(n / 256)) blocks of 256 lanes in a grid-stride loop, so one trip covers up to 262144 elements
and element 262144 is the first of the second trip; k_argmax_rows runs one block of 1024 lanes (16 wavefronts) per row, thread t
reading t, t + 1024, ... in ascending order, and takes at most 65535 rows.

The pair-score bound, derived (u = 2^-53):  the kernel adds each of its sums in float64 along chains no longer than
K(n) = ceil(n / (256 grid)) + 10 + grid additions — ceil(n / (256 grid)) trips in one thread, 6 shuffle steps and 4 LDS terms
(the 10), and the host's sum over `grid` blocks — so each sum S of terms t_i comes out with |error| <= K u sum |t_i| to first
order (the rounding of each product, one more u per term, is inside the slack below).  sxx and syy have positive terms: their
relative error is <= K u.  By Cauchy-Schwarz sum |p q| <= sqrt(sxx syy), so sxy carries an absolute error <= K u sqrt(sxx syy).
The score r = sxy / sqrt(sxx syy) therefore moves by <= K u (from sxy) + |r| K u (half from each of sxx and syy under the
root) <= 2 K u, plus 3 u for the root, the product and the quotient.  The means are exact to first order in the centred
sums: a mean off by d changes sxx by n d^2 and sxy by n dx dy, and d <= K u max |x|, far below u sxx.  The yardstick's own
terms are rounded once each (u per term, 3 u on the quotient) and then summed exactly.  |got - want| <= 8 K(n) u leaves a
factor of about 4 over 2 K u for all of that; it is 9.2e-13 at n = 2 * 262144 + 7, in line with the 1e-12 of
test_cc_and_cosine_known_answers_and_golden.  Arg-max and threshold results are compared exactly (threshold: bit for bit,
NaN positions included)."""
import math
import zlib
from dataclasses import dataclass, field
from functools import lru_cache

import numpy as np

from oracle import path_b as O

F32, F64 = np.float32, np.float64
LANES, PAIR_BLOCK, GRID_CAP, ARG_BLOCK, ROW_CAP = 64, 256, 1024, 1024, 65535
TRIP = PAIR_BLOCK * GRID_CAP                      # 262144 elements per grid-stride trip of the capped grid
U = 2.0 ** -53
LENGTHS = (1, 2, 3, 63, 64, 65, 255, 256, 257, 511, 513, TRIP - 1, TRIP, TRIP + 1, TRIP + 257, 2 * TRIP + 7)
SEAMS = (0, 63, 64, 255, 256, TRIP - 1, TRIP)    # + n - 1: lane, wavefront, block and grid-stride boundaries
ARG_ROWS = (1, 5)
ARG_N = (1, 2, 63, 64, 65, 1023, 1024, 1025, 2047, 2049, 100003)
ARG_SEAMS = (0, 63, 64, 1023, 1024)               # + n - 1
FRACTIONS = (0.0, 0.3, 0.5, 1.0)
VALUES = (0.5, -0.25)


@dataclass(frozen=True)
class Probe:
    name: str
    kind: str
    rule: str                      # "kernel: the rule the probe reaches"
    make: object                   # () -> dict of input arrays
    args: dict = field(default_factory=dict)

    def inputs(self):
        return self.make()


def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def grid_of(n):
    return min(GRID_CAP, -(-n // PAIR_BLOCK))


def trips_of(n):
    return -(-n // (PAIR_BLOCK * grid_of(n)))


def chain_length(n):
    """K(n) of the module docstring."""
    return trips_of(n) + 10 + grid_of(n)


def pair_bound(n):
    return 8.0 * chain_length(n) * U


def place_of(i, n):
    """(trip, block, wavefront in the block, lane) of element i in the grid-stride kernels."""
    stride = PAIR_BLOCK * grid_of(n)
    t = i % stride
    return i // stride, t // PAIR_BLOCK, (t % PAIR_BLOCK) // LANES, t % LANES


def seams_below(n, seams=SEAMS):
    return sorted({i for i in seams + (n - 1,) if 0 <= i < n})


# ---------------------------------------------------------------------------------------------------------- pearson / cosine
def _noise(name, n, dt):
    r = _rng(name)
    z = r.normal(size=n)
    x64, y64 = 4096.0 + z, 0.3 * z + r.normal(size=n) - 77.0
    x, y = x64.astype(F32), y64.astype(F32)
    if dt == "f32":
        return dict(a=x, b=y)
    x64, y64 = x64 * (1 + 1e-9), y64 * (1 + 1e-9)            # full float64 mantissas: rounding them to float32 moves every element
    return dict(a=x, b=y64) if dt == "mixed" else dict(a=x64, b=y64)


def _spike(n, i):
    ramp = (np.arange(n) / n - 0.5).astype(F32)
    x, y = ramp.copy(), -ramp
    x[i] = y[i] = F32(4.0 * math.sqrt(n))
    return dict(a=x, b=y)


def _affine(name, n, alpha, beta):
    x = _rng(name).normal(size=n).astype(F32).astype(F64)
    return dict(a=x, b=alpha * x + beta)          # exact: x has 24 bits, alpha a power of two, beta a small integer


def _orthogonal(n):
    k = np.arange(n)
    return dict(a=np.where(k % 4 < 2, 1.0, -1.0).astype(F32), b=np.where(k % 2 == 0, 1.0, -1.0).astype(F32))


def _constant(name, n, dt):
    x = _noise(name, n, dt)["a"]
    return dict(a=x, b=np.full(n, 2.5, dtype=x.dtype))


def _scaled(name, n, scale):
    r = _rng(name)
    z = r.normal(size=n)
    return dict(a=z * scale, b=(0.3 * z + r.normal(size=n)) * scale)


def _masked(name):
    r = _rng(name)
    p, q = r.random((64, 64)), r.random((64, 64))
    m = O.radial_band_mask(64, 64)
    return dict(a=p[m], b=q[m])                   # the masked idiom of lib/alignment.py:144-147


def _view2d(name):
    r = _rng(name)
    p, q = r.normal(size=(80, 48)).astype(F32), r.normal(size=(80, 48)).astype(F32)
    return dict(a=p.T, b=q.T)                     # 2-D, not contiguous: flattened in the view's own row-major order


def _pair_probes():
    out = []

    def add(kind, tag, n, dt, rule, make, **args):
        name = f"{kind}/{tag}/n{n}/{dt}"
        out.append(Probe(name, kind, rule, (lambda name=name: make(name)), dict(n=n, **args)))

    for kind in ("pearson", "cosine"):
        entry = "hh_cross_correlation" if kind == "pearson" else "hh_cosine_similarity"
        for n in LENGTHS:
            zero = kind == "pearson" and n == 1
            where = f"grid {grid_of(n)}, {trips_of(n)} trip(s), tail {n % PAIR_BLOCK}"
            add(kind, "noise", n, "f32", f"k_pair_sums<float> via {entry}: every element once ({where})" + ("; n = 1 gives 0" if zero else ""),
                lambda name, n=n: _noise(name, n, "f32"), exact_zero=zero)
            add(kind, "noise", n, "f64", f"k_pair_sums<double> via {entry}_f64: float64 inputs kept ({where})" + ("; n = 1 gives 0" if zero else ""),
                lambda name, n=n: _noise(name, n, "f64"), exact_zero=zero)
            spike_lengths = LENGTHS if kind == "pearson" else (257, 2 * TRIP + 7)
            if n >= 2 and n in spike_lengths:
                for i in seams_below(n):
                    t, b, w, l = place_of(i, n)
                    add(kind, f"spike{i}", n, "f32", f"k_pair_sums: element {i} (trip {t}, block {b}, wavefront {w}, lane {l}) read exactly once",
                        lambda name, n=n, i=i: _spike(n, i), spike=i)
        add(kind, "noise", TRIP + 1, "mixed", f"_pair: a float32 / float64 pair goes through {entry}_f64",
            lambda name: _noise(name, TRIP + 1, "mixed"), exact_zero=False)
        for n in (3, 257, TRIP + 1):
            beta = 3.0 if kind == "pearson" else 0.0
            add(kind, "affine_plus", n, "f64", "k_pair_sums: y = 2 x + b gives +1", lambda name, n=n, beta=beta: _affine(name, n, 2.0, beta), closed=1.0)
            add(kind, "affine_minus", n, "f64", "k_pair_sums: y = -x / 2 + b gives -1", lambda name, n=n, beta=beta: _affine(name, n, -0.5, beta), closed=-1.0)
        for n in (64, 256, TRIP):
            add(kind, "orthogonal", n, "f32", "k_pair_sums: orthogonal +-1 patterns give exactly 0", lambda name, n=n: _orthogonal(n), exact_zero=True, closed=0.0)
        add(kind, "masked", int(O.radial_band_mask(64, 64).sum()), "f64", "the masked idiom p[m], q[m] of 2-D float64 inputs", _masked)
        add(kind, "view2d", 48 * 80, "f32", "_pair: a non-contiguous 2-D input is flattened in its own row-major order", _view2d)
        # sqrt(sxx syy) (Pearson, analysis.py:796) against sqrt(sxx) sqrt(syy) (cosine, np.linalg.norm twice): they part where the product
        # of the two sums leaves the float64 range
        add(kind, "huge", 257, "f64", ("pearson: sqrt(sxx syy) overflows, the score is 0 as in the reference" if kind == "pearson" else
                                        "cosine: sqrt(sxx) sqrt(syy) does not overflow"), lambda name: _scaled(name, 257, 1e100))
        add(kind, "tiny", 257, "f64", ("pearson: sxx syy underflows to 0, norm == 0 gives 0 as in the reference" if kind == "pearson" else
                                        "cosine: sqrt(sxx) sqrt(syy) does not underflow"), lambda name: _scaled(name, 257, 1e-100),
            exact_zero=kind == "pearson")
    for n in (3, 257, TRIP + 1, 2 * TRIP + 7):
        for dt in ("f32", "f64"):
            add("pearson", "constant", n, dt, "pearson: a constant operand gives exactly 0 (its float64 mean is exact)",
                lambda name, n=n, dt=dt: _constant(name, n, dt), exact_zero=True)
    for n in (1, 257, TRIP + 1):
        add("cosine", "zero_vector", n, "f32", "cosine: the zero vector gives exactly 0",
            lambda name, n=n: dict(a=_noise(name, n, "f32")["a"], b=np.zeros(n, F32)), exact_zero=True)
    return out


def _fsum(v):
    return math.fsum(np.asarray(v, dtype=F64).tolist())


def pair_yardstick(kind, a, b):
    """The score of the inputs as the device receives them, cast exactly to float64: means and the three centred sums by
    math.fsum; norm == 0 -> 0; Pearson's norm is sqrt(sxx syy), cosine's sqrt(sxx) sqrt(syy), as in the reference."""
    x, y = np.asarray(a).astype(F64).ravel(), np.asarray(b).astype(F64).ravel()
    n = x.size
    if kind == "pearson":
        x, y = x - _fsum(x) / n, y - _fsum(y) / n
    sxx, syy, sxy = _fsum(x * x), _fsum(y * y), _fsum(x * y)
    norm = math.sqrt(sxx * syy) if kind == "pearson" else math.sqrt(sxx) * math.sqrt(syy)
    return 0.0 if norm == 0 else sxy / norm


@lru_cache(maxsize=None)
def _pair_reference(name):
    p = BY_NAME[name]
    inp = p.inputs()
    return pair_yardstick(p.kind, inp["a"], inp["b"])


def _pair_reduce(x, y, mx, my, *, drop_tail=False, max_trips=None, waves=PAIR_BLOCK // LANES):
    """pair_reduce + k_pair_sums in NumPy: the five sums in the kernel's own order of float64 additions."""
    n = x.size
    grid = grid_of(n)
    stride, trips = grid * PAIR_BLOCK, trips_of(n)
    p, q = x - mx, y - my
    terms = np.zeros((5, trips * stride))
    terms[:, :n] = np.stack([p, q, p * p, q * q, p * q])
    if drop_tail:
        terms[:, n - n % PAIR_BLOCK:] = 0.0
    terms = terms.reshape(5, trips, grid, PAIR_BLOCK // LANES, LANES)
    acc = np.zeros_like(terms[:, 0])
    for t in range(trips if max_trips is None else min(trips, max_trips)):       # one thread, ascending
        acc = acc + terms[:, t]
    off = LANES // 2
    while off:                                                                   # __shfl_down tree: lane 0 ends with the sum
        acc[..., :off] = acc[..., :off] + acc[..., off:2 * off]
        off //= 2
    r = np.zeros((5, grid))
    for k in range(waves):                                                       # the LDS sum over the block's wavefronts
        r = r + acc[..., k, 0]
    out = np.zeros(5)
    for g in range(grid):                                                        # the host's sum over blocks
        out = out + r[:, g]
    return out


def pair_kernel_numpy(kind, a, b, *, single_pass=False, round_f32=False, norm_rule=None, **rules):
    """pearson() / cosine() of helicon_hip.hip restated: with no rule changed it is the device's arithmetic up to FMA
    contraction (the yardstick to well inside the bound); each keyword changes one rule."""
    x, y = np.asarray(a).ravel(), np.asarray(b).ravel()
    if round_f32:
        x, y = x.astype(F32), y.astype(F32)
    x, y = x.astype(F64), y.astype(F64)
    n = x.size
    s = _pair_reduce(x, y, 0.0, 0.0, **rules)
    if kind == "pearson":
        mx, my = s[0] / n, s[1] / n
        if single_pass:
            s = np.array([0, 0, s[2] - n * mx * mx, s[3] - n * my * my, s[4] - n * mx * my])
        else:
            s = _pair_reduce(x, y, mx, my, **rules)
    norm_rule = norm_rule or ("product" if kind == "pearson" else "separate")
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        norm = np.sqrt(s[2] * s[3]) if norm_rule == "product" else np.sqrt(s[2]) * np.sqrt(s[3])
        return 0.0 if norm == 0 else float(s[4] / norm)


# ---------------------------------------------------------------------------------------------------------------- arg-max
def argmax_cases(n):
    """The rows a length-n probe can carry: (tag, positions...)."""
    c = [("max", i) for i in seams_below(n, ARG_SEAMS)] + [("all_nan",), ("ninf_all",)]
    if n >= 2:
        c.append(("tie", 10, 11) if n >= 12 else ("tie", 0, 1))               # within a wavefront
        c += [("tie", a, b) for a, b in ((63, 64), (5, 1029), (1023, 1024)) if b < n]  # across wavefronts; one thread's trips; the block's ends
        a, b = (3, 70) if n > 70 else (0, n - 1)
        c += [("zeros_pm", a, b), ("zeros_mp", a, b), ("inf_tie", a, b), ("nan0_equal",), ("nan_ninf", min(65, n - 1)),
              ("nan_after_max", min(63, n - 2))]
    return c


CASE_RULE = {"max": "the maximum at {0}", "tie": "equal maxima at {0} and {1}: the lower index", "zeros_pm": "+0.0 at {0} ties -0.0 at {1}: the lower index",
             "zeros_mp": "-0.0 at {0} ties +0.0 at {1}: the lower index", "inf_tie": "+inf at {0} and {1}: the lower index", "all_nan": "all NaN gives 0",
             "ninf_all": "all -inf gives 0", "nan0_equal": "NaN at 0, then equal values: 1", "nan_ninf": "NaN and -inf: the first -inf, {0}",
             "nan_after_max": "NaN right after the maximum at {0}"}


def _case_tag(case):
    return "_".join(str(v) for v in case)


def argmax_row(case, n, rng):
    """(row, the index the rule gives) of one case."""
    tag, pos = case[0], case[1:]
    row = np.clip(0.5 * rng.normal(size=n), -3, 3).astype(F32)
    if tag == "max":
        row[pos[0]] = 9
    elif tag == "tie":
        row[list(pos)] = 9
    elif tag in ("zeros_pm", "zeros_mp"):
        row = -np.abs(row) - 1
        row[pos[0]], row[pos[1]] = (0.0, -0.0) if tag == "zeros_pm" else (-0.0, 0.0)
    elif tag == "inf_tie":
        row[list(pos)] = np.inf
    elif tag == "all_nan":
        row[:] = np.nan
        return row, 0
    elif tag == "ninf_all":
        row[:] = -np.inf
        return row, 0
    elif tag == "nan0_equal":
        row[:] = 2
        row[0] = np.nan
        return row, 1
    elif tag == "nan_ninf":
        row[:] = np.nan
        row[pos[0]::3] = -np.inf
    elif tag == "nan_after_max":
        row[pos[0]] = 9
        row[pos[0] + 1] = np.nan
    else:
        raise KeyError(tag)
    return row, min(pos)


def _argmax_scores(name, cases, n, ld):
    """[rows][ld or n]: row r carries cases[r]; the padding beyond n holds +inf and NaN sentinels."""
    rng = _rng(name)
    width = ld or n
    s = np.empty((len(cases), width), dtype=F32)
    s[:, n:] = np.where(np.arange(width - n) % 2 == 0, np.inf, np.nan).astype(F32)
    expect = np.empty(len(cases), dtype=np.int64)
    for r, case in enumerate(cases):
        s[r, :n], expect[r] = argmax_row(case, n, rng)
    return dict(scores=s, expect=expect)


def _argmax_probes():
    out = []

    def add(kind, rows, n, ld, route, tag, cases):
        name = f"{kind}/r{rows}/n{n}/ld{ld}/{route}/{tag}"
        kern = "k_argmax_rows" if kind == "argmax" else "hh_argmax"
        said = sorted({CASE_RULE[c[0]].format(*c[1:]) for c in cases})
        rule = f"{kern}: " + "; ".join(said[:6]) + (f"; ... ({len(said)} row rules)" if len(said) > 6 else "")
        if ld:
            rule += f"; ld = {ld} > n with +inf / NaN in the padding"
        if kind == "argmax":
            rule += f"; indices through {'a caller buffer' if route == 'd' else 'h_index'}"
        out.append(Probe(name, kind, rule, (lambda name=name: _argmax_scores(name, cases, n, ld)), dict(n=n, ld=ld, route=route, cases=tuple(cases))))

    for n in ARG_N:
        cases = argmax_cases(n)
        for k, case in enumerate(cases):                                         # one row
            add("argmax", 1, n, 0, "hd"[k % 2], _case_tag(case), [case])
            add("argmax_host", 1, n, 0, "h", _case_tag(case), [case])
        groups = [[cases[(g + k) % len(cases)] for k in range(5)] for g in range(0, len(cases), 5)]
        for g, group in enumerate(groups):                                       # five rows, dense and strided
            for j, ld in enumerate((0, n + 1, n + 37)):
                add("argmax", 5, n, ld, "dh"[(g + j) % 2], f"g{g}", group)
            add("argmax_host", 5, n, 0, "h", f"g{g}", group)
    cases3 = argmax_cases(3)
    cap = [cases3[r % len(cases3)] for r in range(ROW_CAP)]                      # the documented cap on rows
    add("argmax", ROW_CAP, 3, 0, "h", "cap", cap)
    add("argmax", ROW_CAP, 3, 4, "d", "cap", cap)
    add("argmax_host", ROW_CAP, 3, 0, "h", "cap", cap)
    for tag, bad, why in (("rows65536", (ROW_CAP + 1, 5, 0), "n_rows = 65536 is refused"), ("ld_below_n", (2, 5, 4), "ld < n is refused"),
                          ("n0", (2, 0, 0), "n = 0 is refused")):
        name = f"argmax_refusal/{tag}"
        good = [("max", 4), ("tie", 1, 3)]
        out.append(Probe(name, "argmax_refusal", f"hh_argmax_device: {why}, and the next call on the context is served",
                         (lambda name=name, good=good: _argmax_scores(name, good, 5, 0)), dict(bad=bad, n=5, ld=0, route="h", cases=tuple(good))))
    return out


def argmax_numpy(scores, n):
    """The project's rule, row by row: NaN never wins, the lowest index wins among equal maxima, nothing valid gives 0."""
    s = np.asarray(scores)[:, :n]
    out = np.zeros(s.shape[0], dtype=np.int64)
    valid = ~np.isnan(s)
    some = valid.any(axis=1)
    with np.errstate(invalid="ignore"):
        top = np.max(np.where(valid, s, -np.inf), axis=1)
        out[some] = np.argmax(valid[some] & (s[some] == top[some, None]), axis=1)
    return out


def argmax_kernel_numpy(scores, n, ld=0, *, waves=ARG_BLOCK // LANES, thread_rule="first", wave_rule="lower", block_rule="lower", nan_wins=False,
                        stride_as_n=False, length_as_ld=False, none_valid=0):
    """k_argmax_rows in NumPy: thread t of 1024 reads t, t + 1024, ... ascending and keeps its first maximum; a __shfl_down tree
    over each 64-lane wavefront and thread 0's loop over the wavefronts prefer the lower index among equals.  Each keyword
    changes one rule."""
    s = np.asarray(scores, dtype=F32)
    rows, flat = s.shape[0], s.ravel()
    step = n if (stride_as_n or not ld) else ld
    m = (ld or n) if length_as_ld else n
    R = flat[np.arange(rows)[:, None] * step + np.arange(m)[None, :]]
    trips = -(-m // ARG_BLOCK)
    V = np.full((rows, trips * ARG_BLOCK), np.nan, dtype=F32)
    V[:, :m] = R
    V = V.reshape(rows, trips, ARG_BLOCK)
    real = (np.arange(trips * ARG_BLOCK) < m).reshape(trips, ARG_BLOCK)
    I = np.arange(trips * ARG_BLOCK, dtype=np.int64).reshape(trips, ARG_BLOCK)

    def gt(v, w):
        with np.errstate(invalid="ignore"):
            return (v > w) | (np.isnan(v) & ~np.isnan(w)) if nan_wins else v > w

    def eq(v, w):
        with np.errstate(invalid="ignore"):
            return (v == w) | (np.isnan(v) & np.isnan(w)) if nan_wins else v == w

    def better(ov, oi, bv, bi, rule):
        tie = oi < bi if rule == "lower" else oi > bi
        return (oi >= 0) & ((bi < 0) | gt(ov, bv) | (eq(ov, bv) & tie))

    bv = np.full((rows, ARG_BLOCK), -np.inf, dtype=F32)
    bi = np.full((rows, ARG_BLOCK), -1, dtype=np.int64)
    for t in range(trips):
        v, i = V[:, t], np.broadcast_to(I[t], (rows, ARG_BLOCK))
        ok = real[t][None, :] & (nan_wins | ~np.isnan(v))
        take = ok & ((bi < 0) | gt(v, bv) | ((thread_rule == "last") & eq(v, bv)))
        bv, bi = np.where(take, v, bv), np.where(take, i, bi)
    bv, bi = bv.reshape(rows, -1, LANES).copy(), bi.reshape(rows, -1, LANES).copy()
    off = LANES // 2
    while off:
        take = better(bv[..., off:2 * off], bi[..., off:2 * off], bv[..., :off], bi[..., :off], wave_rule)
        bv[..., :off] = np.where(take, bv[..., off:2 * off], bv[..., :off])
        bi[..., :off] = np.where(take, bi[..., off:2 * off], bi[..., :off])
        off //= 2
    fv, fi = bv[:, 0, 0], bi[:, 0, 0]
    for k in range(1, waves):
        take = better(bv[:, k, 0], bi[:, k, 0], fv, fi, block_rule)
        fv, fi = np.where(take, bv[:, k, 0], fv), np.where(take, bi[:, k, 0], fi)
    return np.where(fi < 0, none_valid, fi).astype(np.int64)


# -------------------------------------------------------------------------------------------------------------- threshold
def _thr_data(name, tag, n, pos=None):
    r = _rng(name)
    if tag == "pos":
        x = r.uniform(0.5, 2.0, n)
    elif tag == "mixed":
        x = r.normal(size=n)
    elif tag == "neg":
        x = r.uniform(-2.0, -0.5, n)
    elif tag == "neg_zero":
        x = r.uniform(-2.0, -0.5, n)
        x[n // 2] = 0.0
    elif tag == "zeros":
        x = np.zeros(n)
    elif tag == "negzero_max":                                   # n = 2: [-1, -0.0]
        x = np.full(n, -1.0)
        x[n - 1] = -0.0
    elif tag == "all_negzero":
        x = np.full(n, -0.0)
    elif tag == "wave_neg":                                      # the first wavefront holds negative values only
        x = r.uniform(0.5, 2.0, n)
        first = np.arange(n) % (PAIR_BLOCK * grid_of(n)) < LANES    # its elements of every trip
        x[first] = r.uniform(-2.0, -0.5, int(first.sum()))
    elif tag == "max":
        x = r.uniform(-1.0, 0.5, n)
        x[pos] = 3.0
    elif tag == "negmax":
        x = r.uniform(-3.0, -2.25, n)                            # (half of anything here is below -1: a maximum that is missed shows)
        x[pos] = -1.0
    elif tag == "nan":
        x = r.normal(size=n)
        x[pos] = np.nan
    else:
        raise KeyError(tag)
    return dict(data=x.astype(F32))


THR_RULE = {"pos": "all positive", "mixed": "both signs", "neg": "all negative: the maximum is the negative value nearest 0",
            "neg_zero": "negative values and exactly one +0.0", "zeros": "all zeros", "negzero_max": "a maximum of -0.0 among negative values",
            "all_negzero": "every element -0.0", "wave_neg": "one wavefront negative-only while others hold the positive maximum"}


def _threshold_probes():
    out = []

    def add(tag, n, mode, thresh, rule, pos=None):
        name = f"threshold/{tag}{'' if pos is None else pos}/n{n}/{mode}{thresh:g}"
        kern = "k_array_max / k_threshold" if mode == "fraction" else "k_threshold"
        out.append(Probe(name, "threshold", f"{kern}: {rule} (grid {grid_of(n)}, {trips_of(n)} trip(s), tail {n % PAIR_BLOCK})",
                         (lambda name=name: _thr_data(name, tag, n, pos)), dict(n=n, mode=mode, thresh=thresh, tag=tag, pos=pos)))

    modes = [("fraction", f) for f in FRACTIONS] + [("value", v) for v in VALUES]
    for n in LENGTHS:
        for tag in THR_RULE:
            if (tag == "wave_neg" and n <= LANES) or (tag == "negzero_max" and n < 2):
                continue
            for mode, t in modes:
                add(tag, n, mode, t, THR_RULE[tag])
        for i in seams_below(n):
            trip, b, w, l = place_of(i, n)
            where = f"at {i} (trip {trip}, block {b}, wavefront {w}, lane {l})"
            add("max", n, "fraction", 0.5, f"the maximum {where}, everything else lower", i)
            add("negmax", n, "fraction", 0.5, f"the negative maximum {where}, everything else lower", i)
        for i in seams_below(n, (0, 64, TRIP)):
            add("nan", n, "fraction", 0.5, f"one NaN at {i}: the maximum is NaN, every output is NaN", i)
            add("nan", n, "value", 0.5, f"one NaN at {i}: NaN at that position only", i)
    return out


def threshold_numpy(data, mode, thresh, *, vmax=None, launder=False, fraction_f64=False, drop_tail=False):
    """np.clip(data, t, None) - t in float32, t = float32(max) float32(fraction) (fraction mode) or float32(value).  The
    keywords restate wrong rules: another maximum, fmaxf for the clip, the fraction applied in float64, the last n % 256 left out."""
    x = np.asarray(data, dtype=F32)
    if mode == "fraction":
        head = x[:x.size - x.size % PAIR_BLOCK] if drop_tail and x.size >= PAIR_BLOCK else x
        m = F32(np.max(head)) if vmax is None else F32(vmax(head))
        with np.errstate(invalid="ignore"):
            t = F32(F64(m) * F64(thresh)) if fraction_f64 else m * F32(thresh)
    else:
        t = F32(thresh)
    with np.errstate(invalid="ignore"):
        out = (np.fmax(x, t) if launder else np.clip(x, t, None)) - t
    if drop_tail and mode == "fraction":
        out[x.size - x.size % PAIR_BLOCK:] = -1.0                # never written
    return out.astype(F32)


def wavefront_maxima(x):
    """The maximum each 64-lane wavefront of k_array_max ends with (NaN dropped, as fmaxf does): element i belongs to thread
    i mod (256 grid).  Wavefronts without an element are left out."""
    n = x.size
    stride = PAIR_BLOCK * grid_of(n)
    wave = (np.arange(n) % stride) // LANES
    out = np.full(stride // LANES, -np.inf, dtype=F32)
    with np.errstate(invalid="ignore"):
        np.fmax.at(out, wave, x)
    return out[np.unique(wave)]


def max_by_key(x):
    """k_array_max restated: one unsigned key per value that orders like the floats (sign bit set for a cleared sign, all bits
    inverted for a set one; 0xFFFFFFFF for a NaN), the largest key over the wavefronts, decoded."""
    x = np.ascontiguousarray(x, dtype=F32)
    u = x.view(np.uint32)
    key = np.where(np.isnan(x), np.uint32(0xFFFFFFFF), np.where(u >> 31 != 0, ~u, u | np.uint32(0x80000000))).astype(np.uint32)
    stride = PAIR_BLOCK * grid_of(x.size)
    waves = np.zeros(stride // LANES, dtype=np.uint32)
    np.maximum.at(waves, (np.arange(x.size) % stride) // LANES, key)
    k = waves.max()                                              # (a wavefront without an element keeps key 0, below every value's)
    bits = k ^ np.uint32(0x80000000) if k & np.uint32(0x80000000) else ~k
    return np.array([bits], dtype=np.uint32).view(F32)[0]


def _max_nan_dropped(x):
    """fmaxf all the way: a NaN never enters the maximum (-inf, the start value, where nothing else is there)."""
    v = x[~np.isnan(x)]
    return v.max() if v.size else F32(-np.inf)


def _max_signed_negative(x):
    """Negative maxima ordered as signed integers: the bits of a negative float grow with its magnitude."""
    m = np.max(x)
    return np.min(x) if m < 0 else m


def _max_negzero_unrecorded(x):
    """Two slots, non-negative maxima by signed atomicMax from INT_MIN and negative ones by unsigned atomicMin from 0xFFFFFFFF,
    with `m >= 0` sending -0.0 to the first slot: its bits ARE INT_MIN, so nothing is recorded and the second slot is read."""
    w = wavefront_maxima(x)
    recorded = w[(w > 0) | ((w == 0) & ~np.signbit(w))]
    if recorded.size:
        return recorded.max()
    negative = w[w < 0]
    return negative.max() if negative.size else F32(np.nan)


# ---------------------------------------------------------------------------------------------------------------- the table
PROBES = tuple(_pair_probes() + _argmax_probes() + _threshold_probes())
BY_NAME = {p.name: p for p in PROBES}
assert len(BY_NAME) == len(PROBES)


def reference(probe, inp=None):
    k, a = probe.kind, probe.args
    if k in ("pearson", "cosine"):
        return _pair_reference(probe.name)                     # (inputs are a function of the name: computed once)
    inp = probe.inputs() if inp is None else inp
    if k in ("argmax", "argmax_host"):
        return argmax_numpy(inp["scores"], a["n"])
    if k == "argmax_refusal":
        return ("refused", argmax_numpy(inp["scores"], a["n"]))
    if k == "threshold":
        return threshold_numpy(inp["data"], a["mode"], a["thresh"])
    raise KeyError(k)


# ---------------------------------------------------------------------------------------------------------- the comparison
@dataclass
class Verdict:
    figure: float          # the largest difference of a compared number (0 for a purely exact comparison)
    bound: float           # what the figure is held to (0: exact)
    mismatches: int        # exactly compared items that differ (indices, bit patterns, NaN positions, exact zeros, refusals)
    ok: bool
    note: str = ""

    def bitten(self):
        """What the host test asks of a wrong-rule variant: an exact item changed, or a number moved by 100 bounds."""
        return self.mismatches > 0 or (self.bound > 0 and self.figure >= 100.0 * self.bound)


def compare(probe, got, want, inp=None):
    k, a = probe.kind, probe.args
    if k in ("pearson", "cosine"):
        bound = pair_bound(a["n"])
        g, w = float(got), float(want)
        if math.isnan(g) or math.isnan(w):
            bad = int(math.isnan(g) != math.isnan(w))
            return Verdict(0.0, bound, bad, bad == 0, "NaN")
        fig = abs(g - w)
        exact = int(a.get("exact_zero", False) and g != 0)
        return Verdict(fig, bound, exact, exact == 0 and fig <= bound, "exactly 0 asked" if a.get("exact_zero") else "")
    if k in ("argmax", "argmax_host"):
        g, w = np.asarray(got), np.asarray(want)
        bad = int((g != w).sum()) if g.shape == w.shape else max(1, w.size)
        return Verdict(0.0, 0.0, bad, bad == 0)
    if k == "argmax_refusal":
        g, w = np.asarray(got[1]), np.asarray(want[1])
        bad = int(got[0] != want[0]) + (int((g != w).sum()) if g.shape == w.shape else max(1, w.size))
        return Verdict(0.0, 0.0, bad, bad == 0)
    if k == "threshold":
        g, w = np.asarray(got), np.asarray(want)
        if g.shape != w.shape or g.dtype != F32 or w.dtype != F32:
            return Verdict(np.inf, 0.0, max(1, w.size), False, "shape or dtype")
        nan = np.isnan(g) | np.isnan(w)
        bad = int((np.isnan(g) != np.isnan(w)).sum()) + int((g.view(np.uint32) != w.view(np.uint32))[~nan].sum())
        return Verdict(0.0, 0.0, bad, bad == 0, f"NaN positions {int(np.isnan(w).sum())}")
    raise KeyError(k)


# ------------------------------------------------------------------------------------------------- the wrong-rule variants
def _pair_variant(**kw):
    return lambda probe, inp: pair_kernel_numpy(probe.kind, inp["a"], inp["b"], **kw)


def _argmax_variant(**kw):
    return lambda probe, inp: argmax_kernel_numpy(inp["scores"], probe.args["n"], probe.args["ld"], **kw)


def _threshold_variant(**kw):
    return lambda probe, inp: threshold_numpy(inp["data"], probe.args["mode"], probe.args["thresh"], **kw)


def _names(prefix, *contains, where=None):
    return tuple(p.name for p in PROBES if p.name.startswith(prefix) and all(c in p.name for c in contains) and (where is None or where(p)))


@dataclass(frozen=True)
class Variant:
    rule: str          # the one rule changed
    run: object        # (probe, inputs) -> what the device would return under the wrong rule
    probes: tuple      # the probes listed for it: at least one must be bitten


def _small(p):
    return p.args["n"] <= 1025


VARIANTS = {
    "pair: the tail n % 256 dropped": Variant("k_pair_sums grid-stride bound i < n", _pair_variant(drop_tail=True),
                                              _names("pearson/spike", where=lambda p: p.args["spike"] == p.args["n"] - 1 and p.args["n"] % 256)),
    "pair: the second grid-stride trip dropped": Variant("k_pair_sums i += gridDim.x * blockDim.x", _pair_variant(max_trips=1),
                                                         _names("pearson/spike262144/") + _names("cosine/spike262144/")),
    "pair: the fourth wavefront left out of the LDS sum": Variant("k_pair_sums red[k], k < blockDim.x / 64", _pair_variant(waves=3),
                                                                  _names("pearson/spike255/") + _names("pearson/noise/n256/")),
    "pair: single-pass raw moments": Variant("pearson(): two passes, means first", _pair_variant(single_pass=True), _names("pearson/noise/")),
    "pair: float64 input rounded to float32": Variant("_pair / k_pair_sums<double>", _pair_variant(round_f32=True),
                                                      _names("pearson/noise/", "/f64") + _names("cosine/noise/", "/mixed")),
    "pearson: sqrt(sxx) sqrt(syy)": Variant("pearson(): norm = sqrt(sxx syy)", _pair_variant(norm_rule="separate"),
                                            _names("pearson/huge/") + _names("pearson/tiny/")),
    "cosine: sqrt(sxx syy)": Variant("cosine(): norm = sqrt(sxx) sqrt(syy)", _pair_variant(norm_rule="product"), _names("cosine/huge/") + _names("cosine/tiny/")),
    "argmax: the higher index wins a cross-wavefront tie": Variant("k_argmax_rows thread 0's loop: i < bi", _argmax_variant(block_rule="higher"),
                                                                   _names("argmax/r1/", "tie_63_64") + _names("argmax/r1/", "tie_1023_1024")),
    "argmax: the higher lane wins a tie inside a wavefront": Variant("k_argmax_rows shuffle tree: i < bi", _argmax_variant(wave_rule="higher"),
                                                                     _names("argmax/r1/", "tie_10_11") + _names("argmax/r1/", "zeros_")),
    "argmax: the later trip of one thread wins": Variant("k_argmax_rows per-thread loop: v > bv", _argmax_variant(thread_rule="last"),
                                                         _names("argmax/r1/", "tie_5_1029")),
    "argmax: NaN wins": Variant("k_argmax_rows: v != v is skipped", _argmax_variant(nan_wins=True),
                                _names("argmax/r1/", "nan_after_max", where=_small) + _names("argmax/r1/", "nan0_equal", where=_small)),
    "argmax: ld taken as n": Variant("k_argmax_rows row = scores + blockIdx.x * ld", _argmax_variant(stride_as_n=True),
                                     _names("argmax/r5/", where=lambda p: p.args["ld"] and _small(p))),
    "argmax: a row read to ld": Variant("k_argmax_rows loop bound i < n", _argmax_variant(length_as_ld=True),
                                        _names("argmax/r5/", where=lambda p: p.args["ld"] and _small(p))),
    "argmax: all NaN returns -1": Variant("k_argmax_rows bi < 0 ? 0 : bi", _argmax_variant(none_valid=-1), _names("argmax/r1/", "all_nan", where=_small)),
    "argmax: 4 of 16 wavefronts combined": Variant("k_argmax_rows k < blockDim.x / 64", _argmax_variant(waves=4),
                                                   _names("argmax/r1/", "max_1023") + _names("argmax/r1/n1024/", "max_")),
    "threshold: negative maxima ordered as signed": Variant("k_array_max key of a negative value", _threshold_variant(vmax=_max_signed_negative),
                                                            _names("threshold/neg/", "fraction0.5", where=_small) + _names("threshold/negmax", where=_small)),
    "threshold: a maximum of -0.0 unrecorded": Variant("k_array_max: -0.0 is above every negative value and has a key of its own",
                                                       _threshold_variant(vmax=_max_negzero_unrecorded),
                                                       _names("threshold/negzero_max/", "fraction0.5") + _names("threshold/all_negzero/", "fraction0.5")),
    "threshold: NaN dropped by the maximum": Variant("k_array_max: a NaN's key is the largest", _threshold_variant(vmax=_max_nan_dropped),
                                                     _names("threshold/nan", "fraction")),
    "threshold: NaN laundered to 0 by the clip": Variant("k_threshold: v < thresh ? thresh : v", _threshold_variant(launder=True), _names("threshold/nan", "value")),
    "threshold: the fraction applied in float64": Variant("k_threshold: float32 max times float32 fraction", _threshold_variant(fraction_f64=True),
                                                          _names("threshold/pos/", "fraction0.3", where=_small) + _names("threshold/mixed/", "fraction0.3", where=_small)),
    "threshold: the tail n % 256 dropped": Variant("k_array_max / k_threshold grid-stride bound i < n", _threshold_variant(drop_tail=True),
                                                   _names("threshold/max", where=lambda p: p.args["pos"] == p.args["n"] - 1 and 256 < p.args["n"] <= 1025)),
}
