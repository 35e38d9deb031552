"""Shared by tests/test_path_a_products_host.py and tests/test_gpu_path_a_products.py (host only: NumPy and the oracle, no
device): the geometries at which the six implementations of the Path A products y = A x and g = A^T y — the
single-candidate hh_pa (nearest neighbour and trilinear) and the batch's sliced, general, LDS, separable ("factored") and
banded forms — are compared with the float64 oracle matrix [A_data; A_hsym] of oracle/path_a.py.

An explicit list, not a Cartesian product.  Every case names the batch form it is meant to exercise; the host test checks
that every value of every axis occurs and that every form has its cases, the device test that the batch reports the form.

Nearest neighbour, "stays sliced": a batch keeps the sliced form only if no ray rounds into two slices.  With tilt = psi = 0 a
ray's axial coordinate Z is one number up to the ~1e-16 noise of Ry(90), so that happens exactly where Z sits on a
half-integer: ``stays_sliced`` asks that no operation the oracle uses and no image column has Z within 1e-9 of one.  Cases
that name "general" are either not sliceable by themselves (a half-integer Z, or tilt / psi) or sliceable and pushed there
by HH_PAB_GENERAL (``force_general``)."""
from collections import namedtuple

import numpy as np
from scipy.sparse import vstack

from oracle import path_a as A

Case = namedtuple("Case", "box cand scale dy tilt psi min_lines min_sym interp fsc_mode fsc_half form force_general")

# (D2d, L2d, D3d, D3d_inner, L3d)
B_4P1 = (16, 20, 14, 0, 6)      # mz - 1 = 5: groups of 4 + 1 home layers
B_ODD = (15, 21, 15, 4, 5)      # odd sides, a hole, exactly one full group
B_ONE = (16, 24, 8, 2, 2)       # one home layer, disc much smaller than the region
B_2G = (17, 20, 17, 0, 9)       # two full groups
B_3G = (17, 20, 17, 0, 10)      # three groups
B_64 = (64, 12, 64, 0, 3)       # the 64-bit word edge of the masks
B_65 = (65, 12, 65, 0, 3)
B_128 = (128, 8, 128, 0, 3)     # the separable form's last D2d — but two planes of this disc (12,449 voxels) pass the LDS:
#                                 a trilinear batch is refused without HH_PAB_ALLOW_BANDED and banded with it (measured)
B_128S = (128, 8, 40, 0, 3)     # its neighbours that do take the separable form at D2d = 128: groups of G = 4 home layers ...
B_128G = (128, 8, 84, 0, 3)     # ... and the largest disc that fits: G = 1 (G shrinks until G + 1 planes fit 120 KB), two groups
B_130 = (130, 8, 40, 0, 3)      # the direct LDS form
BOXES = (B_4P1, B_ODD, B_ONE, B_2G, B_3G, B_64, B_65, B_128, B_128S, B_128G, B_130)
SMALL_BOXES = (B_4P1, B_ODD, B_ONE, B_2G, B_3G)

# (twist, rise, csym)
C_ORD = (27.0, 2.3, 1)
C_Q90 = (90.0, 2.0, 1)
C_Q45 = (45.0, 1.5, 4)
C_Q180 = (180.0, 4.0, 3)
C_NEG = (-41.5, 3.7, 2)
C_C7 = (10.0, 3.0, 7)
C_LONG = (29.0, 25.0, 1)        # a rise longer than the box: hmax = 1, operations with few or no rays
C_MANY = (29.0, 0.6, 1)         # many operations, the row target reached mid-list
CANDIDATES = (C_ORD, C_Q90, C_Q45, C_Q180, C_NEG, C_C7, C_LONG, C_MANY)
QUARTER_TURNS = (C_Q90, C_Q45, C_Q180)

SCALES = (1.0, 0.8, 0.5, 1.25)
DYS = (0.0, 0.5, -0.25, 3.0)
LOW, MID, ALL = 40, 700, 10**6   # min_projection_lines: below one operation's rows / reached mid-list / above all of them
MIN_SYMS = (0, 300)
FORMS = ("sliced", "general", "lds", "factored", "banded")


def _c(box, cand, form, interp, scale=1.0, dy=0.0, lines=ALL, sym=300, tilt=0.0, psi=0.0, fsc=(0, 0), force_general=False):
    return Case(box, cand, scale, dy, tilt, psi, lines, sym, interp, fsc[0], fsc[1], form, force_general)


def _nn():
    s, g = "sliced", "general"
    return [
        # sliced: integer or never-half-integer Z
        _c(B_4P1, C_Q90, s, "nn"),
        _c(B_4P1, C_Q180, s, "nn", dy=0.5, lines=LOW),
        _c(B_4P1, C_ORD, s, "nn", lines=LOW, sym=0),
        _c(B_4P1, C_Q90, s, "nn", scale=0.8, dy=-0.25),
        _c(B_4P1, C_C7, s, "nn", scale=0.8, lines=MID),
        _c(B_ODD, C_Q180, s, "nn"),
        _c(B_ODD, C_C7, s, "nn", dy=3.0, sym=0),
        _c(B_ODD, C_LONG, s, "nn", dy=0.5),
        _c(B_ONE, C_Q90, s, "nn", dy=3.0),
        _c(B_ONE, C_LONG, s, "nn", sym=0),
        _c(B_2G, C_NEG, s, "nn", lines=LOW),
        _c(B_2G, C_Q90, s, "nn", fsc=(2, 1)),
        _c(B_3G, C_MANY, s, "nn", lines=MID),
        _c(B_3G, C_C7, s, "nn", lines=MID),
        _c(B_64, C_Q180, s, "nn", sym=0),
        _c(B_65, C_Q90, s, "nn", scale=0.8, sym=0),
        # general by themselves: a half-integer Z ...
        _c(B_4P1, C_Q45, g, "nn"),
        _c(B_4P1, C_ORD, g, "nn", scale=0.5),
        _c(B_4P1, C_NEG, g, "nn", scale=1.25, dy=-0.25),         # (on B_ODD the half-integers fall on the box's two ends only:
        #                                                            one slice or none, and the batch stays sliced — measured)
        _c(B_3G, C_MANY, g, "nn", scale=0.5, lines=MID),
        _c(B_2G, C_Q45, g, "nn", scale=1.25, lines=MID),
        # ... or tilt / psi
        _c(B_4P1, C_ORD, g, "nn", tilt=3.0, psi=-2.0, dy=0.5),
        _c(B_ODD, C_NEG, g, "nn", tilt=-2.0, psi=1.5),
        # general by HH_PAB_GENERAL on candidates that would stay sliced
        _c(B_ONE, C_Q90, g, "nn", force_general=True),
        _c(B_2G, C_Q180, g, "nn", scale=0.8, dy=0.5, force_general=True),
        _c(B_65, C_Q90, g, "nn", sym=0, force_general=True),
        _c(B_128, C_Q180, g, "nn", sym=0, lines=LOW),            # (a slice of 12076 voxels: past the sliced form's 60 KB)
    ]


def _linear():
    f, b, l = "factored", "banded", "lds"
    small = [
        (B_4P1, C_ORD, dict()),
        (B_4P1, C_Q90, dict(scale=0.8, dy=0.5)),
        (B_4P1, C_MANY, dict(lines=MID)),
        (B_ODD, C_Q180, dict(dy=-0.25)),
        (B_ODD, C_NEG, dict(scale=1.25)),
        (B_ONE, C_Q45, dict(dy=3.0)),
        (B_ONE, C_LONG, dict(scale=0.5, sym=0)),
        (B_2G, C_Q90, dict(fsc=(4, 2), lines=MID)),
        (B_2G, C_C7, dict(lines=LOW, sym=0)),
        (B_3G, C_Q45, dict(scale=0.5, lines=MID)),
        (B_3G, C_MANY, dict(lines=LOW)),
    ]
    out = [_c(box, cand, f, "linear", **kw) for box, cand, kw in small]
    out += [_c(box, cand, b, "linear", **kw) for box, cand, kw in small]     # each small box also under HH_PAB_FORCE_BANDED
    out += [
        _c(B_64, C_Q90, f, "linear", sym=0),
        _c(B_64, C_ORD, f, "linear", scale=0.8, sym=0, lines=LOW),
        _c(B_65, C_Q180, f, "linear", sym=0),
        _c(B_65, C_NEG, f, "linear", dy=0.5, sym=0, lines=LOW),
        _c(B_128, C_Q90, b, "linear", sym=0, lines=LOW),                    # (HH_PAB_ALLOW_BANDED: see B_128)
        _c(B_128, C_ORD, b, "linear", scale=1.25, sym=0, lines=LOW),
        _c(B_128S, C_Q90, f, "linear", sym=0, lines=LOW),
        _c(B_128S, C_ORD, f, "linear", scale=1.25, sym=0),
        _c(B_128G, C_Q180, f, "linear", sym=0, lines=LOW),
        _c(B_128G, C_NEG, f, "linear", scale=0.8, dy=0.5, sym=0),
        _c(B_130, C_ORD, l, "linear"),
        _c(B_130, C_Q90, l, "linear", dy=0.5),
        _c(B_130, C_C7, l, "linear", lines=LOW, sym=0),
        _c(B_130, C_Q45, l, "linear", scale=0.8, sym=0),
        _c(B_130, C_Q180, l, "linear", scale=0.8, dy=-0.25, lines=LOW, sym=0),
    ]
    return out


CASES = tuple(_nn() + _linear())


def case_id(c):
    d2, l2, d3, d3i, l3 = c.box
    tw, rs, cs = c.cand
    parts = [c.interp, c.form + ("!" if c.force_general else ""), f"{d2}x{l2}x{d3}i{d3i}x{l3}", f"t{tw:g}r{rs:g}c{cs}", f"s{c.scale:g}"]
    parts += [f"dy{c.dy:g}"] if c.dy else []
    parts += [f"tilt{c.tilt:g}psi{c.psi:g}"] if c.tilt or c.psi else []
    parts += [f"m{c.min_lines}", f"p{c.min_sym}"]
    parts += [f"fsc{c.fsc_mode}h{c.fsc_half}"] if c.fsc_half else []
    return "-".join(parts)


def batch_key(c):
    """Cases of one key share a batch: one box, scale and interpolation; sliceable and non-sliceable candidates apart."""
    return (c.box, c.scale, c.interp, c.form, c.force_general)


def banded_by(c):
    """How a case that names the banded form gets it: forced on the small boxes (which would take the separable form), allowed
    on a box whose planes do not fit the LDS."""
    return "force" if c.box in SMALL_BOXES else "allow"


def separable_group(c):
    """Home layers per group of the separable form (csrc/path_a_batch.inc: G = 4, less while G + 1 planes pass 120 KB), and
    whether the form fits at all: two planes and the disc's table within 150 KB, D2d <= 128."""
    d2, l2, d3, d3i, l3 = c.box
    n = int(np.count_nonzero(A.get_cylindrical_mask(1, d2, d2, rmin=d3i / 2, rmax=d3 // 2 - 1)))
    G = 4
    while G > 1 and (G + 1) * n * 8 > 120 << 10:
        G -= 1
    return G, d2 <= 128 and 16 * n + 4 * d2 * d2 <= 150 << 10


def image(c):
    """Seeded noise two rows and three columns larger than the 2-D region, so that the region's offset is exercised."""
    d2, l2 = c.box[0], c.box[1]
    return np.random.default_rng(1000 * d2 + l2).standard_normal((d2 + 2, l2 + 3)).astype(np.float32)


def data_args(c):
    """The arguments of build_A_data_matrix after the image (the reference's order)."""
    d2, l2, d3, d3i, l3 = c.box
    tw, rs, cs = c.cand
    return (c.scale, tw, rs, cs, c.tilt, c.psi, c.dy, d2, l2, d3, d3i, l3, c.min_lines, c.interp)


def sym_args(c):
    """The arguments of build_A_helical_sym_matrix as lsq_reconstruct passes them: the (L3d, D3d, D3d) box."""
    d2, l2, d3, d3i, l3 = c.box
    tw, rs, cs = c.cand
    return (l3, d3, d3, tw, rs, cs, d3i / 2, d3 // 2 - 1, c.min_sym, c.interp)


def oracle_data(c, dtype=np.float64):
    """(A_data, b, pixel ids, operations used): the oracle's data block; the number of operations its loop visited is counted
    by handing it the operation list as a generator."""
    used = [0]
    listed = A.hcsym_order

    def counted(*args):
        for op in listed(*args):
            used[0] += 1
            yield op

    A.hcsym_order = counted
    try:
        Ad, b, pid = A.build_A_data_matrix(image(c), *data_args(c), dtype=dtype)
    finally:
        A.hcsym_order = listed
    return Ad.tocsr(), b, pid, used[0]


def half_rows(pid, mode, half):
    """split_A_b's deterministic rules (solver:175-203) as oracle.path_a.lsq_reconstruct restates them: the rows of half 1 / 2."""
    ids = sorted(set(pid.tolist()))
    n = len(ids)
    set1 = ids[::2] if mode == 2 else ids[: n // 3] + ids[n * 2 // 3:] if mode >= 4 else ids[: n // 2]
    is1 = np.isin(pid, set1)
    return is1 if half == 1 else ~is1


def oracle_system(c):
    """The float64 matrix [A_data; A_hsym] of a case with b, the pixel ids, the operations used and the row counts.

    The data block holds the summed float64 weights.  The symmetry block is the reference's own: its trilinear weights are
    float32 numbers (the reference stores them so and the device reproduces them bit for bit, tests/test_gpu_path_a.py), here
    widened to float64; the +-1 pairs of nearest neighbour are exact either way."""
    Ad, b, pid, used = oracle_data(c)
    if c.fsc_half:
        keep = half_rows(pid, c.fsc_mode, c.fsc_half)
        Ad, b, pid = Ad[keep], b[keep], pid[keep]
    As = A.build_A_helical_sym_matrix(*sym_args(c))[0] if c.min_sym else None
    full = vstack((Ad, As.astype(np.float64))).tocsr() if As is not None else Ad
    return dict(A=full, b=b, pid=pid, ops=used, m_data=Ad.shape[0], m_sym=0 if As is None else As.shape[0], n=Ad.shape[1])


def axial_coordinates(c, ops):
    """Z of every sample of the first ``ops`` operations of the oracle's list (tilt = psi = 0: Rz leaves it alone)."""
    d2, l2, d3, d3i, l3 = c.box
    tw, rs, cs = c.cand
    (_, _, Z0), _ = A.back_project_2d_coords_to_3d_coords(image(c), c.scale, d2, l2)
    hs = np.array([h for h, _ in A.hcsym_order(tw, rs, cs, l3, Z0.shape[0])[:ops]], dtype=np.float64)
    return Z0[None] - (hs * rs)[:, None, None, None] + l3 // 2


def stays_sliced(c):
    """No operation the oracle uses and no image column has Z within 1e-9 of a half-integer (and there is no tilt / psi)."""
    if c.tilt or c.psi:
        return False
    Z = axial_coordinates(c, oracle_data(c)[3])
    return bool((np.abs(Z - np.floor(Z) - 0.5) > 1e-9).all())


def probes(n, seed):
    """Four seeded probes of length n: two Gaussian, all ones, small integers in [-8, 8]."""
    rng = np.random.default_rng(seed)
    return [rng.standard_normal(n), rng.standard_normal(n), np.ones(n), rng.integers(-8, 9, n).astype(np.float64)]


def slice_fits(c):
    """A slice of the cylinder as float64 fits the sliced form's 60 KB of LDS (include/helicon_hip.h)."""
    d2, l2, d3, d3i, l3 = c.box
    n = int(np.count_nonzero(A.get_cylindrical_mask(1, d2, d2, rmin=d3i / 2, rmax=d3 // 2 - 1)))
    return 8 * n <= 60 << 10


def expected_nn_form(c):
    """What a nearest-neighbour batch of candidates like c takes, from the CPU alone."""
    return "sliced" if stays_sliced(c) and slice_fits(c) and not c.force_general else "general"


# The cases pinned to the reference itself by tests/golden/g22_path_a_grid.npz: sides <= 24, every small box, every candidate,
# scale, dy and row target, with and without symmetry rows, both half-set rules' cases, tilt / psi, both interpolations
G22 = (
    _c(B_4P1, C_Q180, "sliced", "nn", dy=0.5, lines=LOW),
    _c(B_4P1, C_C7, "sliced", "nn", scale=0.8, lines=MID),
    _c(B_ODD, C_LONG, "sliced", "nn", dy=0.5),
    _c(B_4P1, C_NEG, "general", "nn", scale=1.25, dy=-0.25),
    _c(B_ONE, C_Q90, "sliced", "nn", dy=3.0),
    _c(B_2G, C_Q90, "sliced", "nn", fsc=(2, 1)),
    _c(B_4P1, C_ORD, "general", "nn", tilt=3.0, psi=-2.0, dy=0.5),
    _c(B_4P1, C_ORD, "factored", "linear"),
    _c(B_4P1, C_MANY, "factored", "linear", lines=MID),
    _c(B_ODD, C_Q180, "factored", "linear", dy=-0.25),
    _c(B_ONE, C_LONG, "factored", "linear", scale=0.5, sym=0),
    _c(B_2G, C_Q90, "factored", "linear", fsc=(4, 2), lines=MID),
    _c(B_3G, C_Q45, "factored", "linear", scale=0.5, lines=MID),
)
