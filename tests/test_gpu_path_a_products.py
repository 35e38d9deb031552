"""Every implementation of the Path A products y = A x and g = A^T y against the float64 oracle matrix [A_data; A_hsym]
(oracle/path_a.py, built outside the library and pinned to the reference at these corners by fixture G22): the
single-candidate hh_pa (nearest neighbour and trilinear) and the batch's sliced, general, LDS, separable ("factored") and
banded forms, over the case table of tests/path_a_product_cases.py — scales 0.8 / 0.5 / 1.25, quarter turns (coordinates on
integers, where the ~1e-16 noise of Ry(90) decides a truncation), odd sides, a hole, dy up to rows without a ray, one to
three groups of home layers, the 64-bit word edge of the footprint masks, the separable form's last size and the first size
of the direct LDS form, rises longer and much shorter than the box, half sets, tilt / psi.

Per case: the dimensions, the operations used, b and the pixel ids are the oracle's exactly (half sets: its rows selected by
split_A_b's rule); hh_pa and the batch form the case NAMES (asserted) apply four seeded probes each way — two Gaussian, all
ones, small integers — and are compared with the oracle's products directly, never with each other; with nearest
neighbour the entries are hit counts and the integer probe's A x is the oracle's exactly; <A x, y> = <x, A^T y> to 1e-12.

The symmetry block: its trilinear weights are float32 numbers in the reference, and the device stores those (bit for bit,
tests/test_gpu_path_a.py); the oracle's block is that one widened to float64.  The data block is the oracle's summed float64
weights.

BOUND: normalised error max |got - ref| / max(1, max |ref|).  The project's figure for product parity, 1e-12, had been
measured between two device implementations only; measured here against the oracle over the whole table on the MI355X
(profiles/path_a_products.json) — see BOUND below."""
import os

import numpy as np
import pytest

from helicon_amd._lib import hh_pa_params
from helicon_amd.solver import PAB_ALLOW_BANDED, PAB_FORCE_BANDED, PathABatch, PathAProblem
from tests import path_a_product_cases as C

pytestmark = pytest.mark.gpu

# Largest normalised error per implementation over the table, MI355X (profiles/path_a_products.json): hh_pa nearest neighbour
# 7.7e-16, hh_pa trilinear 7.6e-15, sliced 4.8e-16, general 7.7e-16, LDS 3.9e-15, separable 9.2e-15, banded 1.1e-14 — every one
# within the project's 1e-12, which therefore stays (the rule: keep 1e-12 if the measurement is within it, else the
# measurement x 4 rounded up to one digit, never above 1e-10).
BOUND = {"hh_pa_nn": 1e-12, "hh_pa_linear": 1e-12, "sliced": 1e-12, "general": 1e-12, "lds": 1e-12, "factored": 1e-12,
         "banded": 1e-12}


def _params(c):
    d2, l2, d3, d3i, l3 = c.box
    tw, rs, cs = c.cand
    return hh_pa_params(c.scale, tw, rs, cs, c.tilt, c.psi, c.dy, d2, l2, d3, d3i, l3, c.min_lines, c.min_sym,
                        1 if c.interp == "linear" else 0, c.fsc_mode, c.fsc_half)


@pytest.fixture(scope="module")
def batch_of():
    """case -> (its batch, its index): the cases of one batch_key share a PathABatch, built on first use."""
    built = {}

    def get(c):
        key = C.batch_key(c)
        if key not in built:
            members = [m for m in C.CASES if C.batch_key(m) == key]
            before = os.environ.pop("HH_PAB_GENERAL", None)
            if c.force_general:
                os.environ["HH_PAB_GENERAL"] = "1"
            try:
                flags = 0 if c.form != "banded" else PAB_FORCE_BANDED if C.banded_by(c) == "force" else PAB_ALLOW_BANDED
                B = PathABatch(C.image(c), [_params(m) for m in members], flags=flags)
            finally:
                os.environ.pop("HH_PAB_GENERAL", None)
                if before is not None:
                    os.environ["HH_PAB_GENERAL"] = before
            built[key] = (B, members)
        B, members = built[key]
        return B, members.index(c)

    yield get
    for B, _ in built.values():
        B.close()


def _err(got, ref):
    return float(np.abs(got - ref).max() / max(1.0, np.abs(ref).max())) if len(ref) else 0.0


def _check_products(name, cid, matvec, rmatvec, S, nn, seed):
    """Four probes each way through one implementation against the oracle matrix; returns the largest normalised error."""
    M, MT = S["A"], S["A"].T.tocsr()
    xs, ys = C.probes(M.shape[1], seed), C.probes(M.shape[0], seed + 1)
    ax = [matvec(x) for x in xs]
    aty = [rmatvec(y) for y in ys]
    worst = max(max(_err(g, M @ x) for g, x in zip(ax, xs)), max(_err(g, MT @ y) for g, y in zip(aty, ys)))
    print(f"path_a_products figure {name} {worst:.3e} {cid}")
    assert worst <= BOUND[name], (name, cid, worst)
    if nn:   # hit counts and +-1 pairs on small integers: every partial sum is an integer
        np.testing.assert_array_equal(ax[3], M @ xs[3], err_msg=f"{name} {cid}")
    for k in (0, 1):
        assert float(np.dot(ax[k], ys[k])) == pytest.approx(float(np.dot(xs[k], aty[k])), rel=1e-12), (name, cid, k)
    return worst


@pytest.mark.parametrize("c", C.CASES, ids=C.case_id)
def test_products_equal_the_oracle_matrix(c, batch_of):
    cid = C.case_id(c)
    S = C.oracle_system(c)
    d2, l2, d3, d3i, l3 = c.box
    tw, rs, cs = c.cand
    nn = c.interp == "nn"
    seed = 7 * C.CASES.index(c)
    with PathAProblem(C.image(c), scale2d_to_3d=c.scale, twist_degree=tw, rise_pixel=rs, csym=cs, tilt_degree=c.tilt, psi_degree=c.psi,
                      dy_pixel=c.dy, reconstruct_diameter_2d_pixel=d2, reconstruct_length_2d_pixel=l2, reconstruct_diameter_3d_pixel=d3,
                      reconstruct_diameter_3d_inner_pixel=d3i, reconstruct_length_3d_pixel=l3, min_projection_lines=c.min_lines,
                      min_sym_pairs=c.min_sym, interpolation=c.interp, fsc_mode=c.fsc_mode, fsc_half=c.fsc_half) as P:
        assert (P.n, P.m_data, P.m_sym, P.n_ops) == (S["n"], S["m_data"], S["m_sym"], S["ops"]), cid
        np.testing.assert_array_equal(P.b_data, S["b"])
        np.testing.assert_array_equal(P.b_pid, S["pid"])
        _check_products("hh_pa_nn" if nn else "hh_pa_linear", cid, P.matvec, P.rmatvec, S, nn, seed)
    B, k = batch_of(c)
    assert B.product_form == c.form, (cid, B.product_form)
    assert (B.n, int(B.m_data[k]), int(B.m_sym[k]), int(B.n_ops[k])) == (S["n"], S["m_data"], S["m_sym"], S["ops"]), cid
    b, pid = B.rhs(k)
    np.testing.assert_array_equal(b, S["b"])
    np.testing.assert_array_equal(pid, S["pid"])
    _check_products(c.form, cid, lambda x: B.matvec(k, x), lambda y: B.rmatvec(k, y), S, nn, seed)
