"""The Path-A oracle (oracle/path_a.py) against outputs of the reference itself (fixtures G4, G5 of
tests/golden/make_golden.py): index structures bit for bit, least-squares scores to the solver's own tolerance."""
import numpy as np
import pytest
from scipy.sparse import csr_matrix

from oracle import path_a as A


def _csr(g, tag):
    return csr_matrix((g[f"{tag}_data"], g[f"{tag}_indices"], g[f"{tag}_indptr"]), shape=tuple(g[f"{tag}_shape"]))


def test_g4_masks_halton_pairs_and_back_projection(golden_dir):
    g = np.load(golden_dir / "g4_path_a.npz")
    for k in range(4):
        nz, ny, nx, rmin, rmax = g[f"mask{k}_args"]
        m = A.get_cylindrical_mask(int(nz), int(ny), int(nx), rmin=rmin, rmax=rmax)
        assert np.count_nonzero(m) == int(g[f"mask{k}_count"][0])
        np.testing.assert_array_equal(np.argwhere(m)[:5], g[f"mask{k}_first_nonzero"])
    assert not A.get_cylindrical_mask(3, 3, 3)[0, 1, 1] and A.get_cylindrical_mask(5, 5, 5)[2, 2, 2]  # test_analysis.py:40-45
    for n in (7, 9, 16, 73):
        np.testing.assert_array_equal(A.halton_order(n), g[f"halton_{n}"])
    assert len(set(A.halton_order(73).tolist())) == 65                       # repeats and omissions are kept
    for k in range(3):
        tw, rs, cs, nz = g[f"pairs{k}_args"]
        got = A.sorted_hsym_csym_pairs(tw, rs, int(cs), int(nz))
        flat = np.asarray([[p[0], p[1], p[2], p[3], p[4], *p[5][0], *p[5][1]] for p in got], dtype=np.float64)
        np.testing.assert_array_equal(flat, g[f"pairs{k}"])
    (X, Y, Z), vals = A.back_project_2d_coords_to_3d_coords(g["bp_image"], 1.0, 4, 4)
    for got, want in ((X, g["bp_X"]), (Y, g["bp_Y"]), (Z, g["bp_Z"]), (vals, g["bp_vals"])):
        np.testing.assert_array_equal(got, want)
    (X, Y, Z), vals = A.back_project_2d_coords_to_3d_coords(np.arange(48, dtype=np.float32).reshape(6, 8), 1.5, 4, 6)
    for got, want in ((X, g["bp2_X"]), (Y, g["bp2_Y"]), (Z, g["bp2_Z"]), (vals, g["bp2_vals"])):
        np.testing.assert_array_equal(got, want)


def test_g4_data_and_symmetry_matrices_are_bit_exact(golden_dir):
    g = np.load(golden_dir / "g4_path_a.npz")
    for k in range(2):
        a = g[f"adata{k}_args"]
        Am, b, pid = A.build_A_data_matrix(g[f"adata{k}_image"], a[0], a[1], a[2], int(a[3]), a[4], a[5], a[6], int(a[7]),
                                           int(a[8]), int(a[9]), int(a[10]), int(a[11]), int(a[12]))
        Am.sum_duplicates()
        Am.sort_indices()
        ref = _csr(g, f"adata{k}")
        assert Am.shape == ref.shape
        np.testing.assert_array_equal(Am.indptr, ref.indptr)
        np.testing.assert_array_equal(Am.indices, ref.indices)
        np.testing.assert_array_equal(Am.data, ref.data)
        np.testing.assert_array_equal(b, g[f"adata{k}_b"])
        np.testing.assert_array_equal(pid, g[f"adata{k}_pid"])
    for k in range(2):
        a = g[f"ahsym{k}_args"]
        Am, b = A.build_A_helical_sym_matrix(int(a[0]), int(a[1]), int(a[2]), a[3], a[4], int(a[5]), a[6], a[7], int(a[8]))
        Am.sort_indices()
        ref = _csr(g, f"ahsym{k}")
        assert Am.shape == ref.shape and len(b) == ref.shape[0] and not b.any()
        np.testing.assert_array_equal(Am.indptr, ref.indptr)
        np.testing.assert_array_equal(Am.indices, ref.indices)
        np.testing.assert_array_equal(Am.data, ref.data)


def test_lsmr_restatement_against_scipy():
    from scipy.sparse import random as sprandom
    from scipy.sparse.linalg import lsmr as sp_lsmr

    rng = np.random.default_rng(0)
    M = sprandom(300, 120, density=0.05, random_state=1, format="csr")
    b = rng.normal(size=300)
    x, istop, itn, normr, normar = A.lsmr(M, b, atol=1e-8, btol=1e-8, maxiter=500)
    ref = sp_lsmr(M, b, atol=1e-8, btol=1e-8, maxiter=500)
    assert (istop, itn) == (ref[1], ref[2])
    np.testing.assert_allclose(x, ref[0], rtol=0, atol=1e-6)     # near convergence the iterates carry rounding noise
    assert normr == pytest.approx(ref[3], rel=1e-10)
    for it in (1, 3, 10):                                         # the recurrences themselves, before the noise grows
        xa = A.lsmr(M, b, atol=0, btol=0, conlim=0, maxiter=it)[0]
        xb = sp_lsmr(M, b, atol=0, btol=0, conlim=0, maxiter=it)[0]
        np.testing.assert_allclose(xa, xb, rtol=0, atol=1e-12)


def test_g5_lsq_reconstruct_scores_and_volumes(golden_dir):
    """The reference runs scipy's LSMR on float32 operands (tolerance 1e-4); the oracle iterates in float64: scores
    agree to 1e-4, the volume to the solver's tolerance."""
    g = np.load(golden_dir / "g5_lsq.npz")
    s2, tw, rs, cs, d2, d3, l2, l3, ov = g["seed42_args"]
    (rec, h1, h2), score = A.lsq_reconstruct(g["seed42_image"], s2, tw, rs, int(cs), reconstruct_diameter_2d_pixel=int(d2),
                                             reconstruct_diameter_3d_pixel=int(d3), reconstruct_length_2d_pixel=int(l2),
                                             reconstruct_length_3d_pixel=int(l3), sym_oversample=ov)
    assert h1 is None and h2 is None and rec.shape == (8, 8, 8) and rec.dtype == np.float32
    assert score == pytest.approx(float(g["seed42_score"][0]), abs=1e-4)
    assert np.abs(rec - g["seed42_rec3d"]).max() < 5e-3 * np.abs(g["seed42_rec3d"]).max()
    s2, rs, cs, d2, d3, l2, l3, ov = g["helix_args"]
    for tw, want in zip(g["helix_twists"], g["helix_scores"]):
        (rec, _, _), score = A.lsq_reconstruct(g["helix_image"], s2, float(tw), rs, int(cs), reconstruct_diameter_2d_pixel=int(d2),
                                               reconstruct_diameter_3d_pixel=int(d3), reconstruct_length_2d_pixel=int(l2),
                                               reconstruct_length_3d_pixel=int(l3), sym_oversample=ov)
        assert score == pytest.approx(float(want), abs=1e-4), tw
        if tw == 29.0:
            assert np.abs(rec - g["helix_rec3d_29"]).max() < 5e-3 * np.abs(g["helix_rec3d_29"]).max()


def test_g4b_linear_matrices_and_scores(golden_dir):
    """Trilinear branch: the data matrix (solver:1414-1503) and the symmetry matrix (:910-1140, weight typos and the
    |d| >= 3 rule included) have the reference's structure exactly and its float32 entries to an ulp; lsq_reconstruct
    with interpolation="linear" reproduces the reference's scores."""
    g = np.load(golden_dir / "g4b_path_a_linear.npz")
    for k in range(3):
        a = g[f"adata{k}_args"]
        Am, b, pid = A.build_A_data_matrix(g[f"adata{k}_image"], a[0], a[1], a[2], int(a[3]), a[4], a[5], a[6], int(a[7]),
                                           int(a[8]), int(a[9]), int(a[10]), int(a[11]), int(a[12]), "linear")
        Am.sum_duplicates()
        Am.sort_indices()
        ref = _csr(g, f"adata{k}")
        assert Am.shape == ref.shape
        np.testing.assert_array_equal(Am.indptr, ref.indptr)
        np.testing.assert_array_equal(Am.indices, ref.indices)
        np.testing.assert_allclose(Am.data, ref.data, rtol=2e-7, atol=1e-9)   # float64 sums rounded to float32 once
        np.testing.assert_array_equal(b, g[f"adata{k}_b"])
        np.testing.assert_array_equal(pid, g[f"adata{k}_pid"])
    for k in range(2):
        a = g[f"ahsym{k}_args"]
        Am, b = A.build_A_helical_sym_matrix(int(a[0]), int(a[1]), int(a[2]), a[3], a[4], int(a[5]), a[6], a[7], int(a[8]), "linear")
        Am.sort_indices()
        ref = _csr(g, f"ahsym{k}")
        assert Am.shape == ref.shape
        np.testing.assert_array_equal(Am.indptr, ref.indptr)
        np.testing.assert_array_equal(Am.indices, ref.indices)
        np.testing.assert_array_equal(Am.data, ref.data)
    (rec, _, _), score = A.lsq_reconstruct(g["seed42_image"], 1.0, 30.0, 2.0, 1, reconstruct_diameter_2d_pixel=8,
                                           reconstruct_diameter_3d_pixel=8, reconstruct_length_2d_pixel=8,
                                           reconstruct_length_3d_pixel=8, sym_oversample=1, interpolation="linear")
    # The matrices above are the reference's; what differs is the arithmetic of the solve: the reference runs scipy's
    # LSMR on float32 operands (float32 vectors and, under NumPy 2's promotion rules, float32 scalar recurrences) and
    # stops the bounded iteration at tol = 1e-2, the oracle iterates in float64.  With trilinear weights that moves the
    # cosine score by up to 1e-3 (with 0/1 hit counts, fixture G5, by less than 1e-4).
    LIN_TOL = 2e-3
    assert score == pytest.approx(float(g["seed42_score"][0]), abs=LIN_TOL)
    got = []
    for tw, want in zip(g["helix_twists"], g["helix_scores"]):
        (rec, _, _), score = A.lsq_reconstruct(g["helix_image"], 1.0, float(tw), 2.0, 1, reconstruct_diameter_2d_pixel=20,
                                               reconstruct_diameter_3d_pixel=20, reconstruct_length_2d_pixel=32,
                                               reconstruct_length_3d_pixel=6, sym_oversample=1, interpolation="linear")
        assert score == pytest.approx(float(want), abs=LIN_TOL), tw
        got.append(score)
        if tw == 29.0:
            assert A.cosine_similarity(rec.ravel(), g["helix_rec3d_29"].ravel()) > 0.995   # same map, loosely converged
    assert int(np.argmax(got)) == int(np.argmax(g["helix_scores"])) == 1


def test_g9_task_function_scores(golden_dir):
    """Fixture G9 (the reference's process_one_task on a 32 x 48 helix): the oracle's lsq_reconstruct on the box sizes
    the reference derived reproduces its cosine scores and maps (nearest neighbour; the low-passed, thresholded
    case 3 is covered on the device, where the whole preparation runs)."""
    g = np.load(golden_dir / "g9_process_one_task.npz")
    for k in (0, 1):
        tw, rs, cs, interp, thr, a3, td, lp = g[f"case{k}_args"]
        d2, d3, l2, l3 = (int(v) for v in g[f"case{k}_dims"])
        (rec, _, _), score = A.lsq_reconstruct(g["image"], 1.0, tw, rs / a3, int(cs), reconstruct_diameter_2d_pixel=d2,
                                               reconstruct_diameter_3d_pixel=d3, reconstruct_length_2d_pixel=l2,
                                               reconstruct_length_3d_pixel=l3, sym_oversample=1, interpolation="nn")
        assert score == pytest.approx(float(g[f"case{k}_score"][0]), abs=1e-4)
        assert np.abs(rec - g[f"case{k}_rec3d"]).max() < 1e-2 * np.abs(g[f"case{k}_rec3d"]).max()


def test_g11_half_set_solves(golden_dir):
    """lsq_reconstruct(fsc_test = 2, 3, 4): the reference's combined score and its three maps (whole image, two pixel
    halves) from the oracle's restatement of split_A_b."""
    g = np.load(golden_dir / "g11_fsc_halves.npz")
    for mode in (2, 3, 4):
        (rec, r1, r2), score = A.lsq_reconstruct(g["image"], 1.0, 29.0, 2.0, 1, reconstruct_diameter_2d_pixel=20,
                                                 reconstruct_diameter_3d_pixel=20, reconstruct_length_2d_pixel=48,
                                                 reconstruct_length_3d_pixel=6, sym_oversample=1, interpolation="nn", fsc_test=mode)
        assert score == pytest.approx(float(g[f"mode{mode}_score"][0]), abs=1e-4)
        for got, name in ((rec, "rec"), (r1, "rec1"), (r2, "rec2")):
            want = g[f"mode{mode}_{name}"]
            assert np.abs(got - want).max() < 1e-2 * np.abs(want).max(), (mode, name)


def test_g22_grid_of_corners(golden_dir):
    """Fixture G22 (tests/golden/make_golden_path_a_grid.py): the reference's own build_A_data_matrix and
    build_A_helical_sym_matrix at the corners of tests/path_a_product_cases.py — scales 0.8 / 0.5 / 1.25, quarter turns, odd
    sides, a hole, dy, tilt / psi, rises longer and much shorter than the box, both interpolations.  The default (float32)
    oracle reproduces the reference's products to 1e-12 max(1, max |ref|); b, pixel ids and shapes exactly (the number of
    stored entries is not compared: at scale 1.25 / twist 90 the two differ in ~1e-16 entries that one side stores and the
    other has as exact zeros); and the float64 oracle rounds to the float32 one entry for entry."""
    from tests import path_a_product_cases as C

    g = np.load(golden_dir / "g22_path_a_grid.npz")
    assert int(g["n_cases"][0]) == len(C.G22)

    def check_products(M, tag, k):
        assert M.shape == tuple(g[f"case{k}_{tag}_shape"])
        M64 = M.tocsr().astype(np.float64)
        for got, want in ((M64 @ g[f"case{k}_{tag}_x"], g[f"case{k}_{tag}_Ax"]), (M64.T @ g[f"case{k}_{tag}_y"], g[f"case{k}_{tag}_ATy"])):
            assert np.abs(got - want).max() <= 1e-12 * max(1.0, np.abs(want).max()), (k, tag)

    def check_rounding(M64, M32, k):
        assert M64.dtype == np.float64 and M32.dtype == np.float32
        # (entry for entry through the dense arrays: whether a ~1e-16 entry is stored does not matter)
        np.testing.assert_array_equal(M64.toarray().astype(np.float32), M32.toarray(), err_msg=str(k))

    for k, c in enumerate(C.G22):
        img, interp = g[f"case{k}_image"], "linear" if g[f"case{k}_linear"][0] else "nn"
        a = g[f"case{k}_args"]
        args = (a[0], a[1], a[2], int(a[3]), a[4], a[5], a[6], *(int(v) for v in a[7:13]), interp)
        assert args == C.data_args(c) and np.array_equal(img, C.image(c))      # the table's case is the fixture's
        Ad, b, pid = A.build_A_data_matrix(img, *args)
        np.testing.assert_array_equal(b, g[f"case{k}_b"])
        np.testing.assert_array_equal(pid, g[f"case{k}_pid"])
        assert b.dtype == g[f"case{k}_b"].dtype and Ad.dtype == np.float32
        check_products(Ad, "data", k)
        Ad64, b64, pid64 = A.build_A_data_matrix(img, *args, dtype=np.float64)
        np.testing.assert_array_equal(b64, b)
        np.testing.assert_array_equal(pid64, pid)
        check_rounding(Ad64, Ad, k)
        if not c.min_sym:
            continue
        s = g[f"case{k}_sym_args"]
        sargs = (int(s[0]), int(s[1]), int(s[2]), s[3], s[4], int(s[5]), s[6], s[7], int(s[8]), interp)
        assert sargs == C.sym_args(c)
        As, _ = A.build_A_helical_sym_matrix(*sargs)
        As64, _ = A.build_A_helical_sym_matrix(*sargs, dtype=np.float64)
        if int(g[f"case{k}_sym_shape"][0]) == 0:
            assert As is None and As64 is None
            continue
        check_products(As, "sym", k)
        check_rounding(As64, As, k)
