#!/usr/bin/env python3
"""Generate tests/golden/g22_path_a_grid.npz — the Path A matrices at the corners of tests/path_a_product_cases.py — by
importing the REFERENCE itself.

Run in the build container only (the reference never travels to the GPU box), from the repository's root:

    PYTHONDONTWRITEBYTECODE=1 PYTHONPATH=<helicon checkout>/src:. python3 tests/golden/make_golden_path_a_grid.py

For every case of ``path_a_product_cases.G22`` (sides <= 24: every small box, candidate, scale, dy and row target of the
table, tilt / psi, both interpolations) the reference's ``build_A_data_matrix`` and ``build_A_helical_sym_matrix``
(solver_linear_regression.py:1304-1654, 847-1298) run on the case's image.  Stored per case: the arguments and the image;
b, the pixel ids, the matrix's shape and number of stored entries; and, for seeded probes x and y (float64, multiples of
1 / 4 so that they compress), the products A x and A^T y of the matrix widened to float64 — products, not CSR triplets,
which keeps the file small.  The same for the symmetry matrix where the case asks for symmetry rows (shape (0, n) where the
reference finds none).  Every array is an INPUT or an OUTPUT of a reference function; no reference source text is stored.
"""
import os
from pathlib import Path

import numpy as np

import helicon  # the reference

from tests import path_a_product_cases as C

OUT = Path(__file__).resolve().parent


def probe(n, seed):
    return np.round(np.random.default_rng(seed).standard_normal(n) * 4) / 4


def products(M, tag, k, out):
    M = M.tocsr().astype(np.float64)
    x, y = probe(M.shape[1], 100 + k), probe(M.shape[0], 200 + k)
    out[f"case{k}_{tag}_shape"] = np.asarray(M.shape, dtype=np.int64)
    out[f"case{k}_{tag}_nnz"] = np.asarray([M.nnz], dtype=np.int64)
    out[f"case{k}_{tag}_x"], out[f"case{k}_{tag}_y"] = x, y
    out[f"case{k}_{tag}_Ax"], out[f"case{k}_{tag}_ATy"] = M @ x, M.T @ y


def main():
    from helicon.webApps.denovo3D.solver_linear_regression import build_A_data_matrix, build_A_helical_sym_matrix

    out = {"n_cases": np.asarray([len(C.G22)], dtype=np.int64)}
    for k, c in enumerate(C.G22):
        img = C.image(c)
        args = C.data_args(c)
        out[f"case{k}_image"] = img
        out[f"case{k}_args"] = np.asarray(args[:-1], dtype=np.float64)
        out[f"case{k}_linear"] = np.asarray([c.interp == "linear"])
        Ad, b, pid = build_A_data_matrix(img.copy(), *args)
        out[f"case{k}_b"], out[f"case{k}_pid"] = np.asarray(b), np.asarray(pid)
        products(Ad, "data", k, out)
        line = f"g22 {k} {C.case_id(c)} data {Ad.shape} nnz {Ad.nnz}"
        if c.min_sym:
            sargs = C.sym_args(c)
            out[f"case{k}_sym_args"] = np.asarray(sargs[:-1], dtype=np.float64)
            As, _ = build_A_helical_sym_matrix(*sargs)
            if As is None:
                out[f"case{k}_sym_shape"] = np.asarray([0, Ad.shape[1]], dtype=np.int64)
            else:
                products(As, "sym", k, out)
            line += f" sym {None if As is None else As.shape}"
        print(line, flush=True)
    np.savez_compressed(OUT / "g22_path_a_grid.npz", **out)
    print((OUT / "g22_path_a_grid.npz").stat().st_size)


if __name__ == "__main__":
    assert "reference" in os.path.abspath(helicon.__file__), helicon.__file__
    main()
