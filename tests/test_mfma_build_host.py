"""The operand and result maps of the pair build on the matrix pipe, modelled in NumPy (tests/mfma_build_cases.py): no GPU.

Every (column, table row, run, component) product occurs exactly once and lands in the accumulator register the transform
reads as x[64 m + lane]; the re-laid factor set is a permutation of the same floats; and the sums, float32 fma in table-row
order from a +0 accumulator, have the bits of the register hand-over's lane map (two column groups per lane, the first row
a plain product) — but for the sign of a zero: fma(e, g, +0) turns a -0 product into +0, which only the groups no row
reaches (zero factors) and zero table entries can show.
"""
import numpy as np
import pytest

from tests import mfma_build_cases as M

ROWS = 160


def test_every_product_once_and_in_the_transforms_place():
    rng = np.random.default_rng(1)
    kgn = 6
    for name, (cg, _) in M.cg_vectors(rng, ROWS, kgn).items():
        seen = set()
        for m in range(M.TILES):
            for lane in range(M.LANES):
                for reg in range(4):
                    col, run, comp = M.result_place(m, lane, reg)
                    assert col == 64 * m + lane and (run, comp) == (reg >> 1, reg & 1)
                    src = (lane & ~3) + reg                  # the lane whose A value register `reg` multiplies
                    for k in range(kgn):
                        entry, part = M.a_operand(m, src, k, cg)
                        assert entry == cg[col >> 2] + k and part == 2 * run + comp, name
                        assert M.b_operand(m, lane, k) == (k, col)
                        key = (col, k, run, comp)
                        assert key not in seen
                        seen.add(key)
        assert len(seen) == M.N * kgn * 4, name


@pytest.mark.parametrize("kg", [1, 7, M.KG_MAX])
def test_the_factor_layout_is_a_permutation_of_the_same_bytes(kg):
    idx = np.array([[M.relaid_index(k, x) for x in range(M.N)] for k in range(kg)])
    assert np.array_equal(np.sort(idx.ravel()), np.arange(kg * M.N))
    assert ((idx // M.N) == np.arange(kg)[:, None]).all()          # a table row stays in its own 2 KB
    # a lane's eight factors of a row are two aligned 16-byte pieces, and a wavefront's reads are contiguous
    lane_idx = idx.reshape(kg, 8, 64)                              # [k][m][lane]
    for half in range(2):
        piece = lane_idx[:, 4 * half:4 * half + 4, :]              # [k][m & 3][lane]
        assert (piece[:, 0, :] % 4 == 0).all() and (np.diff(piece, axis=1) == 1).all()
        assert (np.diff(piece[:, 0, :], axis=1) == 4).all()


@pytest.mark.parametrize("kgn", [1, 2, 6, M.KG_MAX])
@pytest.mark.parametrize("name", ["constant", "one_per_group", "jumps", "unreached"])
def test_the_sums_have_the_lane_maps_bits(name, kgn):
    rng = np.random.default_rng(kgn)
    cg, unreached = M.cg_vectors(rng, ROWS, kgn)[name]
    table = rng.standard_normal((ROWS, 4)).astype(np.float32)
    eg = (rng.random((M.KG_MAX, M.N)) * np.exp(-4 * rng.random((M.KG_MAX, M.N)))).astype(np.float32)
    eg[:, np.repeat(unreached, 4)] = 0.0
    acc = M.build_mfma(table, eg, cg, kgn)
    want = M.build_lanes(table, eg, cg, kgn)
    got = acc.transpose(0, 2, 1).reshape(M.N, 4)                   # (tile, lane) -> column 64 m + lane
    assert np.array_equal(got.view(np.uint32), (want + np.float32(0)).view(np.uint32))
    if not unreached.any():
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    else:
        assert (got[np.repeat(unreached, 4)] == 0).all()
