"""A NumPy model of the pair build on the matrix pipe (k_fused_pass<512, ., ., twists>::build_pair), shared by
tests/test_mfma_build_host.py and tests/test_gpu_mfma_build.py.

`v_mfma_f32_4x4x1_16b_f32` is sixteen 4 x 4 outer products, one per block b of four lanes: D_b[i][j] += A[4 b + i] B[4 b + j]
with D_b[i][j] in register i of lane 4 b + j.  Tile m of the build covers the columns 64 m + lane, so block b of tile m is
column group xg = 16 m + b (four consecutive columns that share their first table row cg[xg]).  The A operand of table
row k is float i = lane & 3 of the 16-byte pair-table entry cg[xg] + k = {G_A.re, G_A.im, G_B.re, G_B.im}; the B operand
is the column factor eg[k][64 m + lane], which a lane reads from a factor set re-laid as [k][half][lane][4] with the
last index m - 4 half.  Register i of tile m in lane L is then component i of column 64 m + L: the transform's
first-stage input x[64 m + lane] of run A (i = 0, 1) and of run B (i = 2, 3).
"""
import numpy as np

N = 512
LANES, TILES, GROUPS = 64, 8, N // 4
KG_MAX = 16


def fma32(a, b, c):
    """float32 fma, elementwise: the product of two float32 is exact in float64."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def a_operand(m, lane, k, cg):
    """(table entry, float of the entry) that `lane` supplies as A of tile m at table row k."""
    return int(cg[16 * m + (lane >> 2)]) + k, lane & 3


def b_operand(m, lane, k):
    """(table row, column) of the factor that `lane` supplies as B of tile m."""
    return k, 64 * m + lane


def relaid_index(k, x):
    """Float index in the LDS factor set of eg[k][x]: [k][half][lane][m & 3], x = 64 m + lane, half = m >> 2."""
    m, lane = x >> 6, x & 63
    return k * N + (m >> 2) * 256 + lane * 4 + (m & 3)


def result_place(m, lane, reg):
    """(column, run, component) held by register `reg` of tile m in `lane`."""
    return 64 * m + lane, reg >> 1, reg & 1


def mfma_4x4x1(a, b, c):
    """a, b: [64] per-lane operands; c: [4][64] accumulator (register, lane).  Returns d = c + outer products per block."""
    lanes = np.arange(LANES)
    d = np.empty_like(c)
    for i in range(4):
        d[i] = fma32(a[(lanes & ~3) + i], b, c[i])
    return d


def build_mfma(table, eg, cg, kgn):
    """table: [rows][4] float32 pair entries; eg: [kg][N]; cg: [N/4].  Returns acc[8][4][64] (tile, register, lane)."""
    lds = np.empty(eg.size, np.float32)
    kk, xx = np.meshgrid(np.arange(eg.shape[0]), np.arange(N), indexing="ij")
    lds[np.vectorize(relaid_index)(kk, xx)] = eg
    lanes = np.arange(LANES)
    acc = np.zeros((TILES, 4, LANES), np.float32)          # the first row's C is +0
    for k in range(kgn):
        for m in range(TILES):
            a = np.array([table[a_operand(m, int(l), k, cg)] for l in lanes], np.float32)
            # the lane's two 16-byte reads of row k: pieces (k, half, lane), float m & 3
            b = lds[k * N + (m >> 2) * 256 + lanes * 4 + (m & 3)]
            acc[m] = mfma_4x4x1(a, b, acc[m])
    return acc


def build_lanes(table, eg, cg, kgn):
    """The register hand-over's build: lane t owns column groups t and t + 64; the first row is a plain product.  Returns
    sums[N][4] (column, {A.re, A.im, B.re, B.im})."""
    out = np.empty((N, 4), np.float32)
    for xg in range(GROUPS):
        cols = 4 * xg + np.arange(4)
        g = table[cg[xg]]
        s = (eg[0, cols][:, None] * g[None, :]).astype(np.float32)
        for k in range(1, kgn):
            g = table[cg[xg] + k]
            s = fma32(np.broadcast_to(eg[k, cols][:, None], (4, 4)), np.broadcast_to(g[None, :], (4, 4)), s)
        out[cols] = s
    return out


def cg_vectors(rng, rows, kgn):
    """First table rows per column group: constant, one entry further per group, with jumps, and with groups no row reaches
    (returned with the mask of those groups, whose factors the factor kernel leaves zero)."""
    top = rows - kgn
    assert top >= GROUPS - 1
    none = np.zeros(GROUPS, bool)
    jumps = np.sort(rng.integers(0, top + 1, GROUPS))
    unreached = rng.random(GROUPS) < 0.3
    unreached[[0, 17, GROUPS - 1]] = True
    return {
        "constant": (np.full(GROUPS, min(3, top)), none),
        "one_per_group": (np.arange(GROUPS), none),
        "jumps": (jumps, none),
        "unreached": (np.where(unreached, 0, jumps), unreached),
    }
