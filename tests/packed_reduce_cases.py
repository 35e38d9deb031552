"""The packed pair walk's reduction of a pair's six sums through the wavefront's exchange buffer, modelled in numpy
(helicon_hip.hip: part_b_packed; sweep_plan.h: packed_sum_slot, packed_sum_first_half, PACKED_SUM_LANES_A / _B), and the
masks of tests/test_gpu_packed_reduce.py.

Sum s = 0..2 is run A's three moments, s = 3..5 run B's.  Lane `lane` stores its sum s to float 64 s + lane; lane L < 48
(sum L >> 3, part L & 7) reads floats 8 L .. 8 L + 7 as two 16-byte halves, lanes 16-31 and 48-63 the upper half first; the
halves are summed apart, left to right, and added; three DPP adds (quad_perm [1,0,3,2], [2,3,0,1], row_half_mirror) close the
group of eight lanes; lane 8 s stores sum s as one double.
"""
import numpy as np

LANES, SUMS, READERS = 64, 6, 48
BANKS, BANK_BYTES = 64, 4

# The sixteen lanes the LDS serves in one cycle of a 16-byte read (four cycles to the wavefront).
B128_GROUPS = [
    [0, 1, 2, 3, 12, 13, 14, 15, 20, 21, 22, 23, 24, 25, 26, 27],
    [4, 5, 6, 7, 8, 9, 10, 11, 16, 17, 18, 19, 28, 29, 30, 31],
    [32, 33, 34, 35, 44, 45, 46, 47, 52, 53, 54, 55, 56, 57, 58, 59],
    [36, 37, 38, 39, 40, 41, 42, 43, 48, 49, 50, 51, 60, 61, 62, 63],
]

LANES_A, LANES_B = 0x010101, 0x010101 << 24   # the lanes that store run A's and run B's sums


def slot(s, lane):
    return 64 * s + lane


def first_half(lane):
    return (lane >> 4) & 1


def read_floats(lane, which, swapped=True):
    """The four float slots of lane's read number `which` (0: first, 1: second)."""
    half = (first_half(lane) if swapped else 0) ^ which
    return [8 * lane + 4 * half + i for i in range(4)]


def read_banks(lane, which, swapped=True):
    return [(4 * f // BANK_BYTES) % BANKS for f in read_floats(lane, which, swapped)]


def quad_perm(v, perm):
    out = np.empty_like(v)
    for lane in range(LANES):
        out[lane] = v[(lane & ~3) | perm[lane & 3]]
    return out


def row_half_mirror(v):
    out = np.empty_like(v)
    for lane in range(LANES):
        out[lane] = v[(lane & ~7) | (7 - (lane & 7))]
    return out


def reduce6_lanes(x):
    """x [6][64] float32, the lanes' sums -> tot [64] float32 as the wavefront computes it, through a 1024-float buffer
    whose other floats are NaN (a read outside the slot map would show)."""
    x = np.asarray(x, dtype=np.float32)
    buf = np.full(1024, np.nan, dtype=np.float32)
    for s in range(SUMS):
        for lane in range(LANES):
            buf[slot(s, lane)] = x[s, lane]
    tot = np.empty(LANES, dtype=np.float32)
    for lane in range(LANES):
        e0 = buf[read_floats(lane, 0)]
        e1 = buf[read_floats(lane, 1)]
        q0 = np.float32(np.float32(np.float32(e0[0] + e0[1]) + e0[2]) + e0[3])
        q1 = np.float32(np.float32(np.float32(e1[0] + e1[1]) + e1[2]) + e1[3])
        tot[lane] = np.float32(q0 + q1)
    with np.errstate(invalid="ignore"):
        tot = (tot + quad_perm(tot, [1, 0, 3, 2])).astype(np.float32)
        tot = (tot + quad_perm(tot, [2, 3, 0, 1])).astype(np.float32)
        tot = (tot + row_half_mirror(tot)).astype(np.float32)
    return tot


def reduce_stated(row):
    """One sum's 64 lane values in the stated association: eight in a row of slots (two halves of four, left to right),
    eight across as ((p0 + p1) + (p2 + p3)) + ((p7 + p6) + (p5 + p4))."""
    f = np.float32
    row = np.asarray(row, dtype=np.float32)
    p = []
    for c in range(8):
        e = row[8 * c:8 * c + 8]
        p.append(f(f(f(f(e[0] + e[1]) + e[2]) + e[3]) + f(f(f(e[4] + e[5]) + e[6]) + e[7])))
    return f(f(f(p[0] + p[1]) + f(p[2] + p[3])) + f(f(p[7] + p[6]) + f(p[5] + p[4])))


def new_stores(ca, nc, cfirst, run_len, row, npart, wpr=1, wave_in_row=0):
    """{byte address from the partials' first: sum index s} of the six store lanes (32-bit lane offsets, as the kernel)."""
    stores = (LANES_A if ca >= 0 else 0) | (LANES_B if ca + 1 < nc else 0)
    first = (cfirst + ca * run_len) * npart + row * wpr + wave_in_row   # A's triple
    b_bytes = (run_len * npart * 24) & 0xFFFFFFFF
    out = {}
    for lane in range(LANES):
        if (stores >> lane) & 1:
            lane_bytes = lane if lane < 24 else (b_bytes + lane - 24) & 0xFFFFFFFF
            addr = first * 24 + lane_bytes
            assert addr not in out
            out[addr] = lane >> 3
    return out


def old_stores(ca, nc, cfirst, run_len, row, npart, wpr=1, wave_in_row=0):
    """The same of the writer lane's two scalar-branched blocks this replaces."""
    out = {}
    if ca >= 0:
        o = ((cfirst + ca * run_len) * npart + row * wpr + wave_in_row) * 3
        out.update({(o + k) * 8: k for k in range(3)})
    if ca + 1 < nc:
        o = ((cfirst + (ca + 1) * run_len) * npart + row * wpr + wave_in_row) * 3
        out.update({(o + k) * 8: 3 + k for k in range(3)})
    return out


def single_lane_mask(n, t0, band):
    """The band's bins of columns kx = t0 (mod 64) on the rows 0 <= ky <= n/2 (frequencies in FFT order), on the fftshifted
    plane.  A half-plane row's weight is mask(k) + mask(-k); with the other rows empty it is this mask's alone, and all of
    it falls to lane t0 of the row's transform (bins kx = lane + 64 m)."""
    k = (np.arange(n) - n // 2) % n            # shifted index -> FFT-order frequency
    live = ((k % 64) == t0)[None, :] & (k <= n // 2)[:, None]
    return band & live
