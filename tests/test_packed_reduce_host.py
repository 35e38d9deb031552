"""The slot map, bank map, summation order and store lanes of the packed pair walk's six-sum reduction, on the host
(tests/packed_reduce_cases.py is the model; the device side is tests/test_gpu_packed_reduce.py).  No GPU."""
import numpy as np
import pytest

from tests import packed_reduce_cases as P


def test_every_slot_is_written_once_and_read_once_by_its_sums_lane():
    written = [P.slot(s, lane) for s in range(P.SUMS) for lane in range(P.LANES)]
    assert sorted(written) == list(range(P.SUMS * P.LANES))
    read_by = {}
    for lane in range(P.READERS):
        floats = P.read_floats(lane, 0) + P.read_floats(lane, 1)
        assert sorted(floats) == list(range(8 * lane, 8 * lane + 8))
        for f in floats:
            assert f not in read_by
            read_by[f] = lane
    assert sorted(read_by) == sorted(written)
    for s in range(P.SUMS):
        for lane in range(P.LANES):
            reader = read_by[P.slot(s, lane)]
            assert reader >> 3 == s and reader & 7 == lane >> 3
    # the lanes that own no sum read floats the six sums do not use, inside the wavefront's 1024
    for lane in range(P.READERS, P.LANES):
        floats = P.read_floats(lane, 0) + P.read_floats(lane, 1)
        assert min(floats) >= P.SUMS * P.LANES and max(floats) < 1024


def conflicts(swapped):
    extra = 0
    for which in (0, 1):
        for group in P.B128_GROUPS:
            seen = {}
            for lane in group:
                for bank in P.read_banks(lane, which, swapped):
                    seen.setdefault(bank, set()).add(lane)
            extra += sum(len(v) - 1 for v in seen.values())
    return extra


def test_each_16_byte_read_fills_the_banks_once_per_group():
    assert sorted(sum(P.B128_GROUPS, [])) == list(range(P.LANES))
    assert conflicts(swapped=True) == 0
    # every lane on its lower half first — one address for both reads — puts two lanes of a group on each bank it touches
    assert conflicts(swapped=False) == 2 * 4 * 32


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_the_sum_is_the_stated_association(seed):
    rng = np.random.default_rng(seed)
    # mixed magnitudes and signs: another association gives other bits
    x = (rng.standard_normal((P.SUMS, P.LANES)) * np.exp2(rng.integers(-12, 12, (P.SUMS, P.LANES)))).astype(np.float32)
    tot = P.reduce6_lanes(x)
    assert np.isfinite(tot[:P.READERS]).all()
    others = 0
    for s in range(P.SUMS):
        want = P.reduce_stated(x[s])
        for lane in range(8 * s, 8 * s + 8):          # every lane of the group holds the sum; lane 8 s stores it
            assert tot[lane].tobytes() == want.tobytes(), (s, lane)
        assert abs(float(want) - float(x[s].astype(np.float64).sum())) <= 64 * 2.0 ** -24 * float(np.abs(x[s]).sum())
        others += int(np.float32(x[s].sum()).tobytes() != want.tobytes()) + int(np.float32(np.cumsum(x[s])[-1]).tobytes() != want.tobytes())
    assert others > 0   # (the data can tell the orders apart)


def test_single_lane_input_lands_in_its_sum_only():
    for lane in (0, 7, 8, 47, 48, 63):
        x = np.zeros((P.SUMS, P.LANES), dtype=np.float32)
        x[:, lane] = np.arange(1, 7, dtype=np.float32)
        tot = P.reduce6_lanes(x)
        assert [float(tot[8 * s]) for s in range(P.SUMS)] == [1.0, 2.0, 3.0, 4.0, 5.0, 6.0]


@pytest.mark.parametrize("nc", [1, 2, 3, 16, 17])
def test_store_lanes_write_what_the_writer_lane_wrote(nc):
    npart, run_len = 257, 16
    for ca in sorted({-1, 0, nc - 1, nc - 2} | set(range(-1, nc, 2))):
        if ca < -1 or ca >= nc:
            continue
        for cfirst, row in ((0, 1), (5, 255), (131072 - 17 * 16 - 16, 8)):
            new = P.new_stores(ca, nc, cfirst, run_len, row, npart)
            old = P.old_stores(ca, nc, cfirst, run_len, row, npart)
            assert new == old, (ca, nc, cfirst, row)
            assert len(new) == 3 * ((ca >= 0) + (ca + 1 < nc))
    # the largest launch: a run as long as the launch keeps B's distance inside 32 bits
    assert 131072 * npart * 24 < 2 ** 32
    assert P.new_stores(0, 2, 0, 65536, 3, npart) == P.old_stores(0, 2, 0, 65536, 3, npart)


def test_single_lane_masks_weigh_one_lane():
    n = 512
    band = np.ones((n, n), dtype=bool)
    for t0 in (0, 7, 8, 47, 48, 63):
        m = P.single_lane_mask(n, t0, band)
        mu = np.fft.ifftshift(m)                                   # FFT-order frequencies
        w = mu[:n // 2 + 1].astype(int)
        w[1:n // 2] += mu[(-np.arange(1, n // 2)) % n][:, (-np.arange(n)) % n]
        assert w.sum() > 0 and set(np.flatnonzero(w.any(axis=0)) % 64) == {t0}
