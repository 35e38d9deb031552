"""Host side of the fused sweep's shared column factors and trimmed run tables (no GPU: both entry points are pure
host arithmetic, like hh_fused_schedule).

* hh_rise_columns_shared: the decision plan_runs takes — one set of column factors per rise when every run of the list
  carries run 0's rise column, value for value and in order.
* hh_table_extent: the subunit index range a run's table covers.  It must contain every (i, u) row that the device's
  float32 window test lets into any image column, and never exceed the lattice's own ceil(height / rise).
"""
import ctypes as C

import numpy as np
import pytest

from helicon_amd import _lib
from helicon_amd.grid import build_grid

F32 = np.float32


def shared(params, run_len):
    p = np.ascontiguousarray(params, dtype=np.float64).reshape(-1, 4)
    rc = _lib.lib().hh_rise_columns_shared(p.ctypes.data_as(C.POINTER(C.c_double)), len(p), run_len)
    assert rc in (0, 1), rc
    return rc


def test_sharing_decision():
    twists, rises = np.arange(20.0, 26.0), 4.0 + 0.25 * np.arange(16)
    grid = build_grid(twists, rises, (1,), tube_length=1000.0).params          # twist-major: 6 runs of 16
    assert shared(grid, 16) == 1
    moved = grid.copy()
    moved[3 * 16 + 5, 1] = np.nextafter(moved[3 * 16 + 5, 1], np.inf)         # one rise of one run, one ulp
    assert shared(moved, 16) == 0
    moved[3 * 16 + 5, 1] = np.nextafter(grid[3 * 16 + 5, 1], -np.inf)
    assert shared(moved, 16) == 0
    reordered = grid.copy()
    reordered[2 * 16:3 * 16, 1] = reordered[2 * 16:3 * 16, 1][::-1]            # the same rises in another order
    assert shared(reordered, 16) == 0
    assert shared(grid[:16], 16) == 0                                          # a single run: nothing to share
    c3 = build_grid(twists, rises, (1, 2, 3), tube_length=1000.0).params       # csym major over the same rises
    assert len(c3) == 3 * 6 * 16 and shared(c3, 16) == 1
    assert shared(grid[:40], 16) == 0                                          # not whole runs
    L = _lib.lib()
    assert L.hh_rise_columns_shared(None, 32, 16) == -1 and L.hh_rise_columns_shared(grid.ctypes.data_as(C.POINTER(C.c_double)), 32, 0) == -1


def geometry(n, apix, units):
    """rpx and slack as hh_set_geometry derives them (ball radius 2 apix, 24 tail bits, no tilt / psi)."""
    br = 2.0 * apix
    sigma2 = br * br / np.log(2.0)
    rpx = max(1, int(np.ceil(np.sqrt(sigma2 * 24 * np.log(2.0)) / apix)))
    slack = float(F32(max(abs(z) for z in units) + 1e-3))
    return rpx, slack


def rows_that_reach(n, apix, rpx, units, rise, i):
    """The device's float32 window test (column_factors_of) for subunit indices i of every unit: does row (i, u) pass
    |x - cx| <= rpx for some column x in [0, n - 1]?  xc = f32(z_u) + f32(i rise), cx = xc inv_apix + n/2, all float32.
    The nearest columns decide, so only they are tried."""
    inv_apix = F32(1.0 / apix)
    hit = np.zeros(len(i), dtype=bool)
    for z in units:
        xc = F32(z) + (i.astype(np.float64) * rise).astype(F32)
        cx = xc * inv_apix + F32(n // 2)
        assert xc.dtype == F32 and cx.dtype == F32
        lo = np.clip(np.floor(cx), 0, n - 1).astype(F32)
        hi = np.clip(np.floor(cx) + 1, 0, n - 1).astype(F32)
        hit |= (np.abs(lo - cx) <= F32(rpx)) | (np.abs(hi - cx) <= F32(rpx))
    return hit


@pytest.mark.parametrize("n", [32, 64, 512])
@pytest.mark.parametrize("apix", [1.0, 5.0])
@pytest.mark.parametrize("units", [(0.0,), (-7.25, 11.5)], ids=["one_unit", "two_units"])
def test_table_extent_contains_every_row_the_window_test_passes(n, apix, units):
    L = _lib.lib()
    rpx, slack = geometry(n, apix, units)
    height = n * apix
    reach = (n / 2 + rpx) * apix + slack
    rises = [np.random.default_rng(n).uniform(1.5, 30.0, 2500)]
    ks = np.arange(1, int(reach / 1.5) + 1)
    edge = (reach / ks)
    edge = edge[(edge >= 1.5) & (edge <= 30.0)]
    edge32 = edge.astype(F32)
    rises += [edge, np.nextafter(edge, np.inf), np.nextafter(edge, -np.inf),                      # float64 neighbours
              edge32.astype(np.float64), np.nextafter(edge32, F32(np.inf)).astype(np.float64),   # float32 neighbours
              np.nextafter(edge32, F32(-np.inf)).astype(np.float64)]
    trimmed = 0
    for rise in np.concatenate(rises):
        full = int(np.ceil(height / rise))
        ext = int(L.hh_table_extent(n, apix, rpx, slack, float(rise)))
        assert 0 < ext <= full, (rise, ext, full)
        trimmed += ext < full
        if ext < full:                                  # every row outside the extent: no column takes it
            i = np.arange(ext + 1, full + 1)
            i = np.concatenate([-i, i])
            out = rows_that_reach(n, apix, rpx, units, float(rise), i)
            assert not out.any(), (rise, ext, i[out][:4])
    # a sanity check of the restatement itself: rows near the centre do reach
    assert rows_that_reach(n, apix, rpx, units, 4.0, np.arange(-3, 4)).all()
    if n == 512:                                        # the lattice spans +-n pixels, the image +-n/2: most rises trim
        assert trimmed > 2000


def test_table_extent_arguments():
    L = _lib.lib()
    assert L.hh_table_extent(64, 2.0, 10, 1e-3, 0.0) == -1 and L.hh_table_extent(64, 0.0, 10, 1e-3, 5.0) == -1
    assert L.hh_table_extent(0, 2.0, 10, 1e-3, 5.0) == -1 and L.hh_table_extent(64, 2.0, 10, 1e-3, float("nan")) == -1
    # 512 px at 1 A, rpx 10: reach = 266.001 A.  rise 1: floor(266.004) + 1 = 267 of the lattice's 512; rise 300: the
    # lattice's own ceil(512 / 300) = 2 is cut to 1 (row 2 sits 600 A out); rise 600: the lattice has 1 row either side
    assert L.hh_table_extent(512, 1.0, 10, 1e-3, 1.0) == 267
    assert L.hh_table_extent(512, 1.0, 10, 1e-3, 300.0) == 1 and L.hh_table_extent(512, 1.0, 10, 1e-3, 600.0) == 1
