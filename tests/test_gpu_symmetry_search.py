"""The helical symmetry search of a 3-D map on the device (csrc/symmetry_search.inc, helicon_amd/symmetry_search.py) against
the oracle composition it is defined by:

    S = oracle.symmetrize.apply_helical_symmetry(V, apix, twist, rise, csym, fraction, V.shape, apix)
    score = oracle.path_b.cross_correlation_coefficient(V[M], S[M])

Tolerance: 2e-4 absolute on every score and the same arg-max — the project's figure for sweep scores against the oracle
(DESIGN.md section 1).  Every test prints the largest difference it saw.  A test that asserts an arg-max first checks that
the ORACLE's two best scores are more than 1e-3 apart (five times the tolerance), so that it cannot pass or fail on a
coin toss of its own input.
"""
import itertools

import numpy as np
import pytest

import helicon_amd as H
from helicon_amd.symmetry_search import SymmetrySearch, helical_symmetry_search
from oracle import path_b as O
from oracle import symmetrize as S

pytestmark = pytest.mark.gpu

TOL = 2e-4
UNIT = ((1.0, 0.0, 0.0), (0.6, 40.0, 1.5))   # balls of the asymmetric unit: (radius / R, azimuth degrees, z offset Angstrom)


def helix_map(shape, apix, twist, rise, csym=1, radius=14.0, sigma=3.0):
    """A helix of Gaussian balls exp(-d^2 / sigma^2) on voxel coordinates (index - n // 2) * apix, float32."""
    nz, ny, nx = shape
    z, y, x = ((np.arange(n) - n // 2) * float(apix) for n in (nz, ny, nx))
    vol = np.zeros(shape, dtype=np.float64)
    imax = int(np.ceil(nz * apix / rise))
    for i in range(-imax, imax + 1):
        for c in range(csym):
            for rho, az, dz in UNIT:
                a = np.deg2rad(twist * i + 360.0 * c / csym + az)
                ez = np.exp(-((z - (i * rise + dz)) ** 2) / sigma**2)
                ey = np.exp(-((y - rho * radius * np.sin(a)) ** 2) / sigma**2)
                ex = np.exp(-((x - rho * radius * np.cos(a)) ** 2) / sigma**2)
                vol += ez[:, None, None] * ey[None, :, None] * ex[None, None, :]
    return vol.astype(np.float32)


def add_noise(vol, seed, level=0.5):
    sd = level * np.std(vol[vol > 1e-3])
    return (vol + np.random.default_rng(seed).normal(scale=sd, size=vol.shape)).astype(np.float32)


def region_mask(shape, rmin=0, rmax=..., z_fraction=0.5):
    nz, ny, nx = shape
    if rmax is ...:
        rmax = min(ny, nx) // 2 - 1
    k, j, i = np.meshgrid(np.arange(nz) - nz // 2, np.arange(ny) - ny // 2, np.arange(nx) - nx // 2, indexing="ij")
    r2 = j * j + i * i
    m = r2 >= rmin**2
    if rmax is not None:
        m &= r2 < rmax**2
    if z_fraction < 1:
        h = max(1, int(nz * z_fraction + 0.5) // 2)
        m &= (k >= -h) & (k < h)
    return m


def oracle_scores(vol, apix, params, mask, fraction=1.0):
    out = []
    for tw, rs, cs in params:
        sym = S.apply_helical_symmetry(vol, apix, float(tw), float(rs), int(cs), fraction, vol.shape, apix)
        out.append(float(O.cross_correlation_coefficient(vol[mask], sym[mask])))
    return np.asarray(out)


def well_separated(ref, what):
    top = np.sort(ref)[::-1]
    assert top[0] - top[1] > 1e-3, (f"{what}: the oracle's two best scores are {top[0]:.6f} and {top[1]:.6f}, less than 1e-3 apart — "
                                    "this INPUT cannot carry an arg-max assertion; change its seed")


GRID_T, GRID_R = np.arange(26.0, 32.5, 1.0), np.arange(4.5, 7.75, 0.5)
SMALL = dict(shape=(32, 24, 24), apix=2.0, twist=29.0, rise=6.0)


@pytest.mark.parametrize("name,noise,fraction,region", [
    ("clean", None, 1.0, {}),
    ("noise", 11, 1.0, {}),
    ("fraction", 12, 0.5, dict(rmax=None, z_fraction=1.0)),
    ("shell", 13, 1.0, dict(rmin=3, rmax=11, z_fraction=0.5)),
])
def test_grid_scores_and_argmax_match_the_oracle(name, noise, fraction, region):
    vol = helix_map(**SMALL)
    if noise is not None:
        vol = add_noise(vol, noise)
    mask = region_mask(vol.shape, **region)
    res = helical_symmetry_search(vol, 2.0, GRID_T, GRID_R, (1,), fraction=fraction, **region)
    assert res.grid.valid.all()
    ref = oracle_scores(vol, 2.0, res.grid.params[:, :3], mask, fraction)
    well_separated(ref, name)
    got = res.scores.reshape(-1)
    err = float(np.abs(got - ref).max())
    print(f"symmetry search [{name}]: max |score - oracle| = {err:.3e} over {len(ref)} candidates, best {res.best[0]}")
    assert err < TOL
    assert int(res.best_index[0]) == int(np.argmax(ref))
    assert res.best[0][:3] == (29.0, 6.0, 1)
    if not region:
        assert int(mask.sum()) == 5968


def test_region_and_z_range_reported():
    vol = helix_map(**SMALL)
    with SymmetrySearch(vol, 2.0, fraction=0.5) as ss:
        assert ss.region_voxels == int(region_mask(vol.shape).sum()) == 5968
        prof = vol.sum(axis=(1, 2), dtype=np.float64)
        nzi = np.where(prof > 0.01 * prof.max())[0]
        z0, z1 = int(nzi[0]), int(nzi[-1])
        zmid = (z0 + z1) // 2 + (z0 + z1) % 2
        assert ss.z_range == (max(z0, zmid - 16 // 2), min(z1, zmid + 16 // 2))
        spec = ss.set_region(3, None, 1.0)
        assert ss.region_voxels == spec["region_voxels"] == int(region_mask(vol.shape, 3, None, 1.0).sum())


@pytest.mark.parametrize("region", [dict(rmax=None, z_fraction=1.0), dict(rmax=9, z_fraction=0.5)])
def test_odd_unequal_sides(region):
    """30 x 21 x 25: rows centred on ny // 2, columns on nx / 2 = 12.5 — the reference puts the axis between voxels there, and
    the oracle's own best is (30, 6) / (31, 6) rather than the map's (29, 6); only equality with the oracle is asserted."""
    full = helix_map((30, 25, 25), 2.0, 29.0, 6.0, radius=12.0)
    vol = add_noise(np.ascontiguousarray(full[:, 2:23, :]), 21)   # 21 rows about row 12: the axis stays on (ny // 2, nx // 2)
    assert vol.shape == (30, 21, 25)
    mask = region_mask(vol.shape, **region)
    res = helical_symmetry_search(vol, 2.0, GRID_T, GRID_R, (1,), **region)
    ref = oracle_scores(vol, 2.0, res.grid.params[:, :3], mask)
    well_separated(ref, f"odd sides {region}")
    got = res.scores.reshape(-1)
    err = float(np.abs(got - ref).max())
    print(f"symmetry search [30 x 21 x 25, {region}]: max |score - oracle| = {err:.3e}, best {res.best[0]}, oracle's "
          f"{tuple(res.grid.params[int(np.argmax(ref)), :3])}")
    assert err < TOL
    assert int(res.best_index[0]) == int(np.argmax(ref))


def test_csym_axis_on_a_c2_map():
    vol = helix_map((32, 24, 24), 2.0, 29.0, 6.0, csym=2)
    params = np.array([(tw, 6.0, cs) for tw in (28.0, 29.0, 30.0) for cs in (1, 2, 3)])
    mask = region_mask(vol.shape, rmax=None, z_fraction=1.0)
    with SymmetrySearch(vol, 2.0) as ss:
        ss.set_region(0, None, 1.0)
        got = ss.search(params)
    ref = oracle_scores(vol, 2.0, params, mask)
    err = float(np.abs(got - ref).max())
    print(f"symmetry search [C2 map, Csym 1 2 3]: max |score - oracle| = {err:.3e}; scores at the truth {got[3:6]}")
    assert err < TOL
    assert got[5] < got[4] - 0.1   # Csym 3 against Csym 2 at (29, 6); Csym 1 and 2 tie on a C2 map


def test_larger_maps():
    vol = add_noise(helix_map((64, 64, 64), 2.0, 29.0, 6.0, radius=40.0, sigma=4.0), 31)
    params = np.array([(tw, rs, 1.0) for tw, rs in itertools.product((28.0, 29.0, 30.0), (5.5, 6.0, 6.5))][:8])
    with SymmetrySearch(vol, 2.0) as ss:
        got = ss.search(params)
    ref = oracle_scores(vol, 2.0, params, region_mask(vol.shape))
    err = float(np.abs(got - ref).max())
    print(f"symmetry search [64^3]: max |score - oracle| = {err:.3e}")
    assert err < TOL

    vol = add_noise(helix_map((128, 128, 128), 2.0, 29.0, 6.0, radius=40.0, sigma=4.0), 32)
    params = np.array([(29.0, 6.0, 1.0), (28.0, 6.0, 1.0), (29.0, 5.5, 1.0), (29.0, 6.0, 2.0)])
    mask = region_mask(vol.shape)
    with SymmetrySearch(vol, 2.0) as ss:
        got = ss.search(params)
    ref = np.array([float(O.cross_correlation_coefficient(vol[mask], H.apply_helical_symmetry(vol, 2.0, tw, rs, int(cs))[mask]))
                    for tw, rs, cs in params])
    err = float(np.abs(got - ref).max())
    print(f"symmetry search [128^3, against apply_helical_symmetry's map]: max |score difference| = {err:.3e}")
    assert err < TOL


def test_bit_reproducible_and_independent_of_the_list():
    vol = add_noise(helix_map(**SMALL), 41)
    grid = np.array([(tw, rs, 1.0) for tw in np.arange(20.0, 40.0, 1.0) for rs in np.arange(4.0, 9.0, 1.0)])   # 100 candidates
    one = np.array([[29.0, 6.0, 1.0]])
    with SymmetrySearch(vol, 2.0) as ss:
        a, b = ss.search(grid), ss.search(grid)
        assert np.array_equal(a, b)
        alone = ss.search(one)
        mixed = np.concatenate([grid[:50], one, grid[50:]])
        got = ss.search(mixed)
        assert got[50] == alone[0]
        assert np.array_equal(np.delete(got, 50), a)
        assert np.array_equal(ss.search(mixed[::-1].copy())[::-1], got)
        assert ss.launches == 5   # the default budget holds each of these lists in one launch
    # the same list cut into many launches: a budget below one candidate's partial sums gives one candidate per launch
    with SymmetrySearch(vol, 2.0, partial_bytes=1) as cut:
        c = cut.search(grid)
        assert cut.launches == len(grid)
    assert np.array_equal(c, a)


def test_skipped_pairs_and_argument_errors():
    vol = add_noise(helix_map(**SMALL), 51)
    res = helical_symmetry_search(vol, 2.0, [0.0, 29.0], [0.005, 6.0, 40.0], (1,))   # length 64 A: rise 40 >= 32 is skipped
    sc = res.scores.reshape(-1)
    assert list(res.grid.valid) == [False, False, False, False, True, False]
    assert np.isneginf(sc[~res.grid.valid]).all() and np.isfinite(sc[4])
    assert int(res.best_index[0]) == 4 and res.best[0][:3] == (29.0, 6.0, 1)

    with SymmetrySearch(vol, 2.0) as ss:
        good = ss.search(np.array([[29.0, 6.0, 1.0]]))
        for bad, word in (((29.0, 0.0, 1.0), "rise"), ((29.0, -6.0, 1.0), "rise"), ((29.0, np.nan, 1.0), "rise"), ((29.0, 6.0, 0.0), "csym")):
            with pytest.raises(ValueError, match=f"candidate 2: {word}"):
                ss.search(np.array([[29.0, 6.0, 1.0], [28.0, 6.0, 1.0], bad]))
        L = ss._L
        assert L.hh_hs_set_region(ss._h, 50.0, 60.0, 0.5) == -1 and b"no voxel" in L.hh_hs_last_error(ss._h)   # past Python's own check
        with pytest.raises(ValueError, match="no voxel"):
            ss.search(np.array([[29.0, 6.0, 1.0]]))
        with pytest.raises(ValueError, match="no voxel"):
            ss.set_region(50, 60)
        ss.set_region()
        assert np.array_equal(ss.search(np.array([[29.0, 6.0, 1.0]])), good)   # the handle lives on
    with pytest.raises(ValueError, match="no density"):
        SymmetrySearch(np.zeros((16, 16, 16), np.float32), 2.0)


def test_two_handles_and_a_sweep_engine_side_by_side():
    vol_a = add_noise(helix_map(**SMALL), 61)
    vol_b = add_noise(helix_map((32, 24, 24), 2.0, 31.0, 5.0), 62)
    params = np.array([(tw, rs, 1.0) for tw in (29.0, 31.0) for rs in (5.0, 6.0)])
    n = 64
    clean = O.simulate_helical_projection(1, 29.0, 10.0, 1, 0.4 * n * 2.0, 4.0, 0, 0, n, n, 2.0)
    img = (clean + np.random.default_rng(0).normal(0, 0.5 * clean.std(), clean.shape)).astype(np.float32)
    sweep_kw = dict(apix=2.0, helical_diameter=0.4 * n * 2.0, ball_radius=4.0)
    tw2, rs2 = np.arange(27.0, 31.5, 1.0), np.arange(9.0, 11.5, 1.0)
    with SymmetrySearch(vol_a, 2.0) as ss:
        alone_a = ss.search(params)
    with SymmetrySearch(vol_b, 2.0) as ss:
        alone_b = ss.search(params)
    alone_2d = H.sweep(img, tw2, rs2, (1,), **sweep_kw).scores
    with SymmetrySearch(vol_a, 2.0) as sa, SymmetrySearch(vol_b, 2.0) as sb:
        a1 = sa.search(params)
        both_2d = H.sweep(img, tw2, rs2, (1,), **sweep_kw).scores
        b1 = sb.search(params)
        a2 = sa.search(params)
    assert np.array_equal(a1, alone_a) and np.array_equal(a2, alone_a) and np.array_equal(b1, alone_b)
    assert np.array_equal(both_2d, alone_2d)
    assert not np.array_equal(alone_a, alone_b)
