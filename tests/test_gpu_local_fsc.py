"""The local resolution map on the device (hh_lres_*; helicon_amd/local_resolution.py) against the float64 yardstick
(tests/local_fsc_cases.py), on both routes.

Per case: (a) every curve within the route's bound of the yardstick's (local_fsc_cases.TOL_CURVE: the largest difference
measured on an MI355X over these cases, profiles/local_fsc.json "accuracy", times 4); (b) every returned resolution equals
resolution_from_curve of the device's own curve in float64, to 1e-12 relative; (c) on every window whose yardstick curve has no
shell k >= 1 within 1e-4 of the threshold (at most 2 % of a case may be left out; tests/test_local_fsc_host.py shows the
yardstick alone stays within that) the branch and k* equal the yardstick's, and on the interpolated branch
|1 / res - 1 / res_yardstick| <= (saxis[1] - saxis[0]) 2 bound / |fsc[k*] - fsc[k* - 1]|, the rule's own error propagation.
Every test prints its figure before it asserts."""
import numpy as np
import pytest

import local_fsc_cases as Y
from helicon_amd.local_resolution import LocalFSC, local_resolution, resolution_from_curve, upsample_grid

pytestmark = pytest.mark.gpu

_ids = lambda v: str(v).replace(" ", "")   # noqa: E731


def _compare(r, want, w, thr, route, label):
    bound = Y.TOL_CURVE[route]
    assert r.route == route and r.curves.shape == want["curves"].shape and r.resolution.dtype == np.float64
    for got, axis in zip(r.centres, want["centres"]):
        assert np.array_equal(got, axis)
    err = float(np.abs(r.curves - want["curves"]).max())
    print(f"LFSC_FIGURE {label} route={route} thr={thr} windows={r.resolution.size} curve={err:.3e}")
    assert err <= bound                                                                        # (a)
    curves, res = r.curves.reshape(-1, w // 2 + 1), r.resolution.reshape(-1)
    for f, v in zip(curves, res):                                                              # (b)
        assert v == pytest.approx(resolution_from_curve(f, w, Y.APIX, thr), rel=1e-12)
    near = Y.near_threshold(want["curves"], thr).reshape(-1)
    assert near.sum() <= Y.MAX_EXCLUDED * near.size
    ds = 1.0 / (w * Y.APIX)
    wc, wr = want["curves"].reshape(-1, w // 2 + 1), want["resolution"].reshape(-1)
    wb, wk = want["branch"].reshape(-1), want["kstar"].reshape(-1)
    worst = 0.0
    for i in np.flatnonzero(~near):                                                            # (c)
        _, branch, k = Y.resolution_from_curve(curves[i], w, Y.APIX, thr)
        assert (branch, k) == (wb[i], wk[i]), (label, i)
        if branch == "first":
            assert res[i] == w * Y.APIX
        elif branch == "nyquist":
            assert res[i] == pytest.approx(2 * Y.APIX, rel=1e-12)
        else:
            allowed = ds * 2 * bound / abs(wc[i, k] - wc[i, k - 1])
            d = abs(1.0 / res[i] - 1.0 / wr[i])
            worst = max(worst, d / allowed)
            assert d <= allowed, (label, i, d, allowed)
    print(f"LFSC_FIGURE {label} route={route} thr={thr} excluded={int(near.sum())} worst share of the resolution allowance={worst:.3f}")


def _case(shape, w, step, route, thr=0.5):
    h1, h2 = Y.make_halves(shape)
    r = local_resolution(h1, h2, Y.APIX, window=w, step=step, threshold=thr, return_curves=True, route=route)
    _compare(r, Y.case(shape, w, step, thr), w, thr, route, f"{shape} w={w} s={step}")
    return r


@pytest.mark.parametrize("shape,w,step", Y.LDS_CASES, ids=_ids)
def test_lds_route_every_window_side(shape, w, step):
    r = _case(shape, w, step, "lds")
    auto = local_resolution(*Y.make_halves(shape), Y.APIX, window=w, step=step, return_curves=True)
    assert auto.route == "lds" and np.array_equal(auto.curves, r.curves) and np.array_equal(auto.resolution, r.resolution)
    assert r.kernel_ms > 0


@pytest.mark.parametrize("shape,w,step", Y.PASSES_CASES, ids=_ids)
def test_passes_route(shape, w, step):
    r = _case(shape, w, step, "passes")
    if w > 24:
        auto = local_resolution(*Y.make_halves(shape), Y.APIX, window=w, step=step, return_curves=True)
        assert auto.route == "passes" and np.array_equal(auto.curves, r.curves)
        with pytest.raises(ValueError, match="LDS route"):
            local_resolution(*Y.make_halves(shape), Y.APIX, window=w, step=step, route="lds")


@pytest.mark.parametrize("shape,w,step", Y.BOTH_CASES, ids=_ids)
@pytest.mark.parametrize("thr", Y.THRESHOLDS)
def test_both_routes_at_both_thresholds(shape, w, step, thr):
    a = _case(shape, w, step, "lds", thr)
    b = _case(shape, w, step, "passes", thr)
    print(f"LFSC_FIGURE {shape} w={w} lds against passes: {float(np.abs(a.curves - b.curves).max()):.3e}")
    assert np.abs(a.curves - b.curves).max() <= Y.TOL_CURVE["lds"] + Y.TOL_CURVE["passes"]


SHAPE, W, STEP = (13, 11, 14), 8, 4
ROUTES = ("lds", "passes")


@pytest.mark.parametrize("route", ROUTES)
def test_identical_halves_never_cross(route):
    h1, _ = Y.make_halves(SHAPE)
    r = local_resolution(h1, h1, Y.APIX, window=W, step=STEP, return_curves=True, route=route)
    assert (r.curves == 1.0).all()                        # num, den1 and den2 are the same integers
    assert (r.resolution == resolution_from_curve(np.ones(W // 2 + 1), W, Y.APIX, 0.5)).all() and r.resolution[0, 0, 0] == pytest.approx(2 * Y.APIX)


@pytest.mark.parametrize("route", ROUTES)
def test_negated_half_crosses_at_the_first_shell(route):
    h1, _ = Y.make_halves(SHAPE)
    r = local_resolution(h1, -h1, Y.APIX, window=W, step=STEP, return_curves=True, route=route)
    assert (r.curves == -1.0).all() and (r.resolution == W * Y.APIX).all()


@pytest.mark.parametrize("route", ROUTES)
def test_slab_of_zeros_gives_ratio_one(route):
    shape = (24, 11, 14)
    a, b = (h.copy() for h in Y.make_halves(shape))
    a[:12] = 0
    b[:12] = 0
    r = local_resolution(a, b, Y.APIX, window=W, step=STEP, return_curves=True, route=route)
    want = Y.local_fsc(a, b, Y.APIX, W, STEP)
    assert (want["curves"][0] == 1.0).all()               # the windows around z = 2 see zeros only
    assert (r.curves[0] == 1.0).all() and (r.resolution[0] == resolution_from_curve(np.ones(W // 2 + 1), W, Y.APIX, 0.5)).all()
    err = float(np.abs(r.curves - want["curves"]).max())
    print(f"LFSC_FIGURE slab route={route} curve={err:.3e}")
    assert err <= Y.TOL_CURVE[route]


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("taper", ((0.8, 0.1), (0.0, 0.5)), ids=("late", "off"))
def test_other_tapers(route, taper):
    h1, h2 = Y.make_halves(SHAPE)
    r = local_resolution(h1, h2, Y.APIX, window=W, step=STEP, taper=taper, return_curves=True, route=route)
    want = Y.local_fsc(h1, h2, Y.APIX, W, STEP, taper=taper)
    base = Y.case(SHAPE, W, STEP)
    assert np.abs(want["curves"] - base["curves"]).max() > 1e-2      # another taper is another curve
    err = float(np.abs(r.curves - want["curves"]).max())
    print(f"LFSC_FIGURE taper={taper} route={route} curve={err:.3e}")
    assert err <= Y.TOL_CURVE[route]
    for f, v in zip(r.curves.reshape(-1, W // 2 + 1), r.resolution.reshape(-1)):
        assert v == pytest.approx(resolution_from_curve(f, W, Y.APIX, 0.5), rel=1e-12)


@pytest.mark.parametrize("route", ROUTES)
def test_mask_drops_centres(route):
    h1, h2 = Y.make_halves(SHAPE)
    mask = np.ones(SHAPE, dtype=bool)
    mask[:, :, :7] = False                                 # the centres x = 2 and x = 6 go, x = 10 stays
    mask[6, 6, 10] = False
    with LocalFSC(h1, h2) as ctx:
        full = ctx.run(Y.APIX, W, STEP, return_curves=True, route=route)
        part = ctx.run(Y.APIX, W, STEP, mask=mask, return_curves=True, route=route)
    keep = mask[np.ix_(*full.centres)]
    assert 0 < keep.sum() < keep.size and not keep[1, 1, 2]
    assert np.isnan(part.resolution[~keep]).all() and np.isnan(part.curves[~keep]).all()
    assert np.array_equal(part.resolution[keep], full.resolution[keep]) and np.array_equal(part.curves[keep], full.curves[keep])
    assert not np.isnan(full.resolution).any()
    none = LocalFSC(h1, h2).run(Y.APIX, W, STEP, mask=np.zeros(SHAPE, dtype=bool), route=route)
    assert np.isnan(none.resolution).all() and none.route == route


@pytest.mark.parametrize("route", ROUTES)
def test_permuted_centres_and_chunked_budgets_give_the_same_bits(route):
    h1, h2 = Y.make_halves(SHAPE)
    axes = [Y.window_centres(n, STEP) for n in SHAPE]
    cen = np.stack([g.ravel() for g in np.meshgrid(*axes, indexing="ij")], axis=1)
    perm = np.random.default_rng(5).permutation(len(cen))
    with LocalFSC(h1, h2) as ctx:
        res, cur, taken, _ = ctx.run_centres(Y.APIX, W, cen, return_curves=True, route=route)
        again = ctx.run_centres(Y.APIX, W, cen, return_curves=True, route=route)
        assert taken == route and np.array_equal(again[0], res) and np.array_equal(again[1], cur)        # run to run
        res_p, cur_p, _, _ = ctx.run_centres(Y.APIX, W, cen[perm], return_curves=True, route=route)
        assert np.array_equal(res_p, res[perm]) and np.array_equal(cur_p, cur[perm])
        budgets = [dict(max_windows_per_launch=1), dict(max_windows_per_launch=3)]
        if route == "passes":
            budgets.append(dict(scratch_bytes=3 * 10 * W ** 3 * 4))         # three windows' planes
        for budget in budgets:
            ctx.set_budget(**budget)
            res_b, cur_b, _, _ = ctx.run_centres(Y.APIX, W, cen, return_curves=True, route=route)
            assert np.array_equal(res_b, res) and np.array_equal(cur_b, cur), budget
        ctx.set_budget(0, 0)
        # another window on the same context, then the first one again: the scratch follows
        ctx.run_centres(Y.APIX, 10, cen[:4], route=route)
        res_c, cur_c, _, _ = ctx.run_centres(Y.APIX, W, cen, return_curves=True, route=route)
        assert np.array_equal(res_c, res) and np.array_equal(cur_c, cur)
        for bad in ([[-1, 5, 5]], [[5, SHAPE[1], 5]], [[5, 5, SHAPE[2]]]):
            with pytest.raises(ValueError, match="outside the map"):
                ctx.run_centres(Y.APIX, W, np.asarray(bad), route=route)


def test_upsample_against_the_yardstick():
    rng = np.random.default_rng(11)
    cases = []
    for shape, step in (((13, 11, 14), 4), ((9, 40, 9), 16), ((8, 8, 8), 12), ((17, 16, 31), 5), ((10, 12, 9), 1)):
        grid_shape = tuple(len(Y.window_centres(n, step)) for n in shape)
        grid = rng.uniform(3.0, 20.0, grid_shape)
        cases.append((grid, step, shape))
        if grid.size > 1:
            holed = grid.copy()
            holed.reshape(-1)[rng.permutation(grid.size)[: max(1, grid.size // 3)]] = np.nan
            cases.append((holed, step, shape))
        cases.append((np.full(grid_shape, np.nan), step, shape))
    assert any(1 in g.shape and max(g.shape) > 1 for g, _, _ in cases)
    for grid, step, shape in cases:
        want = Y.upsample(grid, step, shape)
        got = upsample_grid(grid, step, shape)
        assert got.dtype == np.float32 and got.shape == shape
        assert np.array_equal(np.isnan(got), np.isnan(want))
        ok = ~np.isnan(want)
        if ok.any():
            err = float((np.abs(got[ok] - want[ok]) / np.abs(want[ok])).max())
            print(f"LFSC_FIGURE upsample grid={grid.shape} step={step} nan={int(np.isnan(grid).sum())} rel={err:.3e}")
            assert err <= 1e-6


def test_resolution_map_of_a_run():
    h1, h2 = Y.make_halves(SHAPE)
    r = local_resolution(h1, h2, Y.APIX, window=W, step=STEP)
    m = r.resolution_map()
    assert r.curves is None and m.dtype == np.float32 and m.shape == SHAPE
    want = Y.upsample(r.resolution, STEP, SHAPE)
    assert np.abs(m - want).max() <= 1e-6 * np.abs(want).max()
    zz, yy, xx = np.ix_(*r.centres)
    assert np.array_equal(m[zz, yy, xx], r.resolution.astype(np.float32))      # a centre carries its own window's value
