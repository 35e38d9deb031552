"""Every compiled form of the tuned sweep's scoring kernels: size x segments x spectrum x path (tests/sweep_variants.py).

test_matrix sweeps each of the 24 (N, segments, log) rows on the transform, run-table and fused pipelines, the fused one
with the walk forced to rises and to twists: together `k_fused_pass<N, EPI, LOG, WALK>` for every N, EPI_SCORE / EPI_QSTORE,
LOG 0 / 1 and both walks (44 kernels) and `launch_second<N, EPI, LOG>` for the same sizes.  After every sweep
`last_first_pass`, `last_fused_walk` and `last_factor_sets` say which code ran — a silent fallback fails.  The two walks are
the same arithmetic (`set_fused_walk`): `array_equal`.  Every path is held against `oracle.path_b.sweep_cpu` in float64:
log spectra at the 2e-5 of tests/test_gpu_twist_walk.py, linear ones at LINEAR_TOL[N], which comes from the recorded
distance of the transform path from the same oracle and never from the fused pass (tests/sweep_variants.py).

test_compact_q_edges: several segments under two masks that put the compact q's layout at its edges (no weight in ky block
0; weight in ky block 0 only).  test_forms_in_sequence: one engine through log / linear and one / three segments in turn,
against fresh engines, for what a context keeps between launches (slot caches, table capacities, q row offsets).
"""
import numpy as np
import pytest

import helicon_amd as H
from tests import sweep_variants as SV

pytestmark = pytest.mark.gpu


def engine(case):
    eng = H.SweepEngine(case.n)
    eng.set_geometry(**case.geometry)
    return eng


def sweep_on(eng, case, path, grid):
    """The grid's scores on `path`, after asserting that this path ran."""
    mode, walk = SV.PATHS[path]
    eng.set_table_path(mode)
    eng.set_fused_walk(walk)
    scores = eng.sweep(grid)
    ran = (eng.last_first_pass, eng.last_fused_walk, eng.last_factor_sets)
    assert ran == case.expected(path), (case.id, path, ran)
    assert scores.shape == (case.segments, len(grid)), (case.id, path)
    assert np.isfinite(scores).all() and (scores.std(axis=1) > 0).all(), (case.id, path)
    return scores


def check_footprint(eng, case, ky_blocks=None):
    """The fused pass fits with both walks resident (the report test_long_table_with_the_factor_rows_at_their_limit reads)."""
    f = eng.fused_walk_footprint(float(case.rises.min()))
    print(f"{case.id}: footprint {f}")
    assert 0 < f["kg"] <= 16 and f["per_cu_rises"] > 0
    if SV.twist_walk_built(case.n):
        assert f["per_cu_twists"] >= f["per_cu_rises"]
    else:
        assert f["per_cu_twists"] == 0 and f["lds_twists"] == 0
    if ky_blocks is not None:
        assert f["ky_blocks"] == ky_blocks
    return f


def check_walks_agree(got, case):
    assert np.array_equal(got["fused/rises"], got["fused/twists"]), case.id
    assert np.array_equal(np.argmax(got["fused/rises"], axis=1), np.argmax(got["fused/twists"], axis=1))


def check_oracle(case, got, ref, picks, tol, what=""):
    errs = {path: float(np.abs(s[:, picks] - ref).max()) for path, s in got.items()}
    print(f"{case.id}{what}: max |score - oracle| over {len(picks)} candidates x {case.segments} segments, tolerance {tol:.1e}: "
          + ", ".join(f"{p} {e:.3e}" for p, e in errs.items()))
    for path, s in got.items():
        np.testing.assert_allclose(s[:, picks], ref, rtol=0, atol=tol, err_msg=f"{case.id}{what} {path}")
    return errs


@pytest.mark.parametrize("case", SV.CASES, ids=lambda c: c.id)
def test_matrix(case):
    grid, picks = case.grid, case.picks
    assert len(picks) >= SV.MIN_PICKS[case.n]
    assert not SV.UNREACHABLE                      # every form of the table is swept; an entry needs its own assertion here
    got = {}
    with engine(case) as eng:
        imgs = SV.images(case, eng.simulate)
        eng.set_reference(imgs, log=case.log)
        check_footprint(eng, case, ky_blocks=case.n // 16)
        for path in SV.PATHS:
            got[path] = sweep_on(eng, case, path, grid)
    check_walks_agree(got, case)
    ref = SV.oracle_scores(case, imgs, picks)
    errs = check_oracle(case, got, ref, picks, case.tol)
    if not case.log:
        # the yardstick itself: a transform path that drifts from its recorded distance moves LINEAR_TOL's footing
        print(f"{case.id}: transform against the oracle {errs['transform']:.3e} (recorded maximum at this size "
              f"{SV.TRANSFORM_LINEAR_ERR[case.n]:.3e})")


@pytest.mark.parametrize("name", SV.EDGE_MASKS)
@pytest.mark.parametrize("n", SV.EDGE_SIZES)
def test_compact_q_edges(n, name):
    case, mask = SV.edge_case(n), SV.edge_mask(n, name)
    grid, picks = case.grid, case.picks
    assert case.log and case.segments == (2 if n == 512 else 3) and len(picks) >= SV.MIN_PICKS[n]
    got = {}
    with engine(case) as eng:
        imgs = SV.images(case, eng.simulate)
        eng.set_reference(imgs, mask, log=True)
        check_footprint(eng, case, ky_blocks=SV.edge_ky_blocks(n, name))
        for path in ("fused/rises", "fused/twists"):
            got[path] = sweep_on(eng, case, path, grid)
    check_walks_agree(got, case)
    check_oracle(case, got, SV.oracle_scores(case, imgs, picks, mask), picks, SV.PIPE_TOL, what=f" {name}")


SEQUENCE = [(True, 1), (False, 3), (True, 3), (False, 1)]      # (log, segments), in this order on one engine


def test_forms_in_sequence():
    n = 128
    base = SV.Case(n, 3, True)
    grid = base.grid
    with engine(base) as eng:
        imgs = SV.images(base, eng.simulate)
        kept = []
        for log, segments in SEQUENCE:
            case = SV.Case(n, segments, log)
            eng.set_reference(imgs[:segments], log=log)
            kept.append({path: sweep_on(eng, case, path, grid) for path in ("fused/rises", "fused/twists")})
    for (log, segments), got in zip(SEQUENCE, kept):
        case = SV.Case(n, segments, log)
        with engine(case) as fresh:
            fresh.set_reference(imgs[:segments], log=log)
            for path in ("fused/rises", "fused/twists"):
                assert np.array_equal(got[path], sweep_on(fresh, case, path, grid)), (case.id, path)
        check_walks_agree(got, case)
