"""The pair build of the fused twist walk (N = 512) on the matrix pipe: what the build sees, varied.

The cases of tests/pair_handover_cases.py hold the geometry fixed (apix 1, ball radius 2, rises near 4.7 A: 6 or 7 table
rows per column group).  Here the table-row count per group, the first rows `cg`, the interleaving of rows and the window
change: the longest factor set that still fuses (kg = 16), rises of tens of angstrom (one or two rows, groups that no
row reaches), Csym 3, two axial units, ball radius 4 and a non-unit pixel size; pieces of 1 and 3 runs send dropped halves
through the accumulators, and three segments take the q-storing instantiation.

Every case forces the twist walk, asks `(last_first_pass, last_fused_walk) == ("fused", "twists")`, requires the bits of
the forced rise walk (which keeps the per-lane FMA build and the panel), and holds a handful of candidates against
`oracle.path_b.sweep_cpu` at the 2e-5 of the other sweep tests.  `sweep_cpu` has no argument for an explicit asymmetric
unit: the two-unit case holds its sample against the engine's per-candidate transform pipeline instead, as
tests/test_gpu_twist_pairs.py does.
"""
import numpy as np
import pytest

import helicon_amd as H
from helicon_amd.grid import build_grid
from oracle import path_b as O

pytestmark = pytest.mark.gpu

N = 512
TOL = 2e-5


class Case:
    def __init__(self, twists, rises, csyms=(1,), apix=1.0, ball=2.0, units=None, kg=None, segments=1, pieces=()):
        self.twists, self.rises, self.csyms = np.asarray(twists, float), np.asarray(rises, float), csyms
        self.apix, self.ball, self.units, self.kg, self.segments, self.pieces = apix, ball, units, kg, segments, pieces
        self.diameter = 0.4 * N * apix


T5, T4 = 2.0 + 0.25 * np.arange(5), 2.0 + 0.25 * np.arange(4)
# kg = (floor(((3 + 2 rpx) apix + 2 slack) / rise_min) + 2) units, rpx = ceil(4.9 ball / apix), slack = 1e-3 + the units' largest |z| (fused_shape)
CASES = {
    # ball radius 1: 13.002 / 0.87 = 14.9 -> kg 16, the factor buffer's limit (0.866 A would need 17 rows); 301 table rows a side
    "kg_ceiling": Case(T5, 0.87 + 0.01 * np.arange(8), ball=1.0, kg=16),
    # 23.002 / 30 < 1 -> kg 2: one or two rows per group, and column groups between the rows' windows that none reaches
    "long_rises": Case(T4, 30.0 + 1.5 * np.arange(8), kg=2),
    "long_rises_3_segments": Case(T5, 30.0 + 1.5 * np.arange(8), kg=2, segments=3),
    "csym_3": Case(T4, 4.60 + 0.05 * np.arange(8), csyms=(3,), kg=7),
    # two units: their rows interleave in the table and the slack takes the units' |z| <= 4.5: (floor((23 + 2 * 4.501) / 8) + 2) 2 = 12
    "two_units": Case(T4[:3], 8.0 + 0.05 * np.arange(8), csyms=(1, 3), units=((102.4, 0.0, -3.0), (80.0, 1.0, 4.5)), kg=12),
    # ball radius 4: 43.002 / 3.2 = 13.4 -> kg 15, a window of 41 pixels
    "ball_4": Case(T5, 3.20 + 0.05 * np.arange(8), ball=4.0, kg=15, pieces=(1, 3)),
    # apix 1.5, ball radius 3 (rpx 10): 34.502 / 7 = 4.9 -> kg 6
    "apix_1_5": Case(T4, 7.0 + 0.075 * np.arange(8), apix=1.5, ball=3.0, kg=6),
}


def noisy(eng, truth, seed):
    clean = eng.simulate(*truth)
    return (clean + np.random.default_rng(seed).normal(0, 0.5 * clean.std(), clean.shape)).astype(np.float32)


@pytest.mark.parametrize("name", list(CASES))
def test_walks_agree_and_match_the_oracle(name):
    c = CASES[name]
    grid = build_grid(c.twists, c.rises, c.csyms, tube_length=float(N) * c.apix).params
    runs, run_len = len(c.twists) * len(c.csyms), len(c.rises)
    assert grid.shape[0] == runs * run_len
    truth = (float(c.twists[1]), float(c.rises[3]), int(c.csyms[-1]))
    with H.SweepEngine(N) as eng:
        eng.set_geometry(apix=c.apix, helical_diameter=c.diameter, ball_radius=c.ball,
                         units=None if c.units is None else np.asarray(c.units, dtype=np.float64))
        imgs = noisy(eng, truth, 0) if c.segments == 1 else np.stack([noisy(eng, truth, s) for s in range(c.segments)])
        eng.set_reference(imgs)
        f = eng.fused_walk_footprint(float(c.rises.min()))
        print(f"{name}: footprint {f}")
        assert f["kg"] == c.kg and f["per_cu_twists"] >= f["per_cu_rises"] > 0
        out = {}
        for walk in ("rises", "twists"):
            eng.set_fused_walk(walk)
            out[walk] = eng.sweep(grid)
            assert (eng.last_first_pass, eng.last_fused_walk) == ("fused", walk)
        assert out["twists"].shape == (c.segments, len(grid))
        assert np.isfinite(out["rises"]).all() and out["rises"].std() > 0
        assert np.array_equal(out["rises"], out["twists"])
        for piece in c.pieces:       # (the twist walk is still forced)
            eng.set_fused_piece(piece)
            got = eng.sweep(grid)
            assert (eng.last_first_pass, eng.last_fused_walk) == ("fused", "twists")
            assert np.array_equal(got, out["twists"]), piece
        eng.set_fused_piece(0)
        eng.set_fused_walk("auto")
        # the truth (run 1 of its csym: a B half), the last candidate, and the first rise of run 2 (an A half)
        at_truth = int(np.flatnonzero((grid[:, 0] == truth[0]) & (grid[:, 1] == truth[1]) & (grid[:, 2] == truth[2]))[0])
        picks = {at_truth, runs * run_len - 1}
        if c.segments == 1 and c.kg < 16:    # (the oracle walks every lattice row: two candidates where there are a thousand)
            picks.add(min(2, runs - 1) * run_len)
        picks = sorted(picks)
        if c.units is not None:
            eng.set_table_path(0)
            ref = eng.sweep(grid[picks])
            assert eng.last_first_pass == "transform" and eng.last_fused_walk == "none"
    scores = out["twists"]
    for s, img in enumerate(np.asarray(imgs).reshape(-1, N, N)):
        if c.units is None:
            want = O.sweep_cpu(img, grid[picks, :3], O.radial_band_mask(N, N), apix=c.apix, helical_diameter=c.diameter,
                               ball_radius=c.ball)
        else:
            want = ref[s]
        print(f"{name} segment {s}: max |score - reference| over {picks} = {np.abs(scores[s, picks] - want).max():.3e}")
        np.testing.assert_allclose(scores[s, picks], want, rtol=0, atol=TOL)
