"""The two cuts of sweep_runs (csrc/helicon_hip.hip) that no other GPU test crosses ("The sweep drivers in phases"):

* more than one table group: HH_TABLE_BYTES_MAX is 1 GB, so the list has to carry more than 1 GB of run tables.  Side 256 at
  1 A, ball radius 0.2 A (truncation half-window 1 px), rises 0.360 ... 0.374 A: 359 subunit indices either side, 719 table
  rows, 736,256 bytes per run, 1,458 runs per group; 3,000 runs of 8 are groups of 1,458, 1,458 and 84 runs;
* per-launch column factors in alternating halves over more than two launches: one run of 60,000 distinct rises at side 32
  with two segments (24,576 candidates per launch): launches of 24,576, 24,576 and 10,848.

tests/sweep_plan_check.cpp asserts both cuts from sweep_plan.h on these very numbers.  Each list is swept in one call and in
short calls that each lie inside one group / one launch, bit for bit: that comparison is what covers every candidate.
oracle.path_b (at sweep_variants.SCORE_TOL) ties down a thin test_gpu_launch_cuts.sample() only: at side 256 with 1,425
subunits per candidate the oracle takes 0.5 s per candidate, so of the 24,000 candidates of the table groups it sees 8 —
the first two, the last two and the one on each side of each cut; of the one long run it sees every 250th and 8 on each
side of each cut (275).  Every test prints its figures and its wall time before it asserts.  Measured on an MI355X: both bit-identical
to their short calls; largest distance from the oracle 1.9e-8 (table groups, 59 sampled) and 8.2e-7 (three launches);
device part 0.38 s and 0.29 s."""
import time

import numpy as np
import pytest

import helicon_amd as H
from oracle import path_b as O
from tests import sweep_variants as SV
from tests.test_gpu_launch_cuts import sample

pytestmark = pytest.mark.gpu

GROUP_RUNS, RUN_LEN, RUNS = 1458, 8, 3000          # table groups at side 256 (sweep_plan_check.cpp: check_gpu_test_lists)
PIECE, ONE_RUN = 24576, 60000                       # launches of one run with two segments at side 32


def noisy(eng, truth, segments):
    clean = eng.simulate(*truth)
    return np.stack([(clean + np.random.default_rng(s).normal(0, 0.5 * clean.std(), clean.shape)).astype(np.float32)
                     for s in range(segments)])


def short_calls(eng, params, chunks, step):
    """The list in calls of `step` candidates (the last of a chunk: what is left), none across a chunk's end."""
    out = []
    for c0, c1 in chunks:
        out += [eng.sweep(params[lo:min(c1, lo + step)]) for lo in range(c0, c1, step)]
    return np.concatenate(out, axis=1)


def against_oracle(got, imgs, params, idx, n, apix, d, br, what):
    mask = O.radial_band_mask(n, n)
    worst = 0.0
    for s, img in enumerate(imgs):
        ref = O.sweep_cpu(img, params[idx, :3], mask, apix=apix, helical_diameter=d, ball_radius=br)
        worst = max(worst, float(np.abs(got[s][idx] - ref).max()))
    print(f"{what}: max |score - oracle| over {len(idx)} sampled candidates x {len(imgs)} images = {worst:.3e}")
    return worst


def test_three_table_groups():
    t0 = time.perf_counter()
    n, apix, br = 256, 1.0, 0.2
    d = 0.4 * n * apix
    twists, rises = 20.0 + 0.01 * np.arange(RUNS), 0.36 + 0.002 * np.arange(RUN_LEN)
    params = np.ascontiguousarray(np.array([(t, r, 1.0, 0.0) for t in twists for r in rises]))
    g = len(params)
    cuts = [GROUP_RUNS * RUN_LEN, 2 * GROUP_RUNS * RUN_LEN]
    assert cuts[1] < g < 3 * GROUP_RUNS * RUN_LEN
    with H.SweepEngine(n) as eng:
        eng.set_geometry(apix=apix, helical_diameter=d, ball_radius=br)
        imgs = noisy(eng, (float(twists[1500]), float(rises[3]), 1), 1)
        eng.set_reference(imgs[0], O.radial_band_mask(n, n), log=True)
        long = eng.sweep(params)
        assert eng.last_first_pass == "fused" and eng.last_factor_sets == RUN_LEN
        # 500 runs a call: 500, 500, 458 runs in each full group, 84 in the last
        short = short_calls(eng, params, [(0, cuts[0]), (cuts[0], cuts[1]), (cuts[1], g)], 500 * RUN_LEN)
    t_device = time.perf_counter() - t0
    same = np.array_equal(long, short)
    print(f"three table groups: {g} candidates, one call against short calls bit-identical: {same}; "
          f"max |difference| = {float(np.abs(long.astype(np.float64) - short).max()):.3e}")
    idx = sample(g, cuts, stride=g, side=1)      # the first two, the last two, the candidate on each side of each cut
    worst = against_oracle(long, imgs, params, idx, n, apix, d, br, "three table groups")
    print(f"three table groups: wall time {time.perf_counter() - t0:.2f} s (device part {t_device:.2f} s)")
    assert long.shape == (1, g) and np.isfinite(long).all() and same
    assert worst <= SV.SCORE_TOL


def test_unshared_factor_halves_over_three_launches():
    t0 = time.perf_counter()
    n, apix = 32, 2.0
    d, br = 0.4 * n * apix, 2 * apix
    params = np.zeros((ONE_RUN, 4))
    params[:, 0], params[:, 1], params[:, 2] = 28.0, np.linspace(6.0, 14.0, ONE_RUN), 1.0
    cuts = [PIECE, 2 * PIECE]
    assert cuts[1] < ONE_RUN < 3 * PIECE
    with H.SweepEngine(n) as eng:
        eng.set_geometry(apix=apix, helical_diameter=d, ball_radius=br)
        imgs = noisy(eng, (28.0, 10.0, 1), 2)
        eng.set_reference(imgs, O.radial_band_mask(n, n), log=True)
        long = eng.sweep(params)
        assert eng.last_first_pass == "fused" and eng.last_factor_sets == ONE_RUN     # per-candidate sets: nothing shared
        short = short_calls(eng, params, [(0, cuts[0]), (cuts[0], cuts[1]), (cuts[1], ONE_RUN)], 7000)
    t_device = time.perf_counter() - t0
    same = np.array_equal(long, short)
    print(f"three launches of one run: one call against short calls bit-identical: {same}; "
          f"max |difference| = {float(np.abs(long.astype(np.float64) - short).max()):.3e}")
    idx = sample(ONE_RUN, cuts, stride=250, side=8)
    worst = against_oracle(long, imgs, params, idx, n, apix, d, br, "three launches of one run")
    print(f"three launches of one run: wall time {time.perf_counter() - t0:.2f} s (device part {t_device:.2f} s)")
    assert long.shape == (2, ONE_RUN) and np.isfinite(long).all() and same
    assert worst <= SV.SCORE_TOL
