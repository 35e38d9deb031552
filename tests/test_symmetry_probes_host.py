"""What tests/test_gpu_symmetry_probes.py relies on, shown on the CPU oracle alone (tests/symmetry_probes.py has the cases):

  * the model's constants are the source's (helicon_amd/csrc/symmetry_search.inc), its window of repeats holds every
    repeat the reference admits, its ``sym_plane`` is the oracle's operator;
  * every coverage claim of the probes (the n_ent values, the tile layouts and np values, the rings' union, border flips,
    side parities and orders, the z ranges, the empty planes);
  * the sensitivity condition: a perturbation of the oracle's symmetrised map that imitates the guarded defect moves the
    oracle's score by at least SENSITIVITY = 1e-3 (five times the GPU test's TOL); every probe region holds at least 8
    voxels and both members' variance exceeds 1e-6 of their raw second moment.

Every test prints the figures it asserts on.  Where a perturbation CANNOT bite by arithmetic the test says so and asserts
that instead of leaving the case out: a list of exactly 257 entries with csym 1 ends on the window's widening, which is
never live, and a voxel that no candidate of a list reaches (S = 0: the far corners of an unequal plane) is probed by
admitting the identity there (S set to the map's value) instead of by losing it.
"""
import functools
import re
import time

import numpy as np
import pytest

import symmetry_probes as P
from oracle import path_b as O
from oracle import symmetrize as S
from test_gpu_symmetry_search import TOL, add_noise, helix_map, oracle_scores, region_mask

A = P.APIX


def oracle_sym(vol, cand, fraction=1.0):
    tw, rs, cs = cand
    return S.apply_helical_symmetry(vol, A, float(tw), float(rs), int(cs), fraction, vol.shape, A)


def score(vol, sym, mask):
    return float(O.cross_correlation_coefficient(vol[mask], sym[mask]))


def conditions(vol, sym, mask, what):
    assert int(mask.sum()) >= P.MIN_VOXELS, what
    assert P.variance_share(vol[mask]) > P.MIN_VARIANCE and P.variance_share(sym[mask]) > P.MIN_VARIANCE, what


def test_constants_and_tolerance_are_the_sources():
    text = P.source()
    assert TOL == P.TOL == 2e-4 and P.SENSITIVITY == 5 * TOL
    assert re.findall(r"constexpr int HS_VPT = (\d+);", text) == [str(P.HS_VPT)] == ["8"]
    assert "constexpr int HS_TILE = 256 * HS_VPT;" in text
    assert "__global__ __launch_bounds__(256) void k_hs_score(HsArgs a) {" in text
    assert "hipLaunchKernelGGL(k_hs_score, dim3((unsigned)p->nplanes, (unsigned)p->ntiles, n), dim3(256), 0, p->stream, a);" in text
    assert "for (long long e0 = 0; e0 < n_ent; e0 += 256) {" in text and "const int n = (int)min(256LL, n_ent - e0);" in text
    assert "__shared__ float4 s_ent[256];" in text and P.CHUNK == P.WORKGROUP == 256
    assert "const int p = (tile * a.nv + v) * 256 + tid;" in text
    assert "p->ntiles = (p->np + HS_TILE - 1) / HS_TILE;" in text
    assert "p->nv = ((p->np + p->ntiles - 1) / p->ntiles + 255) / 256;" in text
    assert "p->ntiles = (p->np + 256 * p->nv - 1) / (256 * p->nv);" in text
    assert "long long hi_a = (long long)floor(((double)a.z0 - zc - kk) * a.apix / rise) - 1;" in text
    assert "long long hi_b = (long long)ceil(((double)a.z1 - zc - kk) * a.apix / rise) + 1;" in text
    assert "const long long n_ent = hi_b >= hi_a ? (hi_b - hi_a + 1) * (long long)csym : 0;" in text
    assert "hs_stage(k, hi_a + e / csym, (int)(e % csym), csym, twist, rise, a, ent, kf, cs64)" in text
    assert f"constexpr float HS_EDGE_ULPS = {P.EDGE_ULPS:.0f}.f;" in text
    assert "constexpr int HS_MAX_CSYM = 4096;" in text and P.CSYM_MAX_CANDIDATE[2] == 4096


def test_layout_model_and_the_lists_order():
    assert P.reachable_layouts() == [(1, v) for v in range(1, 9)] + [(2, v) for v in range(5, 9)] + [(3, v) for v in range(6, 9)]
    for n in range(1, 6145):
        ntiles, nv = P.layout(n)
        assert 1 <= nv <= P.HS_VPT and (ntiles - 1) * 256 * nv < n <= ntiles * 256 * nv   # every tile holds a voxel
    assert P.layout(2116) == (2, 5) and P.layout(4225) == (3, 6) and P.layout(2048) == (1, 8) and P.layout(2049) == (2, 5)
    vox = P.voxel_list((4, 7, 9), 1.5, 3.2)
    assert np.array_equal(vox, np.array(sorted(map(tuple, vox))))   # row-major (j, i)
    assert P.slot(0, 5) == (0, 0, 0) and P.slot(255, 5) == (0, 0, 255) and P.slot(256, 5) == (0, 1, 0) and P.slot(1280, 5) == (1, 0, 0)
    for shape, reg in (((32, 24, 24), dict(rmin=3, rmax=11, z_fraction=0.5)), ((30, 21, 25), dict(rmin=0, rmax=None, z_fraction=0.3)),
                       ((7, 9, 8), dict(rmin=2.5, rmax=..., z_fraction=0.01))):
        assert np.array_equal(P.region_mask(shape, **reg), region_mask(shape, **reg))


def test_z_range_and_window_models():
    vol = P.zr_map(helix_map, add_noise)
    prof = vol.sum(axis=(1, 2), dtype=np.float64)
    nzi = np.where(prof > 0.01 * prof.max())[0]
    z0, z1 = int(nzi[0]), int(nzi[-1])
    assert (z0, z1) == (6, 18) and not vol[:6].any() and not vol[19:].any()
    zmid = (z0 + z1) // 2 + (z0 + z1) % 2
    for fraction, want in zip(P.ZR_FRACTIONS, ((6, 18), (9, 15))):
        half = int(24 * fraction + 0.5) // 2
        assert P.z_range(vol, fraction) == (max(z0, zmid - half), min(z1, zmid + half)) == want   # SymmetrySearch.z_range's definition
    # the window is never short of a repeat the reference admits
    rng = np.random.default_rng(0)
    for _ in range(400):
        nz = int(rng.integers(2, 40))
        rise = float(np.exp(rng.uniform(np.log(0.05), np.log(4 * nz * A))))
        a, b = sorted(rng.integers(0, nz, size=2))
        if a == b:
            continue
        for k in range(nz):
            hi, _, _, live = P.entries((nz, 4, 4), A, rise, 1, int(a), int(b), k)
            assert np.array_equal(hi[live], P.live_repeats((nz, 4, 4), A, rise, int(a), int(b), k))
    assert P.n_entries((32, 24, 24), 2.0, 0.2, 1, 0, 31, 16) == 313   # the issue's figure for the small test map
    assert P.n_entries((32, 24, 24), 2.0, 2.0, 12, 0, 31, 16) == 408 and P.n_entries((32, 24, 24), 2.0, 6.0, 64, 0, 31, 16) == 896


def test_sym_plane_is_the_oracles_operator():
    worst = 0.0
    for vol, cands, fraction in ((P.chunk_map(), ((29.0, 6.0, 1), (45.0, 4.0, 2), (29.0, 0.5, 1), (29.0, 20.0, 171)), 1.0),
                                 (P.noise_map((8, 21, 25), 3), ((-90.0, 3.0, 2), (30.0, 1.0, 1)), 1.0),
                                 (P.zr_map(helix_map, add_noise), ((29.0, 6.0, 1), (29.0, 16.0, 1)), 0.25)):
        for cand in cands:
            ref = oracle_sym(vol, cand, fraction)
            got = P.sym_planes(vol, A, cand, (0, vol.shape[0]), fraction)
            worst = max(worst, float(np.abs(got - ref).max() / np.abs(vol).max()))
    print(f"sym_plane against the oracle: largest difference {worst:.2e} of the map's largest value")
    assert worst < 3e-6   # float32 accumulation of up to 171 terms in the oracle


# ---- group 1 --------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def chunk_facts():
    vol = P.chunk_map()
    z = P.z_range(vol)
    planes = P.scored_planes(P.CHUNK_SHAPE, P.CHUNK_REGION["z_fraction"])
    return vol, z, planes, P.region_mask(P.CHUNK_SHAPE, **P.CHUNK_REGION)


def test_chunk_lists_reach_every_count_and_a_lost_chunk_shows():
    vol, z, planes, mask = chunk_facts()
    assert z == (0, 15) and planes == (7, 9)
    for rise in np.exp(np.linspace(np.log(0.01), np.log(200.0), 2000)):   # these planes' windows hold at least three repeats
        assert all(P.n_entries(P.CHUNK_SHAPE, A, float(rise), 1, *z, k) >= 3 for k in range(*planes))
    reached = {1: set(), 2: set()}
    for tw, rs, cs, n in P.CHUNK_CANDIDATES:
        ns = {P.n_entries(P.CHUNK_SHAPE, A, rs, cs, *z, k) for k in range(*planes)}
        assert ns == {n}, (tw, rs, cs, ns)
        reached[1 if cs == 1 else 2].add(n)
        lost = sum(int(P.entries(P.CHUNK_SHAPE, A, rs, cs, *z, k)[3][P.CHUNK:].sum()) for k in range(*planes))
        full = P.sym_planes(vol, A, (tw, rs, cs), planes)
        conditions(vol[planes[0]:planes[1]], full, mask[planes[0]:planes[1]], (tw, rs, cs))
        if n <= P.CHUNK:
            assert lost == 0
            continue
        cut = P.sym_planes(vol, A, (tw, rs, cs), planes, first_entries=P.CHUNK)
        move = abs(P.pearson(vol, full, mask) - P.pearson(vol, cut, mask))
        print(f"chunks: ({tw}, {rs}, {cs}) n_ent {n}: {lost} live entries past the first chunk, losing them moves the score by {move:.2e}")
        if (cs, n) == (1, 257):
            assert lost == 0 and move == 0   # entry 256 is the window's widening: the second pass runs and must add nothing
        else:
            assert lost > 0 and move >= P.SENSITIVITY
    for name, want in P.CHUNK_WANTED.items():
        for kind in (1, 2):
            if (name, kind) == ("at_257", 2):
                continue   # 257 is prime: csym 257 with a window of one repeat, and these planes' windows hold at least three
            assert any(want(n) for n in reached[kind]), (name, kind)
    t0 = time.perf_counter()
    vol = P.noise_map(P.CSYM_MAX_SHAPE, 102)
    sym = oracle_sym(vol, P.CSYM_MAX_CANDIDATE)
    dt = time.perf_counter() - t0
    m = P.region_mask(P.CSYM_MAX_SHAPE, **P.CSYM_MAX_REGION)
    conditions(vol, sym, m, "csym 4096")
    zz = P.z_range(vol)
    ns = {P.n_entries(P.CSYM_MAX_SHAPE, A, P.CSYM_MAX_CANDIDATE[1], 4096, *zz, k) for k in range(4)}
    cut = P.sym_planes(vol, A, P.CSYM_MAX_CANDIDATE, (0, 4), first_entries=P.CHUNK)
    move = abs(score(vol, sym, m) - P.pearson(vol, cut, m))
    print(f"chunks: csym 4096 on {P.CSYM_MAX_SHAPE}: n_ent {sorted(ns)}, oracle {dt:.2f} s, first chunk alone moves the score by {move:.2e}")
    assert min(ns) >= 3 * 4096 and move >= P.SENSITIVITY   # the oracle's time is printed, not asserted: it is the host's


# ---- group 2 --------------------------------------------------------------------------------------------------------------
def test_tile_regions_cover_every_layout_and_seam():
    seen = {}
    for row in P.TILE_REGIONS:
        ny, nx, rmin, rmax, n = row
        vox = P.voxel_list((P.TILE_NZ, ny, nx), rmin, rmax)
        assert len(vox) == n, row
        seen.setdefault(P.layout(n), []).append(n)
    assert sorted(seen) == P.reachable_layouts()
    nps = {row[4] for row in P.TILE_REGIONS}
    for m in (256, 2048, 2560, 4096, 4608):   # 256 nv with (ntiles, nv) = (1, 1), (1, 8), (2, 5), (2, 8), (3, 6)
        assert {m - 1, m, m + 1} <= nps
        assert m % (256 * P.layout(m)[1]) == 0 and P.layout(m + 1) != P.layout(m)
    assert 2116 in nps   # the full 46 x 46 plane, whose list starts and ends on the plane's corners
    print("tiles: layouts", {k: v for k, v in sorted(seen.items())})


@pytest.mark.parametrize("row", P.TILE_REGIONS, ids=lambda r: f"{r[0]}x{r[1]}-np{r[4]}")
def test_a_lost_voxel_under_a_spike_shows(row):
    vol, region = P.tile_case(row)
    shape = vol.shape
    mask = P.region_mask(shape, **region)
    k0, k1 = P.scored_planes(shape, region["z_fraction"])
    vox = P.voxel_list(shape, region["rmin"], region["rmax"])
    ntiles, nv = P.layout(len(vox))
    spikes = P.spike_positions(len(vox))
    assert {0, len(vox) - 1} <= set(spikes) and (len(vox) <= 256 or {255, 256} <= set(spikes))
    assert {t * 256 * nv for t in range(ntiles)} <= set(spikes) and {t * 256 * nv - 1 for t in range(1, ntiles)} <= set(spikes)
    syms = [oracle_sym(vol, c) for c in P.TILE_CANDIDATES]
    for s in syms:
        conditions(vol, s, mask, row)
    # position p of the list in plane k is entry (k - k0) * np + p of vol[mask] (mask is row-major per plane)
    moves = np.max([P.lost_voxel_moves(vol, s, mask) for s in syms], axis=0).reshape(k1 - k0, len(vox))
    worst = {p: float(moves[:, p].min()) for p in spikes}
    print(f"tiles: {row} layout {(ntiles, nv)}: spikes at {spikes}, a lost spiked voxel moves the best candidate's score by "
          f"{min(worst.values()):.2e} ... {max(worst.values()):.2e}")
    assert min(worst.values()) >= P.SENSITIVITY, worst


# ---- group 3 --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", P.RING_SHAPES, ids=str)
def test_rings_cover_the_plane_and_every_voxel_shows(shape):
    vol = P.noise_map(shape, 7)
    syms = [oracle_sym(vol, c) for c in P.RING_CANDIDATES]
    rings = P.rings(shape)
    cover = np.zeros(shape[1:], dtype=int)
    merged = [r for r in rings if r[1] - r[0] > 1]
    assert len(merged) * 10 <= len(rings) + len(merged)
    print(f"rings {shape}: {len(rings)} rings, merged {merged}")
    for rmin, rmax in rings:
        mask = P.region_mask(shape, rmin, rmax, P.RING_Z_FRACTION)
        vox = P.voxel_list(shape, rmin, rmax)
        cover[vox[:, 0], vox[:, 1]] += 1
        for s in syms:
            conditions(vol, s, mask, (shape, rmin))
        lost = np.max([P.lost_voxel_moves(vol, s, mask) for s in syms], axis=0)
        dark = np.all([s[mask] == 0 for s in syms], axis=0)   # no candidate reaches the voxel: S = 0, nothing to lose
        admitted = np.max([P.lost_voxel_moves(vol, s, mask, admitted=True) for s in syms], axis=0)
        move = np.where(dark, admitted, lost)
        print(f"rings {shape}: {rmin} <= r < {rmax}: {int(mask.sum())} voxels ({int(dark.sum())} unreached), least sensitive voxel moves a score by {move.min():.2e}")
        assert move.min() >= P.SENSITIVITY
    assert (cover == 1).all()   # every in-plane voxel, once


def test_lost_voxel_moves_is_the_recomputed_score():
    shape = (8, 21, 25)
    vol = P.noise_map(shape, 7)
    sym = oracle_sym(vol, P.RING_CANDIDATES[0])
    mask = P.region_mask(shape, 5, 6, P.RING_Z_FRACTION)
    fast = P.lost_voxel_moves(vol, sym, mask)
    idx = np.argwhere(mask)
    for t in (0, 7, len(idx) - 1):
        s2 = sym.copy()
        s2[tuple(idx[t])] = 0
        assert abs(abs(score(vol, s2, mask) - score(vol, sym, mask)) - fast[t]) < 2e-6   # the oracle's coefficient is float32


# ---- group 4 --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", P.BORDER_CASES, ids=lambda c: "x".join(map(str, c[0])))
def test_border_candidates_flip_and_the_float32_verdict_shows(case):
    shape, seed, cands = case
    vol = P.border_map(shape, seed)
    z = P.z_range(vol)
    assert z == (0, shape[0] - 1)
    masks = {name: P.region_mask(shape, **reg) for name, reg in P.border_regions(shape).items()}
    parities = {(c[1] % 2, c[2] % 2) for c, _, _ in P.BORDER_CASES}
    assert {(0, 0), (1, 1), (1, 0)} <= parities and any(max(c[0]) == 1024 for c in P.BORDER_CASES)
    for cand in cands:
        flips = [P.border_flips(shape, A, *cand, k, *z) for k in range(shape[0])]
        assert sum(flips) > 0, (shape, cand)
        right = P.sym_planes(vol, A, cand, (0, shape[0]))
        wrong = P.sym_planes(vol, A, cand, (0, shape[0]), verdict="float32")
        moves = {}
        for name, m in masks.items():
            conditions(vol, right, m, (shape, cand, name))
            moves[name] = abs(P.pearson(vol, right, m) - P.pearson(vol, wrong, m))
        print(f"borders {shape} {cand}: flipped samples per plane {flips}; the float32 verdict moves the score by "
              + ", ".join(f"{k} {v:.2e}" for k, v in moves.items()))
        assert min(moves.values()) >= P.SENSITIVITY, (shape, cand, moves)   # the frame and the full plane each
    # the quarter turn is reached through the twist, through 360 / csym and through a multiple of a 30 degree twist
    assert {(90.0, 1), (29.0, 4), (30.0, 1)} <= {(c[0], c[2]) for c in cands} or max(shape) == 1024
    assert all((-c[0], c[1], c[2]) in cands for c in cands)


# ---- group 5 --------------------------------------------------------------------------------------------------------------
def test_side_shapes_cover_parities_and_orders():
    assert {tuple(v % 2 for v in s) for s in P.SIDE_SHAPES} == {(a, b, c) for a in (0, 1) for b in (0, 1) for c in (0, 1)}
    assert {tuple(np.argsort(s)) for s in P.SIDE_SHAPES} == {(0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0)}
    for shape in P.SMALLEST_DEFAULT:
        assert min(shape[1:]) // 2 - 1 == 1 and int(P.region_mask(shape).sum()) == 8
        smaller = (shape[0], min(3, shape[1]), min(3, shape[2]))
        assert min(smaller[1:]) // 2 - 1 == 0    # one voxel less on the short side: no default region
    for shape in P.SMALLEST_ANY:
        assert min(shape) == 2 and int(P.region_mask(shape, 0, None, 1.0).sum()) >= P.MIN_VOXELS


@pytest.mark.parametrize("shape", P.SIDE_SHAPES + P.SMALLEST_DEFAULT + P.SMALLEST_ANY, ids=str)
def test_side_probes_hold_the_conditions_and_the_column_centre_shows(shape):
    vol = P.noise_map(shape, 300 + sum(shape))
    small = shape in P.SMALLEST_ANY
    regions = (dict(rmin=0, rmax=None, z_fraction=1.0),) if small else P.SIDE_REGIONS
    cands = P.SMALLEST_CANDIDATES if small else P.SMALLEST_DEFAULT_CANDIDATES if shape in P.SMALLEST_DEFAULT else P.SIDE_CANDIDATES
    for reg in regions:
        mask = P.region_mask(shape, **reg)
        best = 0.0
        for cand in cands:
            right = P.sym_planes(vol, A, cand, (0, shape[0]))
            conditions(vol, right, mask, (shape, reg, cand))
            if shape[2] % 2:
                wrong = P.sym_planes(vol, A, cand, (0, shape[0]), col_centre=shape[2] // 2)
                best = max(best, abs(P.pearson(vol, right, mask) - P.pearson(vol, wrong, mask)))
        if shape[2] % 2:
            print(f"sides {shape} {reg}: columns centred on nx // 2 move a score by {best:.2e}")
            assert best >= P.SENSITIVITY


@pytest.mark.parametrize("fraction", P.ZR_FRACTIONS)
def test_z_range_probes(fraction):
    vol = P.zr_map(helix_map, add_noise)
    z = P.z_range(vol, fraction)
    cand_e, empty = P.ZR_EMPTY[fraction]
    assert cand_e in P.ZR_CANDIDATES[fraction]
    slabs = [P.scored_planes(P.ZR_SHAPE, zf) for zf in P.ZR_Z_FRACTIONS]
    assert slabs == [(9, 15), (6, 18), (3, 21), (0, 24)]   # thinner than, equal to and wider than [6, 18)
    for cand in P.ZR_CANDIDATES[fraction]:
        sym = oracle_sym(vol, cand, fraction)
        ignored = P.sym_planes(vol, A, cand, (0, 24), z=(0, 23))
        if cand == cand_e:
            for k in empty:
                assert not sym[k].any() and len(P.live_repeats(P.ZR_SHAPE, A, cand[1], *z, k)) == 0
            filled = sym.copy()
            for k in empty:
                filled[k] = vol[k]
        for zf in P.ZR_Z_FRACTIONS:
            mask = P.region_mask(P.ZR_SHAPE, 0, None, zf)
            conditions(vol, sym, mask, (fraction, cand, zf))
            move_e = abs(score(vol, sym, mask) - score(vol, ignored, mask))
            line = f"z range {z} {cand} z_fraction {zf}: the whole map as source moves the score by {move_e:.2e}"
            if cand == cand_e and mask[list(empty)].any():
                move_d = abs(score(vol, sym, mask) - score(vol, filled, mask))
                line += f"; the empty planes {empty} filled with the map by {move_d:.2e}"
                assert move_d >= P.SENSITIVITY
            print(line)
            if cand != cand_e:
                assert move_e >= P.SENSITIVITY


# ---- group 6 --------------------------------------------------------------------------------------------------------------
def test_candidate_values():
    vol = P.value_map(helix_map, add_noise)
    mask = P.region_mask(P.VALUE_SHAPE, **P.VALUE_REGION)
    assert mask.all()
    tw = [c[0] for c in P.VALUE_CANDIDATES]
    assert min(tw) < 0 and {180.0, 181.0, 389.0} <= set(tw)
    L = P.VALUE_SHAPE[0] * A
    assert any(c[1] == L for c in P.VALUE_CANDIDATES) and any(c[1] > L for c in P.VALUE_CANDIDATES)
    assert any(c[1] % A == 0 and c[1] < L for c in P.VALUE_CANDIDATES) and any(360 % c[2] for c in P.VALUE_CANDIDATES)
    ref = oracle_scores(vol, A, P.VALUE_CANDIDATES, mask)
    for c, r in zip(P.VALUE_CANDIDATES, ref):
        conditions(vol, oracle_sym(vol, c), mask, c)
        print(f"values: {c} oracle score {r:.5f}")
    by = dict(zip(P.VALUE_CANDIDATES, ref))
    # the sign and the period of the twist are visible: a kernel that drops either moves these scores by more than 1e-3
    assert abs(by[(29.0, 6.0, 1)] - by[(-29.0, 6.0, 1)]) >= P.SENSITIVITY
    assert abs(by[(181.0, 6.0, 1)] - by[(180.0, 6.0, 1)]) >= P.SENSITIVITY
    assert abs(by[(389.0, 6.0, 1)] - by[(29.0, 6.0, 1)]) < TOL and abs(by[(-331.0, 6.0, 1)] - by[(29.0, 6.0, 1)]) < TOL
    assert abs(by[(29.0, 6.0, 7)] - by[(29.0, 6.0, 1)]) >= P.SENSITIVITY
