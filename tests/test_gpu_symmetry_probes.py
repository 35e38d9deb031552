"""The symmetry search on the device (helicon_amd/csrc/symmetry_search.inc) at its seams: repeat lists that cross the
256-entry chunks, every tile layout and the list positions on each side of a tile, lane and slot seam, every one-voxel
ring of two planes, the border verdicts, map sides and z ranges, and the candidate values at the edges of their ranges.

The cases, the model of the kernel's decomposition and the probe maps are tests/symmetry_probes.py's;
tests/test_symmetry_probes_host.py shows on the CPU that each probe would notice the defect it guards against (the
oracle's own score moves by at least 1e-3 under it).  Here every score is compared with

    S = oracle.symmetrize.apply_helical_symmetry(V, apix, twist, rise, csym, fraction, V.shape, apix)
    score = oracle.path_b.cross_correlation_coefficient(V[M], S[M])

on the test's own statement of M, at tests/test_gpu_symmetry_search.py's TOL = 2e-4; every test prints its largest
difference before it asserts.
"""
import numpy as np
import pytest

import symmetry_probes as P
from helicon_amd.symmetry_search import SymmetrySearch
from oracle import path_b as O
from oracle import symmetrize as S
from test_gpu_symmetry_search import TOL, add_noise, helix_map, oracle_scores, region_mask

pytestmark = pytest.mark.gpu

A = P.APIX


def params_of(cands):
    return np.array([(c[0], c[1], c[2]) for c in cands], dtype=np.float64)


def compare(name, vol, cands, regions, fraction=1.0):
    """Device scores of `cands` on every region of `regions` (a dict; the value {} is the handle's default region, left as
    the constructor set it) against the oracle composition, the symmetrised maps computed once.  Returns the largest
    difference after printing it."""
    params = params_of(cands)
    syms = [S.apply_helical_symmetry(vol, A, float(tw), float(rs), int(cs), fraction, vol.shape, A) for tw, rs, cs in params]
    worst, where = 0.0, None
    with SymmetrySearch(vol, A, fraction=fraction) as ss:
        for rname, reg in regions.items():
            if reg:
                ss.set_region(**reg)
            mask = region_mask(vol.shape, **reg)
            assert ss.region_voxels == int(mask.sum())
            got = ss.search(params)
            ref = np.array([float(O.cross_correlation_coefficient(vol[mask], s[mask])) for s in syms])
            err = np.abs(got - ref)
            if err.max() >= worst:
                worst, where = float(err.max()), (rname, tuple(float(v) for v in params[int(np.argmax(err))]))
    print(f"symmetry probes [{name}]: max |score - oracle| = {worst:.3e} over {len(regions)} region(s) x {len(params)} candidates, at {where}")
    return worst


# ---- 1. repeat chunks -----------------------------------------------------------------------------------------------------
def test_repeat_chunks_against_the_oracle_and_bit_for_bit():
    vol = P.chunk_map()
    mask = region_mask(P.CHUNK_SHAPE, **P.CHUNK_REGION)
    long_ = params_of(P.CHUNK_CANDIDATES)
    plain = params_of(P.ORDINARY)
    mixed = np.concatenate([plain[:1], long_[:8], plain[1:2], long_[8:], plain[2:]])
    with SymmetrySearch(vol, A) as ss:
        ss.set_region(**P.CHUNK_REGION)
        assert ss.z_range == (0, 15)
        got = ss.search(mixed)
        assert np.array_equal(ss.search(mixed), got)
        assert np.array_equal(ss.search(mixed[::-1].copy())[::-1], got)
        alone = np.array([ss.search(row[None, :])[0] for row in mixed])
    with SymmetrySearch(vol, A, partial_bytes=1) as cut:
        cut.set_region(**P.CHUNK_REGION)
        one_per_launch = cut.search(mixed)
        assert cut.launches == len(mixed)
    ref = oracle_scores(vol, A, mixed, mask)
    err = np.abs(got - ref)
    print(f"symmetry probes [chunks, n_ent {sorted({c[3] for c in P.CHUNK_CANDIDATES})}]: max |score - oracle| = {err.max():.3e} "
          f"at {tuple(float(v) for v in mixed[int(np.argmax(err))])}")
    assert np.array_equal(alone, got) and np.array_equal(one_per_launch, got)
    assert err.max() < TOL


def test_csym_4096():
    vol = P.noise_map(P.CSYM_MAX_SHAPE, 102)
    cands = (P.CSYM_MAX_CANDIDATE,) + P.ORDINARY[:1]
    assert compare("csym 4096 on 4 x 8 x 8", vol, cands, {"whole": P.CSYM_MAX_REGION}) < TOL
    with SymmetrySearch(vol, A) as ss:
        ss.set_region(**P.CSYM_MAX_REGION)
        both = ss.search(params_of(cands))
        assert ss.search(params_of(cands[:1]))[0] == both[0] and ss.search(params_of(cands[::-1]))[1] == both[0]


# ---- 2. tile layouts and seams --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", P.TILE_REGIONS, ids=lambda r: f"{r[0]}x{r[1]}-np{r[4]}")
def test_tile_layouts_and_seams(row):
    vol, region = P.tile_case(row)
    layout = P.layout(row[4])
    assert compare(f"tiles {row[0]} x {row[1]}, np {row[4]}, layout {layout}", vol, P.TILE_CANDIDATES, {"region": region}) < TOL


# ---- 3. ring census -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", P.RING_SHAPES, ids=str)
def test_every_ring(shape):
    vol = P.noise_map(shape, 7)
    regions = {f"{a} <= r < {b}": dict(rmin=a, rmax=b, z_fraction=P.RING_Z_FRACTION) for a, b in P.rings(shape)}
    merged = [r for r in P.rings(shape) if r[1] - r[0] > 1]
    print(f"symmetry probes [rings {shape}]: {len(regions)} rings, merged {merged}")
    assert compare(f"rings {shape}", vol, P.RING_CANDIDATES, regions) < TOL


# ---- 4. borders -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", P.BORDER_CASES, ids=lambda c: "x".join(map(str, c[0])))
def test_border_verdicts(case):
    shape, seed, cands = case
    vol = P.border_map(shape, seed)
    assert compare(f"borders {shape}", vol, cands, P.border_regions(shape)) < TOL


# ---- 5. map sides and the z range -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", P.SIDE_SHAPES + P.SMALLEST_DEFAULT + P.SMALLEST_ANY, ids=str)
def test_map_sides(shape):
    vol = P.noise_map(shape, 300 + sum(shape))
    whole = dict(rmin=0, rmax=None, z_fraction=1.0)
    if shape in P.SMALLEST_ANY:
        regions, cands = {"whole": whole}, P.SMALLEST_CANDIDATES
    elif shape in P.SMALLEST_DEFAULT:
        regions, cands = {"default": {}, "whole": whole}, P.SMALLEST_DEFAULT_CANDIDATES
    else:
        regions, cands = {"default": {}, "whole": whole}, P.SIDE_CANDIDATES
    assert compare(f"sides {shape}", vol, cands, regions) < TOL


@pytest.mark.parametrize("fraction", P.ZR_FRACTIONS)
def test_z_range_and_empty_planes(fraction):
    vol = P.zr_map(helix_map, add_noise)
    with SymmetrySearch(vol, A, fraction=fraction) as ss:
        assert ss.z_range == P.z_range(vol, fraction) == {1.0: (6, 18), 0.25: (9, 15)}[fraction]
    regions = {f"z_fraction {zf}": dict(rmin=0, rmax=None, z_fraction=zf) for zf in P.ZR_Z_FRACTIONS}
    regions["shell, z_fraction 1"] = dict(rmin=2, rmax=7, z_fraction=1.0)
    assert compare(f"z range, fraction {fraction}", vol, P.ZR_CANDIDATES[fraction], regions, fraction) < TOL


# ---- 6. candidate values --------------------------------------------------------------------------------------------------
def test_candidate_values():
    vol = P.value_map(helix_map, add_noise)
    assert compare("candidate values", vol, P.VALUE_CANDIDATES, {"whole": P.VALUE_REGION}) < TOL
