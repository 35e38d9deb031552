"""The symmetry search (helicon_amd/csrc/symmetry_search.inc) seam by seam: a Python model of how k_hs_score cuts its work —
the in-plane voxel list and its tiles, the window of repeats of a plane and its 256-entry chunks, the source z range, the
float32 bounds verdict beside the reference's float64 one — and the probe maps, regions and candidate lists that
tests/test_gpu_symmetry_probes.py scores on the device and tests/test_symmetry_probes_host.py justifies on the CPU.

No GPU dependency and no import of the package under test: NumPy and the oracle only.

Why: the device scores are held to 2e-4 on a Pearson coefficient, and a coefficient over thousands of voxels does not
move by 2e-4 when one voxel, one repeat or one border row is lost.  Each probe here is a (map, region, candidate list)
on which the guarded seam carries a visible share of the score; the host test shows that share on the CPU oracle first
(a perturbation of the oracle's symmetrised map that imitates the defect must move the oracle's score by SENSITIVITY =
1e-3, five times TOL).  The perturbations:

    (a) lost voxel      S at one voxel of the region set to 0
    (b) lost chunk      S of a plane from the first 256 entries of the kernel's (hi, ci) list alone
    (c) float32 border  S with the bounds verdict of the float32 positions instead of the float64 one
    (d) no empty plane  S on a plane that no repeat reaches (S = 0 there) replaced by the map itself
    (e) z range         S with the source range [0, nz - 1) instead of the 1 % profile rule's     (group 5)
    (f) column centre   S with the columns centred on nx // 2 instead of nx / 2                    (group 5, odd nx)

``sym_plane`` is the reference's operator for ONE output plane in float64 (the oracle accumulates in float32; the host
test pins the two to each other), with one switch per perturbation.
"""
from __future__ import annotations

import re
from pathlib import Path

import numpy as np

CSRC = Path(__file__).resolve().parent.parent / "helicon_amd" / "csrc"

HS_VPT = 8        # voxels per lane, at most
WORKGROUP = 256   # lanes of a workgroup: a tile is WORKGROUP * nv consecutive list entries
CHUNK = 256       # (hi, ci) entries staged through LDS per pass
EDGE_ULPS = 8.0

TOL = 2e-4           # tests/test_gpu_symmetry_search.py's
SENSITIVITY = 1e-3   # five times TOL, the margin of well_separated
MIN_VOXELS = 8
MIN_VARIANCE = 1e-6  # of the raw second moment; the kernel's "no variance" rule is 1e-12


def source(name="symmetry_search.inc"):
    """The file with comments dropped and white space collapsed."""
    text = re.sub(r"//[^\n]*", "", (CSRC / name).read_text())
    return re.sub(r"\s+", " ", text)


# ---- the model ----------------------------------------------------------------------------------------------------------
def voxel_list(shape, rmin=0, rmax=...):
    """The in-plane voxels of the region in list order, row-major (j, i): an [np, 2] integer array (hs_set_region)."""
    _, ny, nx = shape
    if rmax is ...:
        rmax = min(ny, nx) // 2 - 1
    j, i = np.meshgrid(np.arange(ny), np.arange(nx), indexing="ij")
    r2 = ((j - ny // 2) ** 2 + (i - nx // 2) ** 2).astype(np.float64)
    m = r2 >= float(rmin) * float(rmin)
    if rmax is not None:
        m &= r2 < float(rmax) * float(rmax)
    return np.stack([j[m], i[m]], axis=1)


def layout(np_):
    """(ntiles, nv) of a region with np_ in-plane voxels: the fewest tiles of at most 256 HS_VPT, then equal shares."""
    tile = WORKGROUP * HS_VPT
    ntiles = (np_ + tile - 1) // tile
    nv = ((np_ + ntiles - 1) // ntiles + WORKGROUP - 1) // WORKGROUP
    ntiles = (np_ + WORKGROUP * nv - 1) // (WORKGROUP * nv)
    return ntiles, nv


def slot(p, nv):
    """(tile, v, lane) of list position p: p = (tile * nv + v) * 256 + lane."""
    return p // (WORKGROUP * nv), (p // WORKGROUP) % nv, p % WORKGROUP


def scored_planes(shape, z_fraction):
    nz = shape[0]
    if z_fraction >= 1:
        return 0, nz
    h = max(1, int(nz * z_fraction + 0.5) // 2)
    return max(0, nz // 2 - h), min(nz, nz // 2 + h)


def region_mask(shape, rmin=0, rmax=..., z_fraction=0.5):
    nz, ny, nx = shape
    m = np.zeros(shape, dtype=bool)
    vox = voxel_list(shape, rmin, rmax)
    k0, k1 = scored_planes(shape, z_fraction)
    m[k0:k1, vox[:, 0], vox[:, 1]] = True
    return m


def z_range(vol, fraction=1.0):
    """[z0, z1): the source planes the operator reads (transforms.py:92-99)."""
    nz = vol.shape[0]
    prof = vol.sum(axis=(1, 2), dtype=np.float64)
    idx = np.where(prof > 0.01 * prof.max())[0]
    z0, z1 = int(idx[0]), int(idx[-1])
    zmid = (z0 + z1) // 2 + (z0 + z1) % 2
    half = int(nz * fraction + 0.5) // 2
    return max(z0, zmid - half), min(z1, zmid + half)


def hsym_max(shape, apix, rise):
    return max(1, int(shape[0] * apix / rise))


def hi_window(shape, apix, rise, z0, z1, k):
    """[hi_a, hi_b]: the repeats k_hs_score visits for plane k (widened by one on each side, clamped to +-hsym_max)."""
    nz = shape[0]
    kk, zc = float(k - nz // 2), float(nz // 2)
    hmax = hsym_max(shape, apix, rise)
    hi_a = int(np.floor((float(z0) - zc - kk) * apix / rise)) - 1
    hi_b = int(np.ceil((float(z1) - zc - kk) * apix / rise)) + 1
    return max(hi_a, -hmax), min(hi_b, hmax)


def n_entries(shape, apix, rise, csym, z0, z1, k):
    hi_a, hi_b = hi_window(shape, apix, rise, z0, z1, k)
    return (hi_b - hi_a + 1) * int(csym) if hi_b >= hi_a else 0


def entries(shape, apix, rise, csym, z0, z1, k):
    """The kernel's list for plane k in its order: arrays (hi, ci, k2, live), entry e = (hi - hi_a) * csym + ci."""
    nz = shape[0]
    hi_a, hi_b = hi_window(shape, apix, rise, z0, z1, k)
    hi = np.repeat(np.arange(hi_a, hi_b + 1, dtype=np.int64), int(csym))
    ci = np.tile(np.arange(int(csym), dtype=np.int64), max(0, hi_b - hi_a + 1))
    k2 = ((k - nz // 2) * apix + hi * rise) / apix + nz // 2
    return hi, ci, k2, (k2 >= z0) & (k2 < z1)


def live_repeats(shape, apix, rise, z0, z1, k):
    """The repeats the REFERENCE admits for plane k (its full loop -hsym_max ... hsym_max): what the window must hold."""
    nz = shape[0]
    hmax = hsym_max(shape, apix, rise)
    hi = np.arange(-hmax, hmax + 1, dtype=np.int64)
    k2 = ((k - nz // 2) * apix + hi * rise) / apix + nz // 2
    return hi[(k2 >= z0) & (k2 < z1)]


def _positions(shape, apix, twist, csym, hi, ci, col_centre=None):
    """The reference's float64 sample positions (j2, i2) of every voxel of a plane under one (hi, ci), and cos, sin."""
    _, ny, nx = shape
    jj = (np.arange(ny) - ny // 2).astype(np.float64)[:, None]
    ii = (np.arange(nx) - (nx / 2 if col_centre is None else col_centre))[None, :]
    rot = np.deg2rad(twist * int(hi) + 360 * int(ci) / int(csym))
    c, s = np.cos(rot), np.sin(rot)
    j2 = (c * jj + s * ii) * apix / apix + ny // 2
    i2 = (-s * jj + c * ii) * apix / apix + nx // 2
    return j2, i2, c, s


def _verdict32(shape, c, s):
    """The kernel's bounds test on float32 positions relative to the axis (without hs_border)."""
    _, ny, nx = shape
    jj = (np.arange(ny) - ny // 2).astype(np.float32)[:, None]
    ii = (np.arange(nx).astype(np.float32) - np.float32(nx) * np.float32(0.5))[None, :]
    c32, s32 = np.float32(c), np.float32(s)
    fj = np.floor(c32 * jj + s32 * ii)
    fi = np.floor(c32 * ii - s32 * jj)
    return (fj >= -(ny // 2)) & (fj <= ny - 2 - ny // 2) & (fi >= -(nx // 2)) & (fi <= nx - 2 - nx // 2)


def _verdict64(shape, j2, i2):
    _, ny, nx = shape
    jf, i_f = np.floor(j2), np.floor(i2)
    return (jf >= 0) & (jf < ny - 1) & (i_f >= 0) & (i_f < nx - 1)


def sym_plane(vol, apix, twist, rise, csym, k, z0, z1, *, first_entries=None, verdict="float64", col_centre=None):
    """Plane k of apply_helical_symmetry(vol, apix, twist, rise, csym, new_size = vol.shape) in float64, from the kernel's
    entry list.  ``first_entries``: only entries e < first_entries count (perturbation b).  ``verdict="float32"``: the
    bounds test of the float32 positions, the float64 positions clamped into the plane (perturbation c).
    ``col_centre``: the centre the columns are taken about (perturbation f).  Returns (S, count)."""
    shape = vol.shape
    _, ny, nx = shape
    acc, cnt = np.zeros((ny, nx)), np.zeros((ny, nx))
    hi, ci, k2, live = entries(shape, apix, rise, csym, z0, z1, k)
    for e in np.where(live)[0]:
        if first_entries is not None and e >= first_entries:
            break
        kf, kc = int(np.floor(k2[e])), int(np.ceil(k2[e]))
        wk = k2[e] - kf
        j2, i2, c, s = _positions(shape, apix, twist, csym, hi[e], ci[e], col_centre)
        if verdict == "float32":
            ok = _verdict32(shape, c, s)
        else:
            ok = _verdict64(shape, j2, i2)
        if not ok.any():
            continue
        jf = np.clip(np.floor(j2[ok]), 0, ny - 2).astype(np.int64)
        i_f = np.clip(np.floor(i2[ok]), 0, nx - 2).astype(np.int64)
        wj, wi = np.clip(j2[ok] - jf, 0.0, 1.0), np.clip(i2[ok] - i_f, 0.0, 1.0)
        d0, d1 = vol[kf].astype(np.float64), vol[kc].astype(np.float64)
        a = (1 - wj) * ((1 - wi) * d0[jf, i_f] + wi * d0[jf, i_f + 1]) + wj * ((1 - wi) * d0[jf + 1, i_f] + wi * d0[jf + 1, i_f + 1])
        b = (1 - wj) * ((1 - wi) * d1[jf, i_f] + wi * d1[jf, i_f + 1]) + wj * ((1 - wi) * d1[jf + 1, i_f] + wi * d1[jf + 1, i_f + 1])
        acc[ok] += (1 - wk) * a + wk * b
        cnt[ok] += 1
    return np.where(cnt > 0, acc / np.where(cnt > 0, cnt, 1), 0.0), cnt


def sym_planes(vol, apix, cand, planes, fraction=1.0, z=None, **kw):
    """sym_plane for the planes [k0, k1) of a candidate (twist, rise, csym): float32 [k1 - k0, ny, nx]."""
    z0, z1 = z_range(vol, fraction) if z is None else z
    tw, rs, cs = cand
    return np.stack([sym_plane(vol, apix, float(tw), float(rs), int(cs), k, z0, z1, **kw)[0] for k in range(*planes)]).astype(np.float32)


def border_flips(vol_shape, apix, twist, rise, csym, k, z0=0, z1=None):
    """How many samples (voxel x live entry) of plane k the float32 bounds verdict decides otherwise than the reference's
    float64 one.  A candidate with none never reaches hs_border's reason for being."""
    if z1 is None:
        z1 = vol_shape[0] - 1
    hi, ci, _, live = entries(vol_shape, apix, rise, csym, z0, z1, k)
    n = 0
    for e in np.where(live)[0]:
        j2, i2, c, s = _positions(vol_shape, apix, twist, csym, hi[e], ci[e])
        n += int((_verdict32(vol_shape, c, s) != _verdict64(vol_shape, j2, i2)).sum())
    return n


def pearson(vol, sym, mask):
    """oracle.path_b.cross_correlation_coefficient(vol[mask], sym[mask]) for a symmetrised map given on the scored planes
    only (sym: [k1 - k0, ny, nx] with the planes of mask) or on the whole volume."""
    from oracle import path_b as O

    if sym.shape != vol.shape:
        ks = np.where(mask.any(axis=(1, 2)))[0]
        full = np.zeros(vol.shape, dtype=np.float32)
        full[ks[0]:ks[0] + sym.shape[0]] = sym
        sym = full
    return float(O.cross_correlation_coefficient(vol[mask], sym[mask]))


def variance_share(x):
    """Variance over raw second moment of a region's values."""
    x = np.asarray(x, dtype=np.float64)
    return float(x.var() / max(np.mean(x * x), 1e-300))


# ---- maps ---------------------------------------------------------------------------------------------------------------
def noise_map(shape, seed, mean=3.0):
    return (mean + np.random.default_rng(seed).normal(size=shape)).astype(np.float32)


def spike_positions(np_, last=True):
    """List positions a lost lane, slot or tile would hide: the first and last entry of every tile, the lane seam 255 / 256,
    and (``last``) the list's last entry."""
    ntiles, nv = layout(np_)
    tile = WORKGROUP * nv
    pos = {0, 255, 256}
    for t in range(ntiles):
        pos |= {t * tile, min((t + 1) * tile, np_) - 1}
    if not last:
        pos.discard(np_ - 1)
    return sorted(p for p in pos if p < np_)


def spike_map(shape, seed, region, height=50.0):
    """Unit white noise with `height` added at spike_positions of the region's list, in every scored plane."""
    vol = np.random.default_rng(seed).normal(size=shape).astype(np.float32)
    vox = voxel_list(shape, region.get("rmin", 0), region.get("rmax", ...))
    k0, k1 = scored_planes(shape, region.get("z_fraction", 0.5))
    for p in spike_positions(len(vox)):
        vol[k0:k1, vox[p, 0], vox[p, 1]] += np.float32(height)
    return vol


def spike_map_mean3(shape, seed, region, height=50.0):
    """spike_map on noise of mean 3: S is about 3 wherever a repeat contributes, so a lost voxel under a spike of the map
    moves the covariance by about 3 x height whatever the noise there happens to be."""
    return (spike_map(shape, seed, region, height) + np.float32(3.0)).astype(np.float32)


def hot_border_map(shape, seed, height=50.0, width=2):
    """Noise of mean 3 with `height` added on the outermost rows and columns: the source rows a border verdict admits or
    refuses carry weight in the score."""
    vol = noise_map(shape, seed)
    vol[:, :width, :] += np.float32(height)
    vol[:, -width:, :] += np.float32(height)
    vol[:, :, :width] += np.float32(height)
    vol[:, :, -width:] += np.float32(height)
    return vol


# ---- the cases ----------------------------------------------------------------------------------------------------------
APIX = 2.0
ORDINARY = ((29.0, 6.0, 1), (31.0, 5.0, 1), (45.0, 4.0, 2))

# group 1: repeat chunks.  16 x 12 x 12, the two central planes of the full plane scored; (twist, rise, csym, n_ent on both
# scored planes).  257 is prime and the window of a central plane holds at least 3 repeats, so only csym 1 reaches it.
CHUNK_SHAPE = (16, 12, 12)
CHUNK_REGION = dict(rmin=0, rmax=None, z_fraction=0.01)
CHUNK_CANDIDATES = (
    (29.0, 0.5, 1, 63), (29.0, 0.1195, 1, 255), (29.0, 0.1187, 1, 256), (29.0, 0.1186, 1, 257), (29.0, 0.1173, 1, 260),
    (29.0, 0.1, 1, 303), (29.0, 0.05905, 1, 512), (29.0, 0.0589, 1, 513), (29.0, 0.0375, 1, 804),
    (29.0, 20.0, 12, 36), (29.0, 7.0, 32, 256), (29.0, 20.0, 150, 450), (29.0, 7.0, 64, 512), (29.0, 20.0, 171, 513),
    (29.0, 14.0, 180, 900),
)
CHUNK_WANTED = dict(below=lambda n: n <= 255, at_256=lambda n: n == 256, at_257=lambda n: n == 257,
                    between=lambda n: 258 <= n <= 511, at_512=lambda n: n == 512, at_513=lambda n: n == 513,
                    above_768=lambda n: n > 768)
CSYM_MAX_SHAPE = (4, 8, 8)
CSYM_MAX_REGION = dict(rmin=0, rmax=None, z_fraction=1.0)
CSYM_MAX_CANDIDATE = (29.0, 6.0, 4096)


def chunk_map():
    """Noise of mean 3; the two planes at each end carry ten times the noise, so the far repeats of a long list (the last
    entries of the window, which read those planes) weigh in S."""
    vol = noise_map(CHUNK_SHAPE, 101)
    for sl in (slice(0, 2), slice(14, 16)):
        vol[sl] = 3 + 10 * (vol[sl] - 3)
    return vol


# group 2: tile layouts and seams.  (ny, nx, rmin, rmax, np); maps of 8 planes, the two central ones scored.  Discs inside
# the plane for every reachable (ntiles, nv), then regions with np one below, at and one above 256, 2048, 2560, 4096 and
# 4608 (discs cut by the plane's border, so their list ends on the last rows), and the full 46 x 46 plane.  A region whose
# first entry is column 0 of an odd nx (the full 65 x 65 plane, say) is not used: the reference admits no operation there
# (i2 = -0.5 for the identity), S is 0 and a spike on it shows nothing; (3, 6) is covered by 4097 ... 4608 and a disc.
TILE_NZ = 8
TILE_Z_FRACTION = 0.01
TILE_REGIONS = (
    (20, 21, 0, 9, 249), (28, 29, 0, 12.5, 489), (32, 33, 0, 15, 697), (38, 39, 0, 17.5, 973), (42, 43, 0, 20, 1245),
    (46, 47, 0, 22, 1513), (50, 51, 0, 24, 1789), (56, 57, 0, 27, 2285), (62, 63, 0, 30, 2809), (68, 69, 0, 32.5, 3313),
    (72, 73, 0, 35, 3841), (78, 79, 0, 37.5, 4421), (82, 83, 0, 40, 5013), (88, 89, 0, 43, 5785),
    (16, 16, 0, 11.292, 255), (16, 16, 0, 11.336, 256), (16, 17, 0.707, 9.975, 257),
    (44, 47, 1.871, 30.471, 2047), (45, 48, 0, 27.794, 2048), (44, 47, 0.707, 30.406, 2049),
    (50, 52, 0, 33.234, 2559), (50, 52, 2.121, 33.414, 2560), (50, 53, 2.121, 32.195, 2561),
    (64, 64, 0, 45.249, 4095), (64, 64, 0, 45.260, 4096), (63, 66, 1.225, 41.863, 4097),
    (67, 69, 0, 46.005, 4607), (68, 70, 1.225, 43.006, 4608), (67, 70, 1.871, 44.548, 4609),
    (46, 46, 0, None, 2116),
)
TILE_CANDIDATES = ((29.0, 6.0, 1), (90.0, 3.0, 2), (45.0, 4.0, 4))


def reachable_layouts():
    """Every (ntiles, nv) hs_set_region can give with at most three tiles."""
    return sorted({layout(n) for n in range(1, 3 * WORKGROUP * HS_VPT + 1)})


def tile_case(row):
    ny, nx, rmin, rmax, _ = row
    shape = (TILE_NZ, ny, nx)
    region = dict(rmin=rmin, rmax=rmax, z_fraction=TILE_Z_FRACTION)
    return spike_map_mean3(shape, 200 + ny + nx, region), region


# group 3: ring census.  One-voxel rings out to the corner; ring 0 (the axis voxel alone, 2 voxels in the slab) is merged
# with ring 1.
RING_SHAPES = ((8, 24, 24), (8, 21, 25))
RING_Z_FRACTION = 0.01
RING_CANDIDATES = ((29.0, 4.0, 1), (45.0, 4.0, 4), (-90.0, 3.0, 2))
RING_MERGED = {(8, 24, 24): ((0, 2),), (8, 21, 25): ((0, 2),)}


def rings(shape):
    """[(rmin, rmax)]: r ... r + 1 for every r out to the plane's farthest corner, RING_MERGED applied."""
    _, ny, nx = shape
    far = (ny // 2) ** 2 + (nx // 2) ** 2
    out, r = [], 0
    merged = dict(RING_MERGED.get(shape, ()))
    while r * r <= far:
        top = merged.get(r, r + 1)
        out.append((r, top))
        r = top
    return out


# group 4: borders.  (shape, map seed, candidates); the frame rmin = min(ny, nx) // 2 - 1 outwards and the full plane,
# every plane scored.  Every candidate has border_flips > 0 on its map (asserted by the host test).  The band hs_border
# decides is 8 ulp of 1.5 max(ny, nx) wide, so the long side alone makes it widest: 3 x 1024 x 250 keeps the float64 model
# of the host test at 3 s where 4 x 1024 x 1000 takes 10 s per candidate.
BORDER_CASES = (
    ((8, 24, 24), 9, ((90.0, 4.0, 1), (-90.0, 4.0, 1), (29.0, 4.0, 4), (-29.0, 4.0, 4), (45.0, 4.0, 2), (-45.0, 4.0, 2),
                      (30.0, 1.0, 1), (-30.0, 1.0, 1))),
    ((8, 21, 25), 9, ((90.0, 4.0, 1), (-90.0, 4.0, 1), (29.0, 4.0, 4), (-29.0, 4.0, 4), (45.0, 4.0, 2), (-45.0, 4.0, 2),
                      (30.0, 1.0, 1), (-30.0, 1.0, 1))),
    ((8, 25, 24), 9, ((90.0, 4.0, 1), (-90.0, 4.0, 1), (29.0, 4.0, 4), (-29.0, 4.0, 4), (45.0, 4.0, 2), (-45.0, 4.0, 2),
                      (30.0, 1.0, 1), (-30.0, 1.0, 1))),
    ((3, 1024, 250), 9, ((29.0, 2.0, 4), (-29.0, 2.0, 4), (90.0, 2.0, 1), (-90.0, 2.0, 1))),
)


def border_map(shape, seed):
    return hot_border_map(shape, seed)


def border_regions(shape):
    return dict(frame=dict(rmin=min(shape[1:]) // 2 - 1, rmax=None, z_fraction=1.0), full=dict(rmin=0, rmax=None, z_fraction=1.0))


# group 5: map sides and the z range.  Every parity of (nz, ny, nx) and every order of unequal sides; the smallest sides
# with a default region (rmax = min(ny, nx) // 2 - 1 = 1: the axis voxel, 8 planes of 16) and with any region at all.
SIDE_SHAPES = ((8, 10, 12), (9, 12, 10), (10, 9, 13), (12, 9, 10), (11, 14, 9), (11, 9, 8), (9, 11, 13), (12, 10, 9))
SIDE_REGIONS = (dict(), dict(rmin=0, rmax=None, z_fraction=1.0))
SIDE_CANDIDATES = ((29.0, 6.0, 1), (45.0, 4.0, 2), (-31.0, 5.0, 3))
SMALLEST_DEFAULT = ((16, 4, 4), (16, 4, 5), (16, 5, 4))
SMALLEST_ANY = ((2, 2, 2), (2, 3, 2), (3, 2, 2), (2, 2, 3))
SMALLEST_CANDIDATES = ((29.0, 2.0, 1), (90.0, 1.0, 2), (45.0, 3.0, 1))
SMALLEST_DEFAULT_CANDIDATES = ((29.0, 6.0, 1), (45.0, 10.0, 2), (-90.0, 5.0, 1))   # few repeats: on the axis S is a mean along z

ZR_SHAPE = (24, 16, 16)
ZR_ZERO = (slice(0, 6), slice(19, 24))          # planes set to exactly 0: z0 = 6, z1 = 18
ZR_FRACTIONS = (1.0, 0.25)                       # [6, 18) and [9, 15)
ZR_Z_FRACTIONS = (0.25, 0.5, 0.75, 1.0)          # slabs [9, 15), [6, 18), [3, 21) and every plane
ZR_CANDIDATES = {1.0: ((29.0, 6.0, 1), (29.0, 26.0, 1), (45.0, 5.0, 2)), 0.25: ((29.0, 6.0, 1), (29.0, 16.0, 1), (45.0, 5.0, 2))}
ZR_EMPTY = {1.0: ((29.0, 26.0, 1), (5, 18)), 0.25: ((29.0, 16.0, 1), (7, 8))}   # candidate, planes where S is exactly 0


def zr_map(helix_map, add_noise):
    """A noisy helix whose end planes are exactly zero (the helix builders are tests/test_gpu_symmetry_search.py's)."""
    vol = add_noise(helix_map(ZR_SHAPE, APIX, 29.0, 6.0), 71)
    for sl in ZR_ZERO:
        vol[sl] = 0
    return vol


# group 6: candidate values on a 16 x 12 x 12 noisy helix (length 32 A), the whole volume scored
VALUE_SHAPE = (16, 12, 12)
VALUE_REGION = dict(rmin=0, rmax=None, z_fraction=1.0)
VALUE_CANDIDATES = (
    (29.0, 6.0, 1), (-29.0, 6.0, 1), (180.0, 6.0, 1), (181.0, 6.0, 1), (-181.0, 6.0, 1), (389.0, 6.0, 1), (-331.0, 6.0, 1),
    (29.0, 2.0, 1), (29.0, 4.0, 1), (29.0, 8.0, 2),            # whole multiples of apix: wk = 0
    (29.0, 32.0, 1), (29.0, 40.0, 1), (29.0, 1000.0, 3),       # at and above nz apix: hsym_max = 1
    (29.0, 6.0, 7), (29.0, 6.0, 11), (-29.0, 5.0, 13),         # csym that does not divide 360
)


def value_map(helix_map, add_noise):
    return add_noise(helix_map(VALUE_SHAPE, APIX, 29.0, 6.0, radius=8.0), 81)


# ---- sensitivities ------------------------------------------------------------------------------------------------------
def lost_voxel_moves(vol, sym, mask, admitted=False):
    """|change of Pearson(vol[mask], sym[mask])| when S at ONE voxel of the mask is set to 0 (``admitted``: to the map's
    value there, for voxels where S is 0), for every voxel of the mask at once: the five sums, one term taken out."""
    v, s = vol[mask].astype(np.float64), sym[mask].astype(np.float64)
    n = len(v)
    sv, svv = v.sum(), (v * v).sum()

    def r(ss, sss, svs):
        var_v, var_s = svv - sv * sv / n, sss - ss * ss / n
        return np.where(var_s > 0, (svs - sv * ss / n) / np.sqrt(var_v * np.where(var_s > 0, var_s, 1.0)), 0.0)

    new = v if admitted else np.zeros_like(s)
    base = r(s.sum(), (s * s).sum(), (v * s).sum())
    return np.abs(r(s.sum() - s + new, (s * s).sum() - s * s + new * new, (v * s).sum() - v * s + v * new) - base)
