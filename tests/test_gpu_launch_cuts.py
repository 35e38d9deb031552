"""Every batched device path across its compiled-in launch cut.

A long list is cut into several launches; the code after the first cut offsets the parameters, the scores, the partial sums,
the masks and the host arrays by the chunk's start.  Each test here gives a path a list of all-distinct inputs that spans
the cap more than once and ends in a short chunk whose length is no multiple of 64, and checks it

* against the float64 oracle of the path, at the tolerance of the path's own test file, on a stated sample: every 16th index,
  the 8 indices on each side of every cut, the first two and the last two (`sample`); the arg-max over the sample where the
  path's `check()` asserts one;
* against the same inputs in short calls, each of which lies inside one chunk and none of which lines up with the cap: bit for
  bit where DESIGN.md states independence of the batch (FSC, FRC, true FSC, symmetry search), within the zoom test's
  device-against-device 2e-5 for the three sweeps (each prints whether it was bit-identical).

CAPS is the one table of the caps crossed; tests/test_launch_cuts_host.py reads the .inc files and fails when a constant or
a `min` expression no longer has the value given here, so a raised cap cannot quietly turn these lists into one launch.
No tolerance is new: each is the constant of the path's own test file.  Every test prints its largest difference before it
asserts.  Measured on an MI355X ("Launch cuts", has the table and the temporary edits each test was shown to
catch): every comparison with short calls bit-identical, the sweeps' included; largest distances from the oracle 5.6e-7
(zoom), 3.6e-6 (phase score), 2.4e-7 (filtered), 5.0e-8 / 5.9e-8 (FSC / FRC curves), 1.7e-6 (sums), 7.0e-8 (true FSC),
1.2e-7 (symmetry search); 0.3 ... 2.0 s of wall time per test, oracle included."""
import functools

import numpy as np
import pytest

import fsc_oracle as FO
import true_fsc_oracle as TO
import helicon_amd as H
from helicon_amd import fsc as F
from helicon_amd.grid import build_grid
from helicon_amd.symmetry_search import SymmetrySearch
from oracle import path_b as O

from tests import phase_oracle as P
from tests import test_gpu_filtered_sweep as TF
from tests import test_gpu_fsc as TFSC
from tests import test_gpu_phase_sweep as TP
from tests import test_gpu_symmetry_search as TS
from tests import test_gpu_true_fsc as TT
from tests import test_gpu_zoom_sweep as TZ

pytestmark = pytest.mark.gpu

# the caps these tests cross (csrc/*.inc; pinned by tests/test_launch_cuts_host.py)
CAPS = {
    "ZS_BATCH": 8192,               # zoom_sweep.inc: zoom_sweep and phase_sweep, candidates per launch
    "FS_BATCH": 1024,               # filtered_sweep.inc: filt_sweep, candidates per launch ...
    "FS_BYTES": 128 << 20,          # ... and the bytes of q and T of one launch: (1 + J) planes of float32 per candidate
    "GRID_Z": 65535,                # the HIP limit of grid.y / grid.z
    "FSC_MAPS_PER_PAIR": 2,         # fourier_correlation.inc: cubes, GRID_Z // (2 n) pairs per launch
    "FRC_PAIRS": 32767,             # fourier_correlation.inc: images, pairs per launch
    "TFSC_MAPS_PER_MASK": 4,        # true_fsc.inc: GRID_Z // (4 n) masks per launch
    "HS_CANDIDATES": 65535,         # symmetry_search.inc: candidates per launch (grid.z)
}
DEVICE_TOL = 2e-5                   # test_gpu_zoom_sweep.py: the device's pipelines among themselves
SEGMENT_TOL = 2e-6                  # test_gpu_zoom_sweep.py: several segments against single-segment sweeps


def chunks(n, cap):
    """Lengths of the launches of a list of n under a cap."""
    return [min(cap, n - b0) for b0 in range(0, n, cap)]


def spans_the_cap(n, cap, full=2):
    """The list the issue asks for: `full` whole chunks and a short last one that is no multiple of 64."""
    c = chunks(n, cap)
    assert len(c) == full + 1 and c[:-1] == [cap] * full and 0 < c[-1] < cap and c[-1] % 64 != 0, (n, cap, c)
    return [cap * (k + 1) for k in range(full)]


def sample(n, cuts, stride=16, side=8):
    """Every `stride`-th index, `side` indices on each side of every cut, the first two and the last two."""
    idx = set(range(0, n, stride)) | {0, 1, n - 2, n - 1}
    for c in cuts:
        idx |= set(range(c - side, c + side))
    idx = np.array(sorted(idx))
    assert idx[0] == 0 and idx[-1] == n - 1 and all(c - 1 in idx and c in idx for c in cuts)
    return idx


def in_short_calls(call, n, step, cap):
    """`call(lo, hi)` over slices of `step`: each inside one chunk, none but the first starting on a multiple of the cap."""
    assert step < cap and all(lo % cap for lo in range(step, n, step))
    return np.concatenate([call(lo, min(n, lo + step)) for lo in range(0, n, step)], axis=-1)


def decided(ref, what):
    """A property of the INPUT: two scores within the score tolerance of the oracle's can swap places only if the oracle's
    are less than twice the tolerance apart.  An input that fails here needs another seed, not another tolerance."""
    top = np.sort(ref)[::-1]
    assert np.isfinite(ref).all() and top[0] - top[1] > 2 * TZ.SCORE_TOL, f"{what}: the oracle's two best are {top[0]:.6f} and {top[1]:.6f}"


def device_against_device(long, short, what):
    d = float(np.abs(long.astype(np.float64) - short).max())
    print(f"{what}: max |one call - short calls| = {d:.3e}; bit-identical: {np.array_equal(long, short)}")
    assert long.shape == short.shape and d <= DEVICE_TOL, what


# ------------------------------------------------------------------------------------------
# the three sweeps
# ------------------------------------------------------------------------------------------
LONG_TWISTS, LONG_RISES = np.linspace(1, 179, 131), np.linspace(3, 20, 131)


@functools.lru_cache(maxsize=None)
def _small_case():
    """16 x 24 at 2 A: two noisy images of the truth (29, 10, 1) and the 17,161 distinct candidates of the long list.  The
    second image's seed is 2: with seed 1 the oracle's two best sampled phase scores are 9e-5 apart, less than the score
    tolerance, and such an input cannot carry an arg-max assertion (`decided`)."""
    ny, nx, apix = 16, 24, 2.0
    img0, d, br = TZ.make_image(ny, nx, apix, truth=(29.0, 10.0, 1), seed=0)
    img1 = TZ.make_image(ny, nx, apix, truth=(29.0, 10.0, 1), seed=2)[0]
    grid = build_grid(LONG_TWISTS, LONG_RISES, (1,), tube_length=nx * apix)
    assert len(grid) == 17161 and grid.valid.all() and len(np.unique(grid.params, axis=0)) == len(grid)
    imgs = np.stack([img0, img1])
    imgs.setflags(write=False)
    grid.params.setflags(write=False)
    return imgs, d, br, grid.params


def test_zoom_sweep_across_zs_batch():
    """17,161 candidates: launches of 8192, 8192 and 777, two segments."""
    import torch

    apix, cutoff, size = 2.0, (8, 8), (12, 20)
    imgs, d, br, params = _small_case()
    n = len(params)
    cuts = spans_the_cap(n, CAPS["ZS_BATCH"])
    mask = O.radial_band_mask(*size)
    with H.SweepEngine(imgs.shape[1:]) as eng:
        eng.set_geometry(apix=apix, helical_diameter=d, ball_radius=br)
        multi = TZ.zoomed(eng, imgs, mask, cutoff, size, params)
        assert multi.shape == (2, n) and np.isfinite(multi).all()
        short = in_short_calls(lambda lo, hi: eng.sweep(params[lo:hi]), n, 3000, CAPS["ZS_BATCH"])
        # the device entry point with a row stride: the padding stays, the scores are sweep()'s
        ld = n + 7
        dp = torch.as_tensor(params.copy(), device="cuda")
        ds = torch.full((2, ld), -2.0, dtype=torch.float32, device="cuda")
        eng.sweep_device(dp.data_ptr(), n, ds.data_ptr(), ld_scores=ld)
        eng.synchronize()
        strided = ds.cpu().numpy()
        singles = np.stack([TZ.zoomed(eng, imgs[s], mask, cutoff, size, params)[0] for s in range(2)])
    device_against_device(multi, short, "zoom sweep")
    assert np.array_equal(strided[:, :n], multi) and (strided[:, n:] == -2.0).all()
    d_seg = float(np.abs(multi.astype(np.float64) - singles).max())
    print(f"zoom sweep: max |two segments - single-segment sweeps| = {d_seg:.3e}")
    assert d_seg <= SEGMENT_TOL
    idx = sample(n, cuts)
    spectra = TZ.oracle_spectra(params[idx], imgs.shape[1:], apix, d, br, cutoff, size)
    for s in range(2):
        ref = TZ.oracle_scores(imgs[s], params[idx], mask, apix, d, br, cutoff, size, spectra=spectra)
        decided(ref, "the oracle's sampled scores")
        TZ.check(multi[s][idx], ref, f"zoom sweep across ZS_BATCH, segment {s}, {len(idx)} sampled")


def test_phase_sweep_across_zs_batch():
    """The same images, list and zoom with the phase score at weight 0.5: score, amplitude and phase of every launch."""
    apix, cutoff, size, w = 2.0, (8, 8), (12, 20), 0.5
    imgs, d, br, params = _small_case()
    n = len(params)
    cuts = spans_the_cap(n, CAPS["ZS_BATCH"])
    mask = O.radial_band_mask(*size)
    names = ("score", "amplitude", "phase")
    with H.SweepEngine(imgs.shape[1:]) as eng:
        eng.set_geometry(apix=apix, helical_diameter=d, ball_radius=br)
        multi = TP.parts(eng, imgs, mask, cutoff, size, params, weight=w)
        assert all(x.shape == (2, n) and np.isfinite(x).all() for x in multi)
        pieces = [eng.sweep_parts(params[lo: lo + 3000]) for lo in range(0, n, 3000)]
        assert 3000 < CAPS["ZS_BATCH"] and all(lo % CAPS["ZS_BATCH"] for lo in range(3000, n, 3000))
        singles = [TP.parts(eng, imgs[s], mask, cutoff, size, params, weight=w) for s in range(2)]
    for k, name in enumerate(names):
        device_against_device(multi[k], np.concatenate([p[k] for p in pieces], axis=-1), f"phase sweep, {name}")
        d_seg = max(float(np.abs(multi[k][s].astype(np.float64) - singles[s][k][0]).max()) for s in range(2))
        print(f"phase sweep, {name}: max |two segments - single-segment sweeps| = {d_seg:.3e}")
        assert d_seg <= SEGMENT_TOL
    idx = sample(n, cuts)
    for s in range(2):
        ref_amp, ref_ph = P.scores(imgs[s], params[idx], mask, apix, d, br, cutoff, size)
        for k, ref in enumerate(((1 - w) * ref_amp + w * ref_ph, ref_amp, ref_ph)):
            decided(ref, "the oracle's sampled scores")
            TP.check(multi[k][s][idx], ref, f"phase sweep across ZS_BATCH, segment {s}, {names[k]}, {len(idx)} sampled")


def test_filtered_sweep_across_fs_batch():
    """The first 2,500 rows of the long list on 16 x 24 -> 16 x 16, (lp, hp) = (0.3, 0.05): launches of 1024, 1024 and 452,
    two segments."""
    apix, cutoff, size, lp, hp = 2.0, (8, 8), (16, 16), 0.3, 0.05
    imgs, d, br, params = _small_case()
    params = params[:2500]
    n = len(params)
    plane, terms = size[0] * size[1], 2                                 # even sides: one operator pair per Gaussian
    assert CAPS["FS_BYTES"] // ((1 + terms) * plane * 4) > CAPS["FS_BATCH"]   # FS_BATCH is the branch of the min taken
    cuts = spans_the_cap(n, CAPS["FS_BATCH"])
    mask = O.radial_band_mask(*size)
    with H.SweepEngine(imgs.shape[1:]) as eng:
        eng.set_geometry(apix=apix, helical_diameter=d, ball_radius=br)
        multi = TF.filtered(eng, imgs, mask, cutoff, size, lp, hp, params)
        assert multi.shape == (2, n) and np.isfinite(multi).all()
        short = in_short_calls(lambda lo, hi: eng.sweep(params[lo:hi]), n, 700, CAPS["FS_BATCH"])
        singles = np.stack([TF.filtered(eng, imgs[s], mask, cutoff, size, lp, hp, params)[0] for s in range(2)])
    device_against_device(multi, short, "filtered sweep (FS_BATCH)")
    d_seg = float(np.abs(multi.astype(np.float64) - singles).max())
    print(f"filtered sweep (FS_BATCH): max |two segments - single-segment sweeps| = {d_seg:.3e}")
    assert d_seg <= SEGMENT_TOL
    idx = sample(n, cuts)
    for s in range(2):
        ref = TF.oracle_scores(imgs[s], params[idx], mask, apix, d, br, cutoff, size, lp, hp)
        decided(ref, "the oracle's sampled scores")
        TF.check(multi[s][idx], ref, f"filtered sweep across FS_BATCH, segment {s}, {len(idx)} sampled")


@pytest.mark.parametrize("side,terms,n,step", [(128, 2, 1500, 500), (127, 4, 900, 300)])
def test_filtered_sweep_across_fs_bytes(side, terms, n, step):
    """No zoom, (lp, hp) = (0.3, 0.05).  128 x 128: J = 2 planes of T beside q, 128 MiB / (3 * 16384 * 4) = 682 candidates
    per launch, 1,500 candidates in launches of 682, 682 and 136.  127 x 127: odd sides take the operator pairs of the
    imaginary parts too, J = 4, 416 per launch, 900 candidates in launches of 416, 416 and 68.  The oracle at this size is the
    slow part, so the sample is every 25th index and the 4 on each side of every cut."""
    apix, lp, hp = 2.0, 0.3, 0.05
    fit = CAPS["FS_BYTES"] // ((1 + terms) * side * side * 4)
    assert fit == {128: 682, 127: 416}[side] and fit < CAPS["FS_BATCH"]       # FS_BYTES is the branch of the min taken
    img, d, br = TF.make_image(side, side, apix)
    grid = build_grid(np.linspace(20, 40, 50), np.linspace(4, 9, 30), (1,), tube_length=side * apix)
    params = grid.params[:n]
    assert len(params) == n and len(np.unique(params, axis=0)) == n
    cuts = spans_the_cap(n, fit)
    mask = O.radial_band_mask(side, side)
    with H.SweepEngine((side, side)) as eng:
        eng.set_geometry(apix=apix, helical_diameter=d, ball_radius=br)
        got = TF.filtered(eng, img, mask, None, None, lp, hp, params)
        assert got.shape == (1, n) and np.isfinite(got).all()
        short = in_short_calls(lambda lo, hi: eng.sweep(params[lo:hi]), n, step, fit)
    device_against_device(got, short, f"filtered sweep (FS_BYTES, {side} x {side})")
    idx = sample(n, cuts, stride=25, side=4)
    ref = TF.oracle_scores(img, params[idx], mask, apix, d, br, None, None, lp, hp)
    decided(ref, "the oracle's sampled scores")
    TF.check(got[0][idx], ref, f"filtered sweep across FS_BYTES, {side} x {side}, {len(idx)} sampled")


# ------------------------------------------------------------------------------------------
# Fourier shell / ring correlation
# ------------------------------------------------------------------------------------------
FSC_SIDE = 8
MAX_SKIPPED = 0.05      # of the seeds tried


def _floor_ratios(a, b, full):
    """fsc_oracle.floor_ratio(fsc_oracle.sums_3d(a[i], b[i], full)) of a stack of pairs at once: the same float64 den1 and
    den2, summed over the oracle's own shell table by a matrix product."""
    n = a.shape[-1]
    fft = np.fft.fftn if full else np.fft.rfftn
    shell = (FO.shell_3d_full if full else FO.shell_3d_half)(n).ravel()
    onehot = (shell[:, None] == np.arange(n // 2 + 1)[None, :]).astype(np.float64)
    out = np.ones(len(a))
    for m in (a, b):
        den = (np.abs(fft(m.astype(np.float64), axes=(1, 2, 3))) ** 2).reshape(len(m), -1) @ onehot
        out = np.minimum(out, np.where(den > 0, den, np.inf).min(axis=1) / den.max(axis=1))
    return out


@functools.lru_cache(maxsize=None)
def _cube_pairs():
    """8,230 pairs of 8^3 maps: make_map_pair(8, seed, dc="auto") for seeds 0, 1, 2, ... in order, a seed kept only if the
    oracle's floor_ratio is >= FLOOR on the half and on the full spectrum (a property of the input: the float64 sums alone
    decide it; the tests assert it again, with fsc_oracle's own functions, on every pair they compare)."""
    n = FSC_SIDE
    cap = CAPS["GRID_Z"] // (CAPS["FSC_MAPS_PER_PAIR"] * n)
    assert cap == 4095
    want, block = 2 * cap + 40, 1024
    a, b, kept_seeds, seed = [], [], [], 0
    while len(kept_seeds) < want:
        pairs = [FO.make_map_pair(n, s, dc="auto") for s in range(seed, seed + block)]
        pa, pb = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
        ok = np.minimum(_floor_ratios(pa, pb, False), _floor_ratios(pa, pb, True)) >= TFSC.FLOOR
        a.append(pa[ok])
        b.append(pb[ok])
        kept_seeds += list(seed + np.flatnonzero(ok))
        seed += block
    tried = int(kept_seeds[want - 1]) + 1
    skipped = tried - want
    print(f"FSC cubes: {want} pairs from {tried} seeds, {skipped} skipped ({skipped / tried:.2%})")
    assert skipped <= MAX_SKIPPED * tried
    a, b = np.concatenate(a)[:want], np.concatenate(b)[:want]
    assert len(np.unique(a.reshape(want, -1), axis=0)) == want
    a.setflags(write=False)
    b.setflags(write=False)
    return a, b, cap


def test_fsc_cubes_across_the_grid_limit():
    """8,230 pairs of 8^3 maps: launches of 4095, 4095 and 40 pairs."""
    a, b, cap = _cube_pairs()
    n, batch = FSC_SIDE, len(a)
    cuts = spans_the_cap(batch, cap)
    idx = sample(batch, cuts)
    oracle_sums = [np.stack([FO.sums_3d(a[i], b[i], full) for i in idx]) for full in (False, True)]
    assert all(FO.floor_ratio(s) >= TFSC.FLOOR for per_full in oracle_sums for s in per_full)
    for full in (False, True):
        big = F.fsc_sums_3d(a, b, full)
        assert big.shape == (batch, n // 2 + 1, 3)
        short = np.concatenate([F.fsc_sums_3d(a[lo: lo + 1000], b[lo: lo + 1000], full) for lo in range(0, batch, 1000)])
        assert all(lo % cap for lo in range(1000, batch, 1000))
        same = np.array_equal(big, short)
        print(f"FSC cubes full={int(full)}: max |one call - calls of 1000| = {float(np.abs(big - short).max()):.3e}; bit-identical: {same}")
        assert same
        rev = np.array_equal(F.fsc_sums_3d(a[::-1], b[::-1], full), big[::-1])
        print(f"FSC cubes full={int(full)}: the reversed batch gives the reversed result: {rev}")
        assert rev
        want = oracle_sums[int(full)]
        scale = np.sqrt(want[:, :, 1] * want[:, :, 2])
        assert (scale > 0).all()
        e_sums = float((np.abs(big[idx] - want) / scale[:, :, None]).max())
        curves = H.calc_fsc_batch(a, b, 2.0, per_shell=full)
        if full:
            ref = np.stack([FO.calc_fsc_per_shell(a[i], b[i], 2.0) for i in idx])
            e_fsc = float(np.abs(curves[idx] - ref).max())
        else:
            ref = np.stack([FO.calc_fsc(a[i], b[i], 2.0) for i in idx])
            assert curves[idx].shape == ref.shape and np.array_equal(curves[idx][:, :, 0], ref[:, :, 0])
            e_fsc = float(np.abs(curves[idx][:, :, 1] - ref[:, :, 1]).max())
        print(f"FSC cubes full={int(full)}: {len(idx)} sampled pairs: max |fsc - float64| = {e_fsc:.3e}, sums = {e_sums:.3e}")
        assert e_fsc <= TFSC.TOL_FSC_3D and e_sums <= TFSC.TOL_SUMS


def _image_pairs(batch, seed, shape=(8, 8), signal=8.0, sigma=1.5):
    """make_map_pair(0, ., shape=shape, dc="auto")'s recipe in one vectorised draw."""
    from scipy.ndimage import gaussian_filter

    rng = np.random.default_rng(seed)
    full = (batch,) + shape
    sig = gaussian_filter(rng.standard_normal(full), (0, sigma, sigma)) * signal
    offset = 1.0 / np.sqrt(min(shape))
    board = offset * (1.0 - 2.0 * ((np.arange(shape[0])[:, None] + np.arange(shape[1])[None, :]) % 2))
    a, b = (sig + rng.standard_normal(full) + offset + board for _ in range(2))
    return a.astype(np.float16).astype(np.float32), b.astype(np.float16).astype(np.float32)


def test_frc_images_across_the_pair_cap():
    """32,807 pairs of 8 x 8 images: launches of 32,767 and 40 pairs."""
    cap, shape = CAPS["FRC_PAIRS"], (8, 8)
    batch = cap + 40
    cuts = spans_the_cap(batch, cap, full=1)
    a, b = _image_pairs(batch, 77, shape)
    assert len(np.unique(a.reshape(batch, -1), axis=0)) == batch
    others = np.random.default_rng(78).choice(batch, 48, replace=False)
    idx = np.unique(np.concatenate([np.arange(cuts[0] - 8, cuts[0] + 8), others]))
    # the oracle floor on every sampled pair; one that misses it is redrawn from the next seed of make_map_pair
    oracle_sums, redraws, seed = {}, 0, 0
    for i in idx:
        s = FO.sums_2d(a[i], b[i])
        while FO.floor_ratio(s) < TFSC.FLOOR:
            a[i], b[i] = FO.make_map_pair(0, seed, shape=shape, dc="auto")
            s = FO.sums_2d(a[i], b[i])
            seed += 1
            redraws += 1
        oracle_sums[int(i)] = s
    print(f"FRC images: {len(idx)} sampled pairs, {redraws} redrawn")
    assert redraws <= MAX_SKIPPED * (len(idx) + redraws)
    big = F.frc_sums_2d(a, b)
    assert big.shape == (batch, min(shape) // 2 + 1, 3)
    short = np.concatenate([F.frc_sums_2d(a[lo: lo + 5000], b[lo: lo + 5000]) for lo in range(0, batch, 5000)])
    assert all(lo % cap for lo in range(5000, batch, 5000))
    same = np.array_equal(big, short)
    print(f"FRC images: max |one call - calls of 5000| = {float(np.abs(big - short).max()):.3e}; bit-identical: {same}")
    assert same
    e_frc = e_sums = 0.0
    for i in idx:
        want = oracle_sums[int(i)]
        empty = want[:, 1] == 0
        scale = np.sqrt(want[:, 1] * want[:, 2])
        scale[empty] = 1.0
        assert (big[i][empty] == 0).all()
        e_sums = max(e_sums, float((np.abs(big[i] - want) / scale[:, None]).max()))
        e_frc = max(e_frc, float(np.abs(F._ratio(big[i]) - FO.calc_frc_2d(a[i], b[i], 1.5)[1]).max()))
    print(f"FRC images: {len(idx)} sampled pairs: max |frc - float64| = {e_frc:.3e}, sums = {e_sums:.3e}")
    assert e_frc <= TFSC.TOL_FRC_2D and e_sums <= TFSC.TOL_SUMS


# ------------------------------------------------------------------------------------------
# true FSC
# ------------------------------------------------------------------------------------------
def test_true_fsc_masks_across_the_grid_limit():
    """4,131 masks on one 8^3 context: launches of 2047, 2047 and 37 masks, after a call with 3 masks (the scratch grows)."""
    n = FSC_SIDE
    cap = CAPS["GRID_Z"] // (CAPS["TFSC_MAPS_PER_MASK"] * n)
    assert cap == 2047
    batch = 2 * cap + 37
    cuts = spans_the_cap(batch, cap)
    a, b = _cube_pairs()[0][0], _cube_pairs()[1][0]                      # a pair that meets the floor
    assert FO.floor_ratio(FO.sums_3d(a, b)) >= TT.FLOOR and FO.floor_ratio(FO.sums_3d(a, b, True)) >= TT.FLOOR
    rng = np.random.default_rng(91)
    u = tuple(rng.uniform(0, 2 * np.pi, size=(n, n, n // 2 + 1)) for _ in range(2))
    m1, m2 = (rng.uniform(0.25, 1.0, size=(batch, n, n, n)).astype(np.float32) for _ in range(2))
    cutoff = TT._cutoff(n)
    idx = np.unique(np.concatenate([np.arange(c - 8, c + 8) for c in cuts] + [[0, 1, batch - 2, batch - 1]]))
    ora = TO.OracleTrueFSC(a, b, TT.APIX, cutoff, phases=u)
    with H.TrueFSC(a, b, TT.APIX, cutoff, phases=u) as dev, H.TrueFSC(a, b, TT.APIX, cutoff, phases=u) as again:
        assert dev.m_cut == ora.m_cut
        first = dev.masked_sums(m1[:3], m2[:3])                           # a small first call: tf_scratch has to grow next
        for per_shell in (False, True):
            for name, second in (("two mask sets", m2), ("one mask set", None)):
                what = f"true FSC, {name}, per_shell={int(per_shell)}"
                big = dev.masked_sums(m1, second, per_shell)
                assert big.shape == (batch, 2, n // 2 + 1, 3)
                short = np.concatenate([dev.masked_sums(m1[lo: lo + 700], None if second is None else second[lo: lo + 700], per_shell)
                                        for lo in range(0, batch, 700)])
                assert all(lo % cap for lo in range(700, batch, 700))
                other = again.masked_sums(m1, second, per_shell)
                same, same_ctx = np.array_equal(big, short), np.array_equal(big, other)
                print(f"{what}: max |one call - calls of 700| = {float(np.abs(big - short).max()):.3e}; bit-identical: {same}; "
                      f"a second context bit-identical: {same_ctx}")
                assert same and same_ctx
                if not per_shell and second is not None:
                    assert np.array_equal(big[:3], first)
                # the true pair's sums are hh_fsc_3d's of the host-masked maps
                q = m1 if second is None else second
                host = F.fsc_sums_3d(a[None] * m1[idx], b[None] * q[idx], per_shell)
                same_host = np.array_equal(big[idx, 0], host)
                print(f"{what}: the true pair's sums equal fsc_sums_3d of the host-masked maps on {len(idx)} masks: {same_host}")
                assert same_host
                # and the float64 restatement, at the bounds of test_gpu_true_fsc.py
                want = ora.masked_sums(m1[idx], q[idx], per_shell)
                assert all(FO.floor_ratio(want[j, k]) >= TT.FLOOR for j in range(len(idx)) for k in range(2))
                e_t = float(np.abs(F._ratio(big[idx, 0]) - F._ratio(want[:, 0])).max())
                e_n = float(np.abs(F._ratio(big[idx, 1]) - F._ratio(want[:, 1])).max())
                print(f"{what}: {len(idx)} sampled masks: max |fsc_t - float64| = {e_t:.3e}, |fsc_n - float64| = {e_n:.3e}")
                assert e_t <= TT.TOL_FSC_3D and e_n <= TT.TOL_ROUND_TRIP


# ------------------------------------------------------------------------------------------
# symmetry search
# ------------------------------------------------------------------------------------------
def test_symmetry_search_across_the_grid_limit():
    """65,792 candidates on a 16^3 map with a budget that alone would hold them all: the grid-dimension cap cuts the list
    into launches of 65,535 and 257.  Measured on an MI355X: kernel_ms = 4.1 for the one long search (the estimate was 1e9
    gathers; the default region of a 16^3 map is far smaller), 0.4 s of wall time for the test, 1.2e-7 from the oracle."""
    cap = CAPS["HS_CANDIDATES"]
    vol = TS.add_noise(TS.helix_map((16, 16, 16), 2.0, 29.0, 6.0, radius=9.0, sigma=2.5), 71)
    params = np.array([(tw, rs, 1.0) for tw in np.linspace(10, 60, 256) for rs in np.linspace(4, 12, 257)])
    n = len(params)
    assert n == 65792 and len(np.unique(params, axis=0)) == n
    cuts = spans_the_cap(n, cap, full=1)
    with SymmetrySearch(vol, 2.0, partial_bytes=1 << 40) as ss:
        before = ss.launches
        got = ss.search(params)
        ms = ss.kernel_ms
        print(f"symmetry search: {n} candidates in {ss.launches - before} launches, kernel_ms = {ms:.1f}")
        assert ss.launches - before == 2                                  # the budget holds the list: the grid limit made the cut
        short = np.concatenate([ss.search(params[lo: lo + 10000]) for lo in range(0, n, 10000)])
        assert all(lo % cap for lo in range(10000, n, 10000))
    with SymmetrySearch(vol, 2.0) as default:
        under_default = default.search(params)
    same, same_default = np.array_equal(got, short), np.array_equal(got, under_default)
    print(f"symmetry search: max |one call - calls of 10000| = {float(np.abs(got - short).max()):.3e}; bit-identical: {same}; "
          f"under the default budget bit-identical: {same_default}")
    assert np.isfinite(got).all() and same and same_default
    others = np.random.default_rng(72).choice(n, 32, replace=False)
    idx = np.unique(np.concatenate([np.arange(cuts[0] - 8, cuts[0] + 8), others]))
    ref = TS.oracle_scores(vol, 2.0, params[idx], TS.region_mask(vol.shape))
    err = float(np.abs(got[idx] - ref).max())
    print(f"symmetry search: max |score - oracle| = {err:.3e} over {len(idx)} sampled candidates")
    assert err < TS.TOL
