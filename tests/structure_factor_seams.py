"""Shared by tests/test_structure_factor_seams_host.py and tests/test_gpu_structure_factor_seams.py: the probe table of the
structure-factor kernels' launch geometry (helicon_amd/csrc/structure_factor.inc: k_sf_prepare, k_fc_absmax, k_sf_scales,
k_sf_xpass, k_sf_finish, k_sf_scale, and the shared k_circ_gemm passes and k_tfsc_c2r), the input recipe, the comparisons both
tests apply, and the defect models with which the host test shows that a comparison would notice a lost slice, tile, table
turn or strided tail.  CPU only: nothing here imports the device package.  The yardstick is tests/structure_factor_oracle.py.

Every probe names the seam it is for, the smallest shape that crosses it and the variants it runs.  Each (probe, variant) runs
three checks on noise-floored random data: the spectrum elementwise (return_fft: the check that localises a tile or a slice),
the profile per bin, and the map matched onto a target of another voxel size.  No bin and no voxel is left out.

Inputs: O.make_inputs(shape, seed, noise=4.0); the thresholds are float16(mean + 2 std) of the data and of the target, which
leave sparse spikes (std >> mean) where the fixture's 0.75 leaves a mean whose DC power grows with the voxel count squared.
Every profile that enters a per-bin or matched-map comparison (data and target, in the variant) has its weakest bin's mean
power per voxel at least FLOOR of the strongest bin's; the seeds were searched on the host for that and are fixed here.  Every
row runs all four variants but for the two cells of VARIANTS_LEFT_OUT, which says why.

Bounds: each shape's three figures as an MI355X gave them (MEASURED; profiles/structure_factor.json, "accuracy" / "seams").
Where a figure lies within the existing constant (2e-6, tests/test_gpu_structure_factor.py) the existing constant is the bound;
otherwise the bound is the figure times 4, rounded up to one significant digit.  The inputs are fixed and the device's sums
and matched maps are bit-reproducible, so a figure does not move from run to run; across seeds the per-bin figure follows
the weakest bin (a float32 transform's error is relative to the whole map), which is why the floor is a condition."""
import math
from dataclasses import dataclass
from functools import lru_cache

import numpy as np

import structure_factor_oracle as O

FLOOR = 1e-4
NOISE = 4.0
TOL_SF = TOL_MATCH = TOL_SPECTRUM = 2e-6   # the existing constants (the spectrum's is TOL_MATCH there)
MARGIN = 4.0

# what structure_factor.inc, fourier_correlation.inc and mfma_tile.inc compile in (tests/test_structure_factor_seams_host.py
# reads them from the sources)
FC_T, FC_K, THREADS = 64, 32, 256
GRID_CAP = 4096            # k_sf_prepare, k_sf_scale
ABSMAX_GRID_CAP = 256      # k_fc_absmax
SF_MAX_BINS = 726
PREPARE_REACH = GRID_CAP * THREADS            # 1,048,576: elements of a map before the strided tail
ABSMAX_REACH = ABSMAX_GRID_CAP * THREADS      # 65,536

ALL = ("plain", "mask", "thresh", "both")
SPIKE_SMALL, SPIKE_LARGE = 8.0, 8192.0


@dataclass(frozen=True)
class Probe:
    name: str
    seam: str
    shape: tuple
    apix: float
    seed: int
    variants: tuple = ALL
    spike: float = 0.0          # the absmax probes: one voxel beyond ABSMAX_REACH holds `spike` times the map's maximum
    facts: tuple = ()           # ((fact, value), ...): checked by the host test against the package's own bins and the constants

    @property
    def apix_target(self):
        return self.apix * O.TARGET_APIX_FACTOR


def _name(shape):
    return "x".join(str(s) for s in shape)


def _p(seam, shape, apix, seed, variants=ALL, spike=0.0, name=None, **facts):
    return Probe(name or _name(shape), seam, tuple(shape), apix, seed, tuple(variants), spike, tuple(sorted(facts.items())))


PROBES = [
    _p("k_sf_xpass: second column tile, 5 slices, the last of 2; k_tfsc_c2r: 3 output tiles, 3 slices", (5, 6, 130), 1.2, 5, ALL,
       ncol=66, rows=30, nbins=104, x_col_tiles=2, x_slices=5, x_last_slice=2, c2r_out_tiles=3, c2r_slices=3),
    _p("k_sf_xpass: ncol in (32, 64], both wavefront columns of one tile (rows 30: its two upper wavefronts)", (6, 5, 66), 1.2, 5, ALL,
       ncol=34, rows=30, x_col_tiles=1, x_slices=3, waves_active=2),
    _p("k_sf_xpass: all four wavefronts of one tile active (rows and ncol in (32, 64])", (7, 5, 66), 1.2, 5, ALL,
       ncol=34, rows=35, x_col_tiles=1, x_row_tiles=1, waves_active=4),
    _p("2-D: rows and ncol one past a tile", (67, 129), 2.2, 5, ALL, ncol=65, rows=67, x_col_tiles=2, x_row_tiles=2),
    _p("z pass: nz over 64 (forward K = nz, inverse K = 2 nz)", (70, 6, 10), 1.3, 5, z_tiles=2),
    _p("y pass: ny over 64", (6, 70, 10), 1.3, 5, y_tiles=2),
    _p("the bin table's second turn, 2-D", (20, 380), 1.5, 5, nbins=268, bin_turns=2),
    _p("largest legal side, z", (512, 4, 6), 1.0, 8, nbins=442, bin_turns=2),
    _p("largest legal side, y", (4, 512, 6), 1.0, 1, nbins=442, bin_turns=2),
    _p("largest legal side, x", (4, 6, 512), 1.0, 11, nbins=442, bin_turns=2, ncol=257, x_col_tiles=5, x_slices=16),
    _p("largest legal side, 2-D thin, y", (1024, 6), 1.3, 54, nbins=724, bin_turns=3),
    _p("largest legal side, 2-D thin, x", (6, 1024), 1.3, 365, nbins=724, bin_turns=3, ncol=513, x_col_tiles=9, x_slices=32),
    _p("largest 2-D image", (1024, 1024), 1.0, 6, nbins=724, bin_turns=3, ncol=513, per_map=GRID_CAP * THREADS),
    _p("k_fc_absmax: strided tail, the maximum 8 times the rest's (the scale depends on the tail; no result does: a missed tail "
       "leaves the sums below 2^63, so this row cannot fail under that defect)", (40, 41, 42), 1.1, 6, ALL, SPIKE_SMALL,
       name="40x41x42-spike8", per_map=68880, absmax_tail=1),
    _p("k_fc_absmax: strided tail, the maximum decides whether the sums overflow", (40, 41, 42), 1.1, 6, ("plain", "mask", "thresh"),
       SPIKE_LARGE, name="40x41x42-spike8192", per_map=68880, absmax_tail=1),
    _p("k_sf_prepare and k_sf_scale: strided tails", (104, 100, 202), 1.4, 6, ("plain", "mask", "both"),
       per_map=2100800, per_spec=1060800, nbins=174, prepare_tail=1, scale_tail=1),
    _p("many tiles on every axis with real data (the impulse probe's shape)", (66, 70, 130), 1.2, 5,
       x_row_tiles=73, x_col_tiles=2, z_tiles=2, y_tiles=2),
]
BY_NAME = {p.name: p for p in PROBES}
CASES = [(p.name, v) for p in PROBES for v in p.variants]

# (probe, variant): why it does not run.  Every other row runs all four variants.
VARIANTS_LEFT_OUT = {
    ("104x100x202", "thresh"): "thresh alone stays at 1e-5 to 6e-5 of the strongest bin at every seed tried: below FLOOR",
    ("40x41x42-spike8192", "both"): "the mask is 0 on the whole strided tail (z >= 38) and the threshold, which the spike lifts above "
                                    "every other voxel, removes the rest: a zero map, with no profile to compare or to meet FLOOR",
}

BATCH_SHAPE, BATCH_APIX = (5, 6, 130), 1.2
BATCH_EXPONENTS = (0, 40, -40, 13, -7)
SCALING_SHAPES = [((5, 6, 130), 1.2), ((20, 380), 1.5)]
SCALING_EXPONENTS = (20, -20, 40, -40)
SCALING_ROUTES = ("profile", "match", "match_mask")

# shape -> (spectrum error / max|F|, per-bin error of the bin's own sum, matched-map error / max|want|): the largest figure of the
# shape's probes and variants on an MI355X (profiles/structure_factor.json, "accuracy" / "seams")
MEASURED = {
    (5, 6, 130): (1.170e-07, 6.667e-07, 4.526e-07),
    (6, 5, 66): (1.744e-07, 8.302e-07, 4.929e-07),
    (7, 5, 66): (1.441e-07, 7.552e-07, 5.581e-07),
    (67, 129): (1.744e-07, 3.901e-07, 4.411e-07),
    (70, 6, 10): (1.379e-07, 5.561e-07, 2.867e-07),
    (6, 70, 10): (1.245e-07, 5.172e-07, 4.371e-07),
    (20, 380): (1.541e-07, 3.651e-06, 1.207e-06),
    (512, 4, 6): (2.553e-07, 4.098e-06, 1.050e-06),
    (4, 512, 6): (6.077e-07, 5.499e-06, 1.550e-06),
    (4, 6, 512): (1.288e-07, 1.394e-06, 1.028e-06),
    (1024, 6): (3.765e-07, 1.693e-05, 2.191e-06),
    (6, 1024): (1.506e-07, 3.358e-06, 1.416e-06),
    (1024, 1024): (3.570e-07, 5.654e-07, 2.053e-06),
    (40, 41, 42): (1.038e-06, 5.925e-07, 3.126e-07),
    (104, 100, 202): (1.588e-07, 8.596e-07, 9.029e-07),
    (66, 70, 130): (1.065e-07, 2.833e-07, 6.450e-07),
}
# the batch probe's five maps (other seeds, magnitudes 2^-40 ... 2^40) against float64, per bin: its own figure and bound.  One of
# the maps has its weakest bin at 1.4e-4 of the strongest; the table's probe of the same shape sits at 7.5e-4 and gave 6.7e-7.
MEASURED_BATCH_SF = 3.106e-06


def _round_up_one_digit(x):
    e = math.floor(math.log10(x))
    m = math.ceil(x / 10.0**e - 1e-9)
    return float(f"{m}e{e}")


def bound_from(measured, existing):
    """the existing constant where the measured figure lies within it; else measured x 4, rounded up to one significant digit"""
    return existing if measured <= existing else _round_up_one_digit(MARGIN * measured)


def bounds(p):
    """(spectrum, per bin, matched map) for the probe's shape"""
    m = MEASURED[p.shape]
    return bound_from(m[0], TOL_SPECTRUM), bound_from(m[1], TOL_SF), bound_from(m[2], TOL_MATCH)


# ---------------------------------------------------------------------------------------------------------------------------
# inputs and the yardstick
# ---------------------------------------------------------------------------------------------------------------------------
def spread_threshold(v):
    """float16(mean + 2 std) as a Python float"""
    return float(np.float16(v.mean(dtype=np.float64) + 2.0 * v.std(dtype=np.float64)))


@lru_cache(maxsize=4)
def inputs(p):
    """dict(data, target, mask, thresh, thresh_target)"""
    data, target, mask = O.make_inputs(p.shape, p.seed, noise=NOISE)
    if p.spike:
        flat = data.reshape(-1)
        at = ABSMAX_REACH + (flat.size - ABSMAX_REACH) // 2
        top = np.abs(flat).max()
        flat[at] = np.float32(p.spike) * top
        assert flat[at] == p.spike * float(top) and np.abs(flat[:ABSMAX_REACH]).max() == top
    out = dict(data=data, target=target, mask=mask, thresh=spread_threshold(data), thresh_target=spread_threshold(target))
    for a in (data, target, mask):
        a.setflags(write=False)
    return out


def variant_args(inp, variant):
    """(thresh, thresh_target, mask)"""
    t = variant in ("thresh", "both")
    return (inp["thresh"] if t else None, inp["thresh_target"] if t else None, inp["mask"] if variant in ("mask", "both") else None)


@lru_cache(maxsize=2)
def profiles(p, variant):
    """dict(qbins, sf, F, tbins, tsf): the float64 restatement's spectrum and the two profiles of the probe's inputs"""
    inp = inputs(p)
    thresh, thresh_t, mask = variant_args(inp, variant)
    qbins, sf, F = O.calculate_structural_factor(inp["data"], p.apix, thresh, mask, True)
    tbins, tsf = O.calculate_structural_factor(inp["target"], p.apix_target, thresh_t, mask)
    return dict(qbins=qbins, sf=sf, F=F, tbins=tbins, tsf=tsf)


@lru_cache(maxsize=2)
def yardstick(p, variant):
    """profiles() and `want`, the matched map"""
    inp = inputs(p)
    thresh, _, mask = variant_args(inp, variant)
    y = dict(profiles(p, variant))
    y["want"] = O.set_structural_factors(inp["data"], p.apix, y["tbins"], y["tsf"], thresh, mask)
    return y


def floors(p, variant):
    """(data, target): O.floor_ratio of the two profiles that enter the comparisons"""
    y = profiles(p, variant)
    return O.floor_ratio(p.shape, p.apix, y["sf"]), O.floor_ratio(p.shape, p.apix_target, y["tsf"])


def spectrum_error(got, want):
    return float(np.abs(got - want).max() / np.abs(want).max())


def sf_error(got, want):
    assert (want > 0).all()
    return float(np.abs(np.asarray(got) / want - 1.0).max())


def map_error(got, want):
    return float(np.abs(got - want).max() / np.abs(want).max())


def figures(y, F, sf, out):
    """(spectrum, per bin, matched map) of a device (or defect model) result against the yardstick `y`"""
    return spectrum_error(F, y["F"]), sf_error(sf, y["sf"]), map_error(out, y["want"])


# ---------------------------------------------------------------------------------------------------------------------------
# the launch geometry of a shape, from the constants
# ---------------------------------------------------------------------------------------------------------------------------
def geometry(shape, nbins):
    nx = shape[-1]
    ncol = nx // 2 + 1
    rows = int(np.prod(shape[:-1]))
    tiles = lambda n: -(-n // FC_T)
    slices = lambda n: -(-n // FC_K)
    g = dict(ncol=ncol, rows=rows, nbins=nbins, per_map=rows * nx, per_spec=rows * ncol,
             x_row_tiles=tiles(rows), x_col_tiles=tiles(ncol), x_slices=slices(nx), x_last_slice=nx - (slices(nx) - 1) * FC_K,
             c2r_out_tiles=tiles(nx), c2r_slices=slices(ncol), y_tiles=tiles(shape[-2]), z_tiles=tiles(shape[0]) if len(shape) == 3 else 0,
             bin_turns=-(-nbins // THREADS))
    # wavefronts of the first tile with work: sub-tiles of 32 x 32
    g["waves_active"] = min(2, -(-min(rows, FC_T) // 32)) * min(2, -(-min(ncol, FC_T) // 32))
    g["prepare_tail"] = int(g["per_map"] > PREPARE_REACH)
    g["scale_tail"] = int(g["per_spec"] > PREPARE_REACH)
    g["absmax_tail"] = int(g["per_map"] > ABSMAX_REACH)
    return g


# ---------------------------------------------------------------------------------------------------------------------------
# the device's pipeline in float64 NumPy, with one defect at a time
# ---------------------------------------------------------------------------------------------------------------------------
DEFECTS = ("slice_lost", "column_tile_lost", "column_tile_misread", "rows_swapped", "bins_beyond_256_lost", "prepare_tail_raw",
           "scale_tail_lost", "absmax_tail_lost", "wrong_map_scale")


def _half_columns(shape):
    """for every column of the full spectrum, its column of the half spectrum (kx or nx - kx)"""
    nx = shape[-1]
    c = np.arange(nx)
    return np.minimum(c, nx - c)


def fixed_point_sums(power, lab, nbins, amax, voxels):
    """k_sf_scales and k_sf_xpass's integer sums in Python integers: (scale, [exact sums], [sums as the 64-bit accumulators
    hold them, wrapped], the profile the device would return).  `power` is w |F|^2 over the half spectrum, lab its labels."""
    bound = 2.0 * voxels * voxels * float(amax) * float(amax)
    scale = math.ldexp(1.0, 61 - (math.frexp(bound)[1] - 1))
    q = np.rint(power.ravel() * scale)
    exact = [0] * nbins
    for s, v in zip(lab.ravel().tolist(), q.tolist()):
        exact[s] += int(v)
    wrapped = [(v + 2**63) % 2**64 - 2**63 for v in exact]
    return scale, exact, wrapped, np.array([w / scale for w in wrapped])


def half_power(F, shape):
    """(w |F|^2, labels) over the half spectrum: w = 2 off the planes kx = 0 and kx = nx / 2"""
    nx = shape[-1]
    ncol = nx // 2 + 1
    half = F[..., :ncol]
    col = np.arange(ncol)
    w = np.where((col != 0) & (2 * col != nx), 2.0, 1.0)
    return w * (half.real**2 + half.imag**2)


def model(p, variant, defect=None, arg=None):
    """(F, sf, out) as the device forms them (prepare, spectrum, sums, ratio, scaled half spectrum, c2r), in float64; `defect`
    switches one step to a launch-geometry fault.  With defect=None this is the yardstick (asserted by the host test)."""
    inp = inputs(p)
    thresh, thresh_t, mask = variant_args(inp, variant)
    y = yardstick(p, variant)
    shape = p.shape
    nx = shape[-1]
    ncol = nx // 2 + 1
    data = inp["data"].astype(np.float64)
    work = data
    if thresh:
        work = O.threshold_data(work, thresh)
    if mask is not None:
        work = work * mask.astype(np.float64)
    if defect == "prepare_tail_raw":      # the grid's first sweep is prepared, the strided tail is copied through
        flat = work.reshape(-1).copy()
        flat[PREPARE_REACH:] = data.reshape(-1)[PREPARE_REACH:]
        work = flat.reshape(shape)

    def forward(x):
        if defect == "slice_lost":        # slice `arg` of the x axis never reaches the accumulators
            x = x.copy()
            x[..., FC_K * arg:FC_K * arg + FC_K] = 0.0
        F = np.fft.fftn(x)
        hc = _half_columns(shape)
        if defect == "column_tile_lost":  # the workgroups blockIdx.y >= 1 store and sum nothing
            F = F.copy()
            F[..., hc >= FC_T] = 0.0
        if defect == "column_tile_misread":   # the second column tile reads the table's first 64 columns
            half = F[..., :ncol].copy()
            half[..., FC_T:] = half[..., :ncol - FC_T]
            F = _full_from_half(half, shape)
        if defect == "rows_swapped":      # the row tiles 0 and 1 store each other's rows (as many as the second holds)
            rows = int(np.prod(shape[:-1]))
            m = min(FC_T, rows - FC_T)
            R = F.reshape(rows, nx).copy()
            R[:m], R[FC_T:FC_T + m] = F.reshape(rows, nx)[FC_T:FC_T + m], F.reshape(rows, nx)[:m]
            F = R.reshape(shape)
        return F

    F = forward(work)
    lab = O.labels(shape, p.apix)
    nbins = len(y["qbins"])
    sf = np.bincount(lab.ravel(), weights=(F.real**2 + F.imag**2).ravel(), minlength=nbins)
    if defect == "bins_beyond_256_lost":  # the loops over the bin table stop after one turn of 256 threads
        sf[THREADS:] = 0.0
    if defect == "absmax_tail_lost":      # the maximum of the first 65,536 voxels sets the scale
        amax = np.abs(work.reshape(-1)[:ABSMAX_REACH]).max()
        sf = fixed_point_sums(half_power(F, shape), lab[..., :ncol], nbins, amax, work.size)[3]
    spec = forward(data) if mask is not None else F
    from scipy import interpolate

    target = interpolate.interp1d(y["tbins"], y["tsf"], bounds_error=False, fill_value=0)(y["qbins"])
    ratio = np.zeros_like(sf)
    nz = np.nonzero(sf)
    with np.errstate(invalid="ignore"):
        ratio[nz] = np.sqrt(target[nz] / sf[nz])
    mult = O.ratio_on_grid(y["qbins"], ratio, O.bins(shape, p.apix)[2])[..., :ncol]
    if defect == "scale_tail_lost":       # the half spectrum beyond the grid's first sweep is not multiplied
        flat = mult.reshape(-1).copy()
        flat[PREPARE_REACH:] = 1.0
        mult = flat.reshape(mult.shape)
    out = np.fft.irfftn(spec[..., :ncol] * mult, s=shape, axes=tuple(range(len(shape))))
    return F, sf, out


def _full_from_half(half, shape):
    nx = shape[-1]
    ncol = nx // 2 + 1
    full = np.empty(shape, dtype=np.complex128)
    full[..., :ncol] = half
    if ncol < nx:
        mirror = half
        for axis, n in enumerate(shape[:-1]):
            mirror = np.take(mirror, (-np.arange(n)) % n, axis=axis)
        full[..., ncol:] = np.conj(mirror[..., nx - np.arange(ncol, nx)])
    return full


def impulse_profile(shape, apix, defect=None, arg=None):
    """the profile of a unit impulse at voxel 0 under a forward-path defect (the GPU tests' impulse probe)"""
    nx = shape[-1]
    ncol = nx // 2 + 1
    x = np.zeros(shape)
    x.reshape(-1)[0] = 1.0
    if defect == "slice_lost":
        x[..., FC_K * arg:FC_K * arg + FC_K] = 0.0
    F = np.fft.fftn(x)
    if defect == "column_tile_lost":
        F[..., _half_columns(shape) >= FC_T] = 0.0
    if defect == "column_tile_misread":
        half = F[..., :ncol].copy()
        half[..., FC_T:] = half[..., :ncol - FC_T]
        F = _full_from_half(half, shape)
    if defect == "rows_swapped":
        rows = int(np.prod(shape[:-1]))
        R = F.reshape(rows, nx).copy()
        R[:FC_T], R[FC_T:2 * FC_T] = F.reshape(rows, nx)[FC_T:2 * FC_T], F.reshape(rows, nx)[:FC_T]
        F = R.reshape(shape)
    lab = O.labels(shape, apix)
    nbins = int(lab.max()) + 1
    sf = np.bincount(lab.ravel(), weights=(F.real**2 + F.imag**2).ravel(), minlength=nbins)
    if defect == "bins_beyond_256_lost":
        sf[THREADS:] = 0.0
    if defect == "absmax_tail_lost":
        amax = np.abs(x.reshape(-1)[:ABSMAX_REACH]).max()
        sf = fixed_point_sums(half_power(F, shape), lab[..., :ncol], nbins, amax, x.size)[3]
    return sf


# ---------------------------------------------------------------------------------------------------------------------------
# the batch and the exact scaling probes
# ---------------------------------------------------------------------------------------------------------------------------
@lru_cache(maxsize=1)
def batch_inputs():
    """dict(bases [5], maps [5] = 2^k bases, mask, thresh (of the base maps: one value), tbins, tsf)"""
    bases = np.stack([O.make_inputs(BATCH_SHAPE, 80 + j, noise=NOISE)[0] for j in range(len(BATCH_EXPONENTS))])
    maps = np.stack([np.ldexp(b, k) for b, k in zip(bases, BATCH_EXPONENTS)]).astype(np.float32)
    target, mask = O.make_inputs(BATCH_SHAPE, 90, noise=NOISE)[1:]
    tbins, tsf = O.calculate_structural_factor(target, BATCH_APIX * O.TARGET_APIX_FACTOR)
    return dict(bases=bases, maps=maps, mask=mask, thresh=spread_threshold(bases[0]), tbins=tbins, tsf=tsf)


def wrong_map_scale(sums, amax, voxels):
    """the profiles of a batch when map b's integer sums are divided by map b - 1's scale (map 0 by the last one's)"""
    scales = [math.ldexp(1.0, 61 - (math.frexp(2.0 * voxels * voxels * float(a) ** 2)[1] - 1)) for a in amax]
    return np.stack([s * scales[b] / scales[b - 1] for b, s in enumerate(sums)])


@lru_cache(maxsize=2)
def scaling_inputs(shape, apix):
    data, target, mask = O.make_inputs(shape, 7, noise=NOISE)
    tbins, tsf = O.calculate_structural_factor(target, apix * O.TARGET_APIX_FACTOR)
    return dict(data=data, mask=mask, tbins=tbins, tsf=tsf)


F32_MIN_NORMAL, F32_MAX = float(np.finfo(np.float32).tiny), float(np.finfo(np.float32).max)


def stays_normal(values, k):
    """every non-zero |value| 2^k lies in float32's normal range; of complex values, every real and imaginary part (the device
    holds them as two float32 planes)"""
    v = np.asarray(values)
    a = np.abs(np.concatenate([v.real.ravel(), v.imag.ravel()]) if np.iscomplexobj(v) else v.ravel())
    a = a[a > 0]
    return bool(a.size == 0 or (math.ldexp(float(a.min()), k) >= F32_MIN_NORMAL and math.ldexp(float(a.max()), k) <= F32_MAX))


def device_stages(v, qbins, target, apix):
    """What the device holds in float32 on the way of a map `v` (prepared, float64 here): the planes after the z and y forward
    passes and after the x pass, the spectrum times the interpolated ratio, and the planes after the inverse z and y passes.
    Returns (forward stages, scaled stages): the first scale with the map, the second do not (the ratio takes the factor back)."""
    lead = tuple(range(v.ndim - 1))
    forward = [np.fft.fftn(v, axes=lead[:n]) for n in range(1, len(lead) + 1)] + [np.fft.fftn(v)]
    F = forward[-1]
    lab = O.labels(v.shape, apix)
    sf = np.bincount(lab.ravel(), weights=(F.real**2 + F.imag**2).ravel(), minlength=len(qbins))
    ratio = np.zeros_like(sf)
    nz = np.nonzero(sf)
    ratio[nz] = np.sqrt(target[nz] / sf[nz])
    scaled = F * O.ratio_on_grid(qbins, ratio, O.bins(v.shape, apix)[2])
    return forward, [scaled] + [np.fft.ifftn(scaled, axes=lead[:n]) for n in range(1, len(lead) + 1)]
