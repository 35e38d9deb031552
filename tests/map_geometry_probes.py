"""Shared by tests/test_map_geometry_probes_host.py and tests/test_gpu_map_geometry_probes.py: the probe table of the 3-D map
resampling kernels (k_f32_to_f64 / k_spline_prefilter / k_map_cubic and k_apply_helical_symmetry with its host plan in
helicon_hip.hip; k_map_proj_slices / k_map_proj_columns in map_filter.inc), each probe's reference, the comparison both tests
apply, and the wrong-rule variants the host test uses to show that a comparison would notice a defect.  CPU only: nothing here
imports the device package.

kind            call on the device                                                   reference
transform_map   helicon_amd.transform_map(vol, scale, rot, tilt, psi, dx, dy, dz)    oracle.symmetrize.transform_map (float64)
helical         helicon_amd.apply_helical_symmetry(vol, apix, twist, rise, ...)      oracle.symmetrize.apply_helical_symmetry
symmetrize      helicon_amd.symmetrize_transform_map(vol, ...)                       the two above composed with np_filter_3d
projections     helicon_amd.generate_xyz_projections(vol, is_amyloid, apix), or      float64 sum(axis=...) on the same slab
                hh_map_projections(vol, begin, end) where args holds "slab"

Bounds are the project's own (compare()): transform_map 2e-6 max|want| with the zero pattern equal (test_gpu_path_a.py),
helical 1e-6 absolute on inputs in [0, 1] (test_gpu_parity.py), projections 1e-6 max|want| per projection on inputs in [0, 1]
with an empty slab compared exactly, symmetrize 2e-6 max|want| (test_gpu_map_input.py).  No pixel is left out.

The device forms its rotation matrix, and its cos / sin, on the host, and NumPy may differ from that in the last bit.  The
restatements here (transform_map_numpy, helical_numpy; bit-identical to oracle/symmetrize.py with no rule changed) take a
``nudge`` that moves what may so differ by one ulp, and the host test shows that no probe's exact items depend on it.  What
cannot differ is not nudged: cos 0 = 1 and sin 0 = 0 hold in every libm, and sums and products of 0 and +-1 do not round, so
a matrix entry that no non-zero angle enters (every entry of an identity rotation; the z row and column of a rot / psi only
probe) and the (hi, ci) pair whose angle is exactly 0 are exact on both sides.  That is what lets the border probes — identity
rotation, integer shifts, samples exactly on 0 and n - 1 — stand with no pixel exempted.
"""
import zlib
from dataclasses import dataclass, field

import numpy as np

from oracle import symmetrize as S

F32, F64 = np.float32, np.float64
BOUND_TRANSFORM, BOUND_HELICAL, BOUND_PROJ, BOUND_SYMMETRIZE = 2e-6, 1e-6, 1e-6, 2e-6


@dataclass(frozen=True)
class Probe:
    name: str
    kind: str
    rule: str                      # "kernel: the rule the probe reaches"
    make: object                   # () -> dict of input arrays
    args: dict = field(default_factory=dict)

    def inputs(self):
        return self.make()


def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def _sname(shape):
    return "x".join(str(int(v)) for v in shape)


def _tname(dtype):
    return np.dtype(dtype).name.replace("float", "f").replace("int", "i")


def _unit(name, shape, dtype=F32):
    """Random values in [0, 1) that float32 holds (the wrappers compute on float32 whatever arrives)."""
    return _rng(name).random(shape, dtype=F32).astype(dtype)


def _step(shape, dtype=F32):
    v = np.full(shape, 0.25, dtype=dtype)
    v[shape[0] // 2:, :, :] += 0.25
    v[:, shape[1] // 2:, :] += 0.125
    v[:, :, shape[2] // 2:] = 1.0
    return v


def np_filter_3d(data, low_pass_fraction=0, high_pass_fraction=0):
    """lib/filters.py:349-372 as tests/test_gpu_map_input.py restates it (asserted equal by the host test)."""
    fft = np.fft.fftn(data)
    nz, ny, nx = fft.shape
    Z, Y, X = np.meshgrid(np.arange(nz, dtype=F32) - nz // 2, np.arange(ny, dtype=F32) - ny // 2, np.arange(nx, dtype=F32) - nx // 2, indexing="ij")
    Z /= nz // 2
    Y /= ny // 2
    X /= nx // 2
    R2 = X**2 + Y**2 + Z**2
    if 0 < low_pass_fraction < 1:
        fft *= np.fft.fftshift(np.exp(-np.log(2) / low_pass_fraction**2 * R2))
    if 0 < high_pass_fraction < 1:
        fft *= np.fft.fftshift(1.0 - np.exp(-np.log(2) / high_pass_fraction**2 * R2))
    return np.real(np.fft.ifftn(fft))


# ---------------------------------------------------------------------------------------------- transform_map, restated
def _rz(a):
    c, s = np.cos(np.deg2rad(a)), np.sin(np.deg2rad(a))
    return np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])


def _ry(a):
    c, s = np.cos(np.deg2rad(a)), np.sin(np.deg2rad(a))
    return np.array([[c, 0.0, s], [0.0, 1.0, 0.0], [-s, 0.0, c]])


def euler_matrix(rot, tilt, psi, reverse=False):
    return _rz(psi) @ _ry(tilt) @ _rz(rot) if reverse else _rz(rot) @ _ry(tilt) @ _rz(psi)


def inexact_entries(rot, tilt, psi):
    """The matrix entries a non-zero angle enters (module docstring): those that move when every non-zero angle does."""
    moved = euler_matrix(*(a + 0.123 * (k + 1) if a else a for k, a in enumerate((rot, tilt, psi))))
    return [int(e) for e in np.flatnonzero((moved != euler_matrix(rot, tilt, psi)).ravel())]


def map_coords(shape, scale=1.0, rot=0, tilt=0, psi=0, dx=0, dy=0, dz=0, *, nudge=None, float_centre=False, plus_shift=False,
               reverse_euler=False, scale_offset=False):
    """The (z, y, x) sampling coordinates of transform_map.  ``nudge`` = (entry, +-1) moves one matrix entry one ulp."""
    nz, ny, nx = shape
    cz, cy, cx = (nz / 2.0, ny / 2.0, nx / 2.0) if float_centre else (nz // 2, ny // 2, nx // 2)
    Z, Y, X = np.meshgrid(np.arange(nz, dtype=np.int32) - cz, np.arange(ny, dtype=np.int32) - cy, np.arange(nx, dtype=np.int32) - cx, indexing="ij")
    if scale != 1.0:
        Z, Y, X = Z * scale, Y * scale, X * scale
    xyz = np.vstack((X.ravel(), Y.ravel(), Z.ravel())).astype(F64)
    m = euler_matrix(rot, tilt, psi, reverse_euler)
    if nudge is not None:
        m.flat[nudge[0]] = np.nextafter(m.flat[nudge[0]], np.inf * nudge[1])
    p = m @ xyz
    sign = 1 if plus_shift else -1
    off = [cx + sign * dx, cy + sign * dy, cz + sign * dz]
    if scale_offset:
        off = [o * scale for o in off]
    p[0] += off[0]
    p[1] += off[1]
    p[2] += off[2]
    return p[[2, 1, 0]]


def spline_coefficients(data, *, skip_axis=None, stride_mixup=False):
    """The prefilter on the three axes in turn.  ``stride_mixup``: the lines of axis 1 start where they should and are walked
    with axis 2's stride (1 instead of nx), one after the other on the flat array."""
    c = np.asarray(data, dtype=F64)
    nz, ny, nx = c.shape
    for ax in range(3):
        if ax == skip_axis:
            continue
        if ax == 1 and stride_mixup:
            flat = np.ascontiguousarray(c).ravel().copy()
            for line in range(nz * nx):
                start = (line // nx) * ny * nx + line % nx
                flat[start:start + ny] = S._spline_prefilter_axis(flat[start:start + ny], 0)
            c = flat.reshape(nz, ny, nx)
        else:
            c = S._spline_prefilter_axis(c, ax)
    return c


def sample_cubic(c, coords, *, exclusive=False, clamp=False, w3_direct=False):
    """oracle.symmetrize.map_coordinates_cubic after its prefilter, with the border verdict, the tap fold and w3 exposed."""
    shape = c.shape
    inside = np.ones(coords.shape[1], dtype=bool)
    for d in range(3):
        upper = (coords[d] < shape[d] - 1) if exclusive else (coords[d] <= shape[d] - 1)
        inside &= (coords[d] >= 0) & upper
    out = np.zeros(coords.shape[1], dtype=F64)
    cc = coords[:, inside]
    idx, w = [], []
    for d in range(3):
        f = np.floor(cc[d])
        y = cc[d] - f
        zc = 1.0 - y
        w1 = (y * y * (y - 2.0) * 3.0 + 4.0) / 6.0
        w2 = (zc * zc * (zc - 2.0) * 3.0 + 4.0) / 6.0
        w0 = zc * zc * zc / 6.0
        w3 = y * y * y / 6.0 if w3_direct else 1.0 - w0 - w1 - w2
        w.append((w0, w1, w2, w3))
        start = f.astype(np.int64) - 1
        fold = (lambda i, n: np.clip(i, 0, n - 1)) if clamp else S._mirror
        idx.append([fold(start + t, shape[d]) for t in range(4)])
    acc = np.zeros(cc.shape[1], dtype=F64)
    for a in range(4):
        for b in range(4):
            for e in range(4):
                acc += c[idx[0][a], idx[1][b], idx[2][e]] * (w[0][a] * w[1][b] * w[2][e])
    out[inside] = acc
    return out


def transform_map_numpy(data, scale=1.0, rot=0, tilt=0, psi=0, dx=0, dy=0, dz=0, *, nudge=None, coefficients=None, skip_axis=None,
                        stride_mixup=False, exclusive=False, clamp=False, w3_direct=False, **coord_rules):
    """oracle.symmetrize.transform_map with its rules exposed; the defaults ARE the oracle (asserted bit for bit)."""
    d = np.asarray(data)
    c = spline_coefficients(d, skip_axis=skip_axis, stride_mixup=stride_mixup) if coefficients is None else coefficients
    coords = map_coords(d.shape, scale, rot, tilt, psi, dx, dy, dz, nudge=nudge, **coord_rules)
    out = sample_cubic(c, coords, exclusive=exclusive, clamp=clamp, w3_direct=w3_direct)
    return out.astype(d.dtype if d.dtype.kind == "f" else F64).reshape(d.shape)


# ---------------------------------------------------------------------------------------- apply_helical_symmetry, restated
def z_range(data, fraction, *, threshold_dtype=None, zmid_remainder=True, half_round=True, ge=False):
    """transforms.py:92-99: the slices above 1 % of the peak slice, narrowed to ``fraction`` of nz0 about their middle.
    ``threshold_dtype`` forms the threshold in that type (None: as this NumPy forms 0.01 * float32)."""
    nz0 = data.shape[0]
    profile_z = np.sum(np.sum(data, axis=-1), axis=-1)
    peak = np.max(profile_z)
    threshold = 0.01 * peak if threshold_dtype is None else threshold_dtype(threshold_dtype(0.01) * threshold_dtype(peak))
    hit = np.where(profile_z >= threshold if ge else profile_z > threshold)[0]
    z0, z1 = hit[0], hit[-1]
    zmid = (z0 + z1) // 2 + ((z0 + z1) % 2 if zmid_remainder else 0)
    half = (int(nz0 * fraction + 0.5) if half_round else int(nz0 * fraction)) // 2
    return max(z0, zmid - half), min(z1, zmid + half), float(threshold)


def helical_numpy(data, apix, twist_degree, rise_angstrom, csym=1, fraction=1.0, new_size=None, new_apix=None, *, nudge=None, trace=None,
                  x_int_centre=False, y_float_centre=False, z1_inclusive=False, z0_exclusive=False, hmax_from_input=False, hmax_unclamped=False,
                  crop_ceil=False, zmid_remainder=True, half_round=True, negate_s=False, invert_apix=False, divide_by_pairs=False,
                  ceil_as_floor_plus_1=False, float64_sum=False, profile_ge=False):
    """oracle.symmetrize.apply_helical_symmetry with its rules exposed; the defaults ARE the oracle (asserted bit for bit).
    ``nudge`` = (k_c, k_s) moves every cos / sin whose angle is not exactly 0 by k ulps.  ``trace`` (a dict) receives the work
    volume's contribution counts ``w``, the z range, every k2 met and the crop."""
    if new_apix is None:
        new_apix = apix
    nz0, ny0, nx0 = data.shape
    if new_size is None:
        new_size = data.shape
    new_size = tuple(int(v) for v in new_size)
    if new_size != data.shape:
        nz1, ny1, nx1 = new_size
        work_shape = (max(nz0, nz1), max(ny0, ny1), max(nx0, nx1))
    else:
        work_shape = (nz0, ny0, nx0)
    sum_dtype = F64 if float64_sum else F32
    data_work = np.zeros(work_shape, dtype=sum_dtype)
    nz, ny, nx = work_shape
    w = np.zeros((nz, ny, nx), dtype=F32)
    hsym_max = int((nz0 if hmax_from_input else nz) * new_apix / rise_angstrom)
    if not hmax_unclamped:
        hsym_max = max(1, hsym_max)
    z0, z1, _ = z_range(data, fraction, zmid_remainder=zmid_remainder, half_round=half_round, ge=profile_ge)
    ratio = (apix, new_apix) if invert_apix else (new_apix, apix)
    jj = ((np.arange(ny) - ny / 2) if y_float_centre else (np.arange(ny) - ny // 2).astype(F64))[:, None]
    ii = ((np.arange(nx) - nx // 2).astype(F64) if x_int_centre else (np.arange(nx) - nx / 2))[None, :]
    k2_met = []
    for hi in range(-hsym_max, hsym_max + 1):
        for k in range(nz):
            k2 = ((k - nz // 2) * new_apix + hi * rise_angstrom) / apix + nz0 // 2
            k2_met.append(k2)
            if (k2 <= z0 if z0_exclusive else k2 < z0) or (k2 > z1 if z1_inclusive else k2 >= z1):
                continue
            kf = int(np.floor(k2))
            kc = kf + 1 if ceil_as_floor_plus_1 else int(np.ceil(k2))
            wk = k2 - kf
            for ci in range(csym):
                rot = np.deg2rad(twist_degree * hi + 360 * ci / csym)
                c, s = np.cos(rot), np.sin(rot)
                if nudge is not None and rot != 0.0:
                    for _ in range(abs(nudge[0])):
                        c = np.nextafter(c, np.inf * nudge[0])
                    for _ in range(abs(nudge[1])):
                        s = np.nextafter(s, np.inf * nudge[1])
                if negate_s:
                    s = -s
                j2 = (c * jj + s * ii) * ratio[0] / ratio[1] + ny0 // 2
                i2 = (-s * jj + c * ii) * ratio[0] / ratio[1] + nx0 // 2
                jf, i_f = np.floor(j2).astype(np.int64), np.floor(i2).astype(np.int64)
                jc, i_c = (jf + 1, i_f + 1) if ceil_as_floor_plus_1 else (np.ceil(j2).astype(np.int64), np.ceil(i2).astype(np.int64))
                ok = (jf >= 0) & (jf < ny0 - 1) & (i_f >= 0) & (i_f < nx0 - 1)
                if not ok.any():
                    continue
                jf, jc, i_f, i_c = jf[ok], jc[ok], i_f[ok], i_c[ok]
                wj, wi = j2[ok] - jf, i2[ok] - i_f
                d0, d1 = data[kf], data[kc]
                val = ((1 - wk) * (1 - wj) * (1 - wi) * d0[jf, i_f]
                       + (1 - wk) * (1 - wj) * wi * d0[jf, i_c]
                       + (1 - wk) * wj * (1 - wi) * d0[jc, i_f]
                       + (1 - wk) * wj * wi * d0[jc, i_c]
                       + wk * (1 - wj) * (1 - wi) * d1[jf, i_f]
                       + wk * (1 - wj) * wi * d1[jf, i_c]
                       + wk * wj * (1 - wi) * d1[jc, i_f]
                       + wk * wj * wi * d1[jc, i_c])
                plane = data_work[k]
                plane[ok] = (plane[ok].astype(F64) + val).astype(sum_dtype)
                w[k][ok] += F32(1.0)
    mask = w > 0
    if divide_by_pairs:
        data_work = (data_work / F32((2 * hsym_max + 1) * csym)).astype(sum_dtype)
    else:
        data_work = np.where(mask, data_work / np.where(mask, w, 1), data_work)
    crop = tuple(slice(0, n) for n in work_shape)
    if data_work.shape != new_size:
        crop = tuple(slice(n // 2 - n1 // 2, n // 2 + ((n1 - n1 // 2) if crop_ceil else n1 // 2)) for n, n1 in zip(work_shape, new_size))
        data_work = data_work[crop]
    if trace is not None:
        trace.update(w=w, z0=int(z0), z1=int(z1), k2=np.array(k2_met), crop=crop, hmax=hsym_max, work_shape=work_shape)
    return data_work.astype(F32)


# ------------------------------------------------------------------------------------------------- projections, restated
def amyloid_slab(nz, apix):
    """utils.py:340-343 as Python's slice resolves it: map3d[z0 : z0 + nz_center] -> [begin, end)."""
    nz_center = int(round(4.75 / apix))
    z0 = nz // 2 - nz_center // 2
    picked = np.arange(nz)[z0:z0 + nz_center]
    return (int(picked[0]), int(picked[-1]) + 1) if picked.size else (min(max(z0, 0), nz),) * 2


def probe_slab(probe, nz):
    a = probe.args
    if "slab" in a:
        return tuple(a["slab"])
    return amyloid_slab(nz, a["apix"]) if a.get("is_amyloid") else (0, nz)


def projections_numpy(vol, slab, *, slab_late=False, swap_xy=False, lanes=None, drop_tail_rows=False, float32_sum=False):
    """[sum(axis=2), sum(axis=1), sum(axis=0) over the slab] in float64, returned in the input's type (float64 for integers).
    ``lanes``: only x < lanes enters the sums along x; ``drop_tail_rows``: rows past the last multiple of 4 never get their sum."""
    d = np.asarray(vol)
    out_t = d.dtype if d.dtype == F32 else F64
    v = d.astype(F32 if float32_sum else F64)
    nz, ny, nx = v.shape
    total = (lambda a, axis: np.cumsum(a, axis=axis, dtype=F32).take(-1, axis=axis)) if float32_sum else (lambda a, axis: a.sum(axis=axis))
    px = total(v[:, :, :lanes], 2)
    if drop_tail_rows:
        px[:, ny - ny % 4:] = 0.0
    py = total(v, 1)
    b, e = (min(slab[0] + 1, nz), min(slab[1] + 1, nz)) if slab_late else slab
    pz = total(v[b:e], 0) if e > b else np.zeros((ny, nx))
    out = [px, py, pz]
    if swap_xy:
        out = [py, px, pz]
    return [np.ascontiguousarray(p).astype(out_t) for p in out]


# ------------------------------------------------------------------------------------------------ transform_map probes
TM_SIDES = ((1, 5, 7), (5, 1, 7), (5, 7, 1), (2, 3, 4), (3, 3, 3), (5, 7, 11))
TM_SEAMS = ((4, 8, 16), (4, 3, 43), (3, 1, 127), (16, 8, 4), (43, 3, 4), (1, 127, 3), (8, 4, 16), (43, 4, 3), (127, 3, 1),   # 127 / 128 / 129 lines on each axis
            (4, 8, 8), (3, 5, 17), (1, 1, 257))                                                      # 256, 255, 257 voxels
_K = "k_map_cubic"
_P = "k_spline_prefilter"


def _tm_transforms(shape):
    """(tag, rule, args) for a shape; an axis of side 1 keeps only the transforms that leave its coordinate exactly 0."""
    nz, ny, nx = shape
    out = []

    def add(tag, rule, **a):
        out.append((tag, rule, a))

    fixed = {"z": nz == 1, "y": ny == 1, "x": nx == 1}
    for ax, n in (("x", nx), ("y", ny), ("z", nz)):
        if fixed[ax]:
            continue
        for sh in sorted({1, -1, n // 2, -(n - 1 - n // 2)} - {0}):
            add(f"d{ax}{sh}", f"{_K}: identity, integer d{ax}: samples exactly on 0 and n - 1 are inside (<=), w3 = 0", **{"d" + ax: sh})
        add(f"d{ax}0.5", f"{_K}: half-integer d{ax}: y = 0.5, every weight live, the first and last cell mirrored", **{"d" + ax: 0.5})
        add(f"d{ax}-1.5", f"{_K}: half-integer d{ax} the other way", **{"d" + ax: -1.5})
    add("scale0.5", f"{_K}: scale 0.5 alone (exact): the offset is not scaled", scale=0.5)
    add("scale2", f"{_K}: scale 2 alone (exact): most samples outside, the border met exactly", scale=2.0)
    half = {("d" + ax): 0.5 for ax in "xyz" if not fixed[ax]}
    if not (fixed["x"] or fixed["y"]):
        for tag, a in (("rot90", dict(rot=90)), ("rot180", dict(rot=180)), ("rot-90", dict(rot=-90)), ("psi90", dict(psi=90)), ("psi180", dict(psi=180))):
            add(tag, f"{_K}: quarter / half turn about z on a non-cubic volume, half-integer shifts", **a, **half)
        add("rot37", f"{_K}: rot alone (equals psi alone: Rz Ry(0) Rz)", rot=37.0, dx=0.25)
        add("psi37", f"{_K}: psi alone (equals rot alone)", psi=37.0, dx=0.25)
    if not (fixed["x"] or fixed["z"]):
        for tag, a in (("tilt90", dict(tilt=90)), ("tilt180", dict(tilt=180))):
            add(tag, f"{_K}: quarter / half turn about y on a non-cubic volume, half-integer shifts", **a, **half)
        add("tilt25", f"{_K}: tilt alone", tilt=25.0, dz=-0.25)
    if not any(fixed.values()):
        add("euler", f"{_K}: rot, tilt, psi all non-zero: Rz(rot) Ry(tilt) Rz(psi), not its reverse", rot=31.0, tilt=47.0, psi=-23.0, dx=0.3, dy=-0.2, dz=0.1)
        add("rot_tilt", f"{_K}: rot then tilt (against tilt then psi)", rot=37.0, tilt=25.0)
        add("tilt_psi", f"{_K}: tilt then psi (against rot then tilt)", tilt=25.0, psi=37.0)
        add("scale0.9_euler", f"{_K}: scale 0.9 with a rotation and a shift", scale=0.9, rot=30.0, tilt=20.0, psi=-40.0, dx=0.5, dy=0.25, dz=-0.75)
    return out


def _transform_probes():
    out = []

    def add(tag, rule, shape, args, dtype=F32, step=False):
        name = f"transform_map/{tag}/{_sname(shape)}/{_tname(dtype)}"
        make = (lambda: dict(vol=_step(shape, dtype))) if step else (lambda: dict(vol=(0.25 + _unit(name, shape)).astype(dtype)))
        full = dict(scale=1.0, rot=0, tilt=0, psi=0, dx=0, dy=0, dz=0)
        full.update(args)
        out.append(Probe(name, "transform_map", rule, make, full))

    for shape in TM_SIDES:
        for tag, rule, a in _tm_transforms(shape):
            add(tag, rule, shape, a)
    for shape in TM_SEAMS:
        seam = f"{_P}: line counts {[int(np.prod(shape)) // n for n in shape]} about the 128-lane workgroup, {int(np.prod(shape))} voxels about 256"
        add("seam_shift", seam, shape, {("d" + ax): 0.5 for ax, n in zip("zyx", shape) if n > 1})
        if min(shape) > 1:
            add("seam_euler", seam, shape, dict(rot=31.0, tilt=47.0, psi=-23.0, dx=0.3, dy=-0.2, dz=0.1))
    for shape in ((5, 7, 11), (2, 3, 4), (6, 10, 8)):
        add("step_half", f"{_P}: a step edge, the overshoot in the compared range", shape, dict(dx=0.5, dy=0.5, dz=0.5), step=True)
        add("step_euler", f"{_P}: a step edge under a general rotation", shape, dict(rot=31.0, tilt=47.0, psi=-23.0), step=True)
    for shape in ((6, 10, 8), (7, 9, 13)):                                   # an even volume, and three distinct odd sides
        for tag, rule, a in _tm_transforms(shape):
            if tag.startswith(("euler", "rot", "tilt", "psi", "scale", "dx1", "dy-1", "dz0.5")):
                add(tag, rule, shape, a)
    for dtype in (F64, np.int16):                                            # the wrapper's dtype rule: float64 out
        for tag, a in (("dx1", dict(dx=1)), ("euler", dict(rot=31.0, tilt=47.0, psi=-23.0, dx=0.3, dy=-0.2, dz=0.1))):
            name = f"transform_map/{tag}/5x7x11/{_tname(dtype)}"
            make = (lambda name=name, dtype=dtype: dict(vol=np.floor(1.0 + 200.0 * _unit(name, (5, 7, 11))).astype(dtype)))
            full = dict(scale=1.0, rot=0, tilt=0, psi=0, dx=0, dy=0, dz=0)
            full.update(a)
            out.append(Probe(name, "transform_map", "transform_map wrapper: float64 result for float64 and integer input", make, full))
    return out


# ------------------------------------------------------------------------------------------------------ helical probes
_H = "k_apply_helical_symmetry"
_HP = "hh_apply_helical_symmetry plan"
H_APIX = 1.5


def _helical_probes():
    out = []

    def add(tag, rule, shape, *, twist=31.7, rise=2.6, csym=1, fraction=1.0, new_size=None, ratio=1.0, profile="dense", dtype=F32):
        """``rise`` and ``new_apix`` (= ratio * apix) are given in units of apix."""
        name = f"helical/{tag}/{_sname(shape)}"

        def make():
            v = _unit(name, shape)
            nz = shape[0]
            if profile == "zero_ends":
                v[:2] = 0
                v[nz - 3:] = 0
            elif profile == "zero_low":
                v[:2] = 0
            elif profile == "zero_high":
                v[nz - 1:] = 0
            elif profile == "one_percent":        # the peak slice sums to exactly 100, slice 1 to exactly 1: not above 1 %
                v[0] = 0
                v[1] = 0
                v[1, 2:4, 2:4] = 0.25
                v[5] = 0
                v[5, :10, :10] = 1.0
            elif profile == "single":
                v[:nz // 2] = 0
                v[nz // 2 + 1:] = 0
            return dict(vol=v.astype(dtype))

        out.append(Probe(name, "helical", rule, make, dict(apix=H_APIX, twist=twist, rise=rise * H_APIX, csym=csym, fraction=fraction,
                                                           new_size=tuple(new_size) if new_size is not None else None, new_apix=ratio * H_APIX)))

    for pz in (0, 1):
        for py in (0, 1):
            for px in (0, 1):
                shape = (12 + pz, 10 + py, 12 + px)
                rule = f"{_H}: parities of (nz0, ny0, nx0): float centre i - nx / 2 for x, integer centre j - ny // 2 for y"
                add(f"parity_c1_{pz}{py}{px}", rule, shape)
                add(f"parity_c3_{pz}{py}{px}", rule, shape, csym=3, twist=-17.3)
                add(f"parity_fine_{pz}{py}{px}", rule + ", new_apix < apix", shape, ratio=0.8)
    base = (12, 11, 13)
    sizes = [("equal", base), ("larger_odd", (15, 13, 17)), ("larger_even", (14, 14, 16)), ("smaller_odd", (9, 7, 11)), ("smaller_even", (10, 8, 10)),
             ("mixed_a", (14, 9, 13)), ("mixed_b", (10, 13, 13)), ("mixed_c", (12, 15, 9)), ("mixed_d", (13, 11, 16)), ("mixed_e", (7, 11, 14)),
             ("one_axis", (12, 11, 9)), ("tiny", (2, 3, 3)),
             ("side1_z", (1, 9, 11)), ("side1_y", (12, 1, 13))]         # n1 // 2 = 0: an empty output, as the reference's slice gives
    for tag, ns in sizes:
        for ratio in (0.8, 1.0, 1.25):
            add(f"size_{tag}_r{ratio}", f"{_HP}: work volume = max(input, requested), crop n // 2 - n1 // 2 : n // 2 + n1 // 2 (an odd side loses one), "
                f"new_apix / apix = {ratio}", base, new_size=ns, ratio=ratio)
        add(f"size_{tag}_even_in", f"{_HP}: the same request on an all-even input", (12, 10, 12), new_size=ns, csym=3)
    for shape in ((12, 11, 13), (13, 10, 12)):
        add("rise2", f"{_H}: rise = 2 apix, k2 integer: k2 == z0 is inside (<), k2 == z1 is outside (>=), kf == kc", shape, rise=2.0)
        add("rise2_c3", f"{_H}: integer k2 with Csym 3", shape, rise=2.0, csym=3, twist=41.0)
        add("rise3_fine", f"{_H}: rise = 3 apix with new_apix = apix / 2: k2 on integers and halves", shape, rise=3.0, ratio=0.5)
        add("rise_general", f"{_H}: a general rise", shape, rise=3.37)
        for profile, what in (("zero_ends", "zero slabs at both ends"), ("zero_low", "a zero slab at the low end: z0 + z1 odd"), ("zero_high", "a zero slice at the high end")):
            add(f"profile_{profile}", f"{_HP}: 1 % profile, {what}", shape, profile=profile)
            add(f"profile_{profile}_rise2", f"{_HP}: 1 % profile, {what}; integer k2 meets the narrowed z0 and z1", shape, profile=profile, rise=2.0)
            add(f"profile_{profile}_f0.5", f"{_HP}: {what}, fraction 0.5: zmid = (z0 + z1) // 2 + (z0 + z1) % 2", shape, profile=profile, fraction=0.5, rise=2.0)
        add("profile_single", f"{_HP}: a single dense slice: z0 == z1, empty range, all-zero output", shape, profile="single")
        for fr in (1.0, 0.5, 0.625, 0.58, 0.3, 0.05):
            add(f"fraction{fr}", f"{_HP}: half = int(nz0 fraction + 0.5) // 2 (0.625, 0.58 and 0.3 cross an integer; 0.05 empties the range)", shape, fraction=fr, rise=2.0)
            add(f"fraction{fr}_general", f"{_HP}: fraction {fr} with a general rise", shape, fraction=fr)
    add("profile_one_percent", f"{_HP}: a slice whose sum is exactly 1 % of the peak (1 against 100) is excluded (>)", (12, 10, 12), profile="one_percent", rise=2.0)
    add("profile_one_percent_general", f"{_HP}: the exactly-1 % slice with a general rise", (12, 10, 12), profile="one_percent")
    for shape, ns in (((12, 11, 13), None), ((12, 11, 13), (16, 11, 13)), ((13, 10, 12), (9, 10, 12))):
        tag = "same" if ns is None else _sname(ns)
        add(f"hmax1_{tag}", f"{_HP}: hmax = max(1, int(nz new_apix / rise)) clamped to 1, hi = +-1 still reach the map", shape,
            rise=0.5 * max(shape[0], ns[0] if ns else 0) + 1.0, ratio=0.5, new_size=ns)
        add(f"hmax1_far_{tag}", f"{_HP}: hmax clamped to 1, rise beyond the map", shape, rise=17.0, new_size=ns)
        add(f"hmax8_{tag}", f"{_HP}: hmax about 8, from the WORK volume's nz", shape, rise=1.55, new_size=ns)
        add(f"hmax_edge_{tag}", f"{_HP}: nz new_apix / rise a whole number (int of an exact quotient)", shape, rise=2.0 if ns is None else max(shape[0], ns[0]) / 4.0, new_size=ns)
    # exact landings: quarter and half turns.  The output is cropped inside the input, so no landing meets the input's border
    for csym in (1, 2, 4):
        for twist in (0.0, 90.0, 180.0):
            for shape, ns in (((12, 12, 14), (12, 8, 8)), ((13, 13, 15), (13, 9, 9)), ((12, 15, 13), (10, 9, 7))):
                for ratio in (1.0, 0.5):
                    add(f"landing_c{csym}_t{twist:g}_r{ratio}_{_sname(ns)}", f"{_H}: Csym {csym}, twist {twist:g}: samples on exact quarter turns (wj, wi of 0 and 0.5)",
                        shape, csym=csym, twist=twist, rise=2.0, new_size=ns, ratio=ratio)
    for csym, twist in ((3, 27.3), (3, -27.3), (5, 11.9), (5, -48.1), (6, 63.7), (6, -3.3)):
        for shape in ((12, 11, 13), (13, 12, 12)):    # (an even Csym holds an exact half turn: cropped inside the input like the landings)
            add(f"general_c{csym}_t{twist:g}", f"{_H}: Csym {csym} with a general twist of either sign: s enters j2 with +, i2 with -", shape, csym=csym, twist=twist,
                new_size=None if csym % 2 else (shape[0], shape[1] - 4, shape[2] - 4))
    for dtype in (F64, np.int16):
        name = f"helical/dtype_{_tname(dtype)}/12x11x13"
        out.append(Probe(name, "helical", "apply_helical_symmetry wrapper: float32 result whatever the input type",
                         (lambda name=name, dtype=dtype: dict(vol=(_unit(name, (12, 11, 13)) > 0.5).astype(dtype) if dtype != F64 else _unit(name, (12, 11, 13), F64))),
                         dict(apix=H_APIX, twist=31.7, rise=2.6 * H_APIX, csym=2, fraction=1.0, new_size=(14, 9, 13), new_apix=H_APIX)))
    return out


# -------------------------------------------------------------------------------------------------- projection probes
_PS, _PC = "k_map_proj_slices", "k_map_proj_columns"


def _projection_probes():
    out = []

    def add(tag, rule, shape, dtype=F32, **args):
        name = f"projections/{tag}/{_sname(shape)}/{_tname(dtype)}"
        out.append(Probe(name, "projections", rule, lambda: dict(vol=_unit(name, shape, dtype)), args))

    for ny in (1, 3, 4, 5):
        for nx in (1, 63, 64, 65, 255, 256, 257):
            add("thin", f"{_PS}: ny about the 4 wavefronts, nx about the 64 lanes and the 256 threads; non-square outputs", (2, ny, nx))
    for shape in ((1, 5, 7), (1, 1, 1), (1, 4, 257), (3, 6, 70), (2, 9, 130)):
        add("nz1" if shape[0] == 1 else "wide", f"{_PS} / {_PC}: nz = 1, and rows that wrap the wavefronts more than once", shape)
    for shape in ((2, 5, 65), (3, 4, 257)):
        add("f64", "generate_xyz_projections wrapper: float64 results for float64 input", shape, dtype=F64)
    for nz in (6, 7):
        shape = (nz, 5, 9)
        for tag, apix in (("one", 4.75), ("nz", 4.75 / nz), ("beyond", 0.5), ("far_beyond", 0.2), ("two", 2.4), ("none", 10.0)):
            add(f"amyloid_{tag}", f"{_PC} / _amyloid_slab: nz_center = round(4.75 / apix) of 1, nz, beyond nz (a negative start, as Python resolves it), 0",
                shape, is_amyloid=True, apix=apix)
    for nz in (6, 1):
        shape = (nz, 5, 9)
        for slab in sorted({(0, 0), (nz // 2, nz // 2), (nz, nz), (0, nz), (nz - 1, nz), (0, 1), (1, max(nz - 2, 1))}):
            add(f"slab_{slab[0]}_{slab[1]}", f"{_PC}: hh_map_projections slab [begin, end): begin == end gives zeros, [0, nz) the whole sum", shape, slab=slab)
    add("slab_1_2", f"{_PC}: a slab across more than one 256-thread block of columns", (3, 5, 65), slab=(1, 2))
    return out


# -------------------------------------------------------------------------------------------------- symmetrize probes
def _symmetrize_probes():
    out = []

    def add(tag, rule, shape, **args):
        name = f"symmetrize/{tag}/{_sname(shape)}"
        a = dict(apix=H_APIX, twist=31.7, rise=2.6 * H_APIX, csym=1, fraction=1.0, new_size=None, new_apix=None, axial_rotation=0, tilt=0)
        a.update(args)
        out.append(Probe(name, "symmetrize", rule, lambda: dict(vol=_unit(name, shape)), a))

    s = (12, 11, 13)
    add("plain", "symmetrize_transform_map: no filter (new_apix None), no rotation", s)
    add("filter", "symmetrize_transform_map: new_apix > apix switches the low pass on", s, new_apix=1.25 * H_APIX)
    add("equal_apix", "symmetrize_transform_map: new_apix == apix is not above: no filter", s, new_apix=H_APIX, axial_rotation=20.0)
    add("finer", "symmetrize_transform_map: new_apix < apix, rotation and tilt", s, new_apix=0.8 * H_APIX, axial_rotation=20.0, tilt=5.0)
    add("filter_mixed", "symmetrize_transform_map: filter, mixed grow / shrink new_size, rotation and tilt", s, new_apix=1.25 * H_APIX, new_size=(14, 9, 13),
        axial_rotation=-35.0, tilt=7.0, csym=3)
    add("tilt_only", "symmetrize_transform_map: tilt without axial rotation on an even volume", (12, 10, 12), tilt=9.0, new_size=(10, 12, 12))
    add("rotation_only_filter", "symmetrize_transform_map: filter and axial rotation, shrinking", (13, 12, 12), new_apix=1.5 * H_APIX, new_size=(9, 8, 10), axial_rotation=35.0)
    return out


# ------------------------------------------------------------------------------------------------------------ the table
PROBES = tuple(_transform_probes() + _helical_probes() + _projection_probes() + _symmetrize_probes())
BY_NAME = {p.name: p for p in PROBES}
assert len(BY_NAME) == len(PROBES), [p.name for p in PROBES if sum(q.name == p.name for q in PROBES) > 1]


def _helical_args(a):
    return (a["apix"], a["twist"], a["rise"], a["csym"], a["fraction"], a["new_size"], a["new_apix"])


def reference(probe, inp=None):
    inp = probe.inputs() if inp is None else inp
    a, vol = probe.args, inp["vol"]
    if probe.kind == "transform_map":
        return S.transform_map(vol, **a)
    if probe.kind == "helical":
        return S.apply_helical_symmetry(vol, *_helical_args(a))
    if probe.kind == "symmetrize":
        na = a["new_apix"]
        work = np_filter_3d(vol, a["apix"] / na).astype(F32) if na is not None and na > a["apix"] else vol
        m = S.apply_helical_symmetry(work, *_helical_args(a))
        if a["axial_rotation"] or a["tilt"]:
            m = S.transform_map(m, rot=a["axial_rotation"], tilt=a["tilt"])
        return m
    if probe.kind == "projections":
        return projections_numpy(vol, probe_slab(probe, vol.shape[0]))
    raise KeyError(probe.kind)


# ---------------------------------------------------------------------------------------------------------- the comparison
@dataclass
class Verdict:
    figure: float          # the largest difference of a compared number
    bound: float           # what the figure is held to (0: exact)
    mismatches: int        # exactly compared items that differ (shape, dtype, zero pattern, an empty slab's zeros)
    ok: bool
    note: str = ""

    def bitten(self):
        """What the host test asks of a wrong-rule variant: an exact item changed, or a number moved by 100 bounds."""
        return self.mismatches > 0 or (self.bound > 0 and self.figure >= 100.0 * self.bound)


def _values(got, want, bound, zero_pattern=False):
    g, w = np.asarray(got), np.asarray(want)
    if g.shape != w.shape or g.dtype != w.dtype:
        return Verdict(np.inf, bound, 1, False, f"shape / dtype {g.shape} {g.dtype} != {w.shape} {w.dtype}")
    bad = int((~np.isfinite(g)).sum())
    if zero_pattern:
        bad += int(((g == 0) != (w == 0)).sum())
    fig = float(np.abs(g.astype(F64) - w.astype(F64)).max()) if g.size else 0.0
    if not np.isfinite(fig):
        fig = np.inf
    return Verdict(fig, bound, bad, bad == 0 and fig <= bound)


def compare(probe, got, want, inp=None):
    k = probe.kind
    if k == "transform_map":
        return _values(got, want, BOUND_TRANSFORM * float(np.abs(want).max()), zero_pattern=True)
    if k == "helical":
        return _values(got, want, BOUND_HELICAL)
    if k == "symmetrize":
        return _values(got, want, BOUND_SYMMETRIZE * float(np.abs(want).max()))
    if k == "projections":
        if len(got) != 3:
            return Verdict(np.inf, BOUND_PROJ, 1, False, "three projections expected")
        worst = Verdict(0.0, BOUND_PROJ, 0, True)
        for g, w in zip(got, want):
            scale = float(np.abs(w).max()) if np.asarray(w).size else 0.0
            v = _values(g, w, BOUND_PROJ * scale)
            worst.mismatches += v.mismatches
            if scale == 0.0:                                        # an empty slab (or an all-zero sum): exact
                worst.mismatches += int(np.count_nonzero(np.asarray(g))) if v.mismatches == 0 else 0
            elif v.mismatches == 0:
                worst.figure = max(worst.figure, v.figure / scale)  # in units of the projection's own max |want|
        worst.ok = worst.mismatches == 0 and worst.figure <= worst.bound
        worst.note = "figure in units of max |want| of its projection"
        return worst
    raise KeyError(k)


# ------------------------------------------------------------------------------------------------- the wrong-rule variants
@dataclass(frozen=True)
class Variant:
    rule: str          # the one rule changed
    run: object        # (probe, inputs) -> what the device would return under the wrong rule
    probes: tuple      # the probes listed for it: at least one must be bitten


def _tm(**kw):
    return lambda probe, inp: transform_map_numpy(inp["vol"], **probe.args, **kw)


def _hl(**kw):
    return lambda probe, inp: helical_numpy(inp["vol"], *_helical_args(probe.args), **kw)


def _pj(**kw):
    return lambda probe, inp: projections_numpy(inp["vol"], probe_slab(probe, inp["vol"].shape[0]), **kw)


def _names(prefix, *contains):
    return tuple(p.name for p in PROBES if p.name.startswith(prefix) and all(c in p.name for c in contains))


_T, _HN, _PN = "transform_map/", "helical/", "projections/"
_BORDER = tuple(n for n in _names(_T) if n.split("/")[1] in ("dx1", "dx-1", "dy1", "dy-1", "dz1", "dz-1"))
VARIANTS = {
    "transform_map: prefilter skipped on axis 0": Variant(f"{_P} on z", _tm(skip_axis=0), _names(_T, "/5x7x11/") + _names(_T + "seam")),
    "transform_map: prefilter skipped on axis 1": Variant(f"{_P} on y", _tm(skip_axis=1), _names(_T, "/5x7x11/") + _names(_T + "seam")),
    "transform_map: prefilter skipped on axis 2": Variant(f"{_P} on x", _tm(skip_axis=2), _names(_T, "/5x7x11/") + _names(_T + "seam")),
    "transform_map: axis-1 lines walked with axis-2's stride": Variant(f"{_P} stride", _tm(stride_mixup=True), _names(_T, "/5x7x11/") + _names(_T, "/7x9x13/")),
    "transform_map: border test exclusive": Variant(f"{_K}: c <= n - 1", _tm(exclusive=True), _BORDER),
    "transform_map: taps clamped instead of mirrored": Variant(f"{_K} / spline_mirror", _tm(clamp=True), _names(_T + "dx0.5/") + _BORDER),
    "transform_map: centre n / 2.0": Variant(f"{_K}: i - nx / 2 in integers", _tm(float_centre=True), _names(_T, "/5x7x11/") + _names(_T, "/7x9x13/")),
    "transform_map: +dx instead of -dx": Variant("hh_transform_map: ox = nx // 2 - dx", _tm(plus_shift=True), _names(_T + "dx") + _names(_T + "dy") + _names(_T + "dz")),
    "transform_map: Euler order reversed": Variant("hh_transform_map: Rz(rot) Ry(tilt) Rz(psi)", _tm(reverse_euler=True),
                                                   _names(_T + "euler/") + _names(_T + "rot_tilt/") + _names(_T + "tilt_psi/")),
    "transform_map: the offset scaled too": Variant(f"{_K}: scale multiplies the grid, not the offset", _tm(scale_offset=True), _names(_T + "scale")),
    "helical: integer centre for x": Variant(f"{_H}: ii = i - nx / 2.0", _hl(x_int_centre=True), _names(_HN + "parity_")),
    "helical: float centre for y": Variant(f"{_H}: jj = j - ny // 2", _hl(y_float_centre=True), _names(_HN + "parity_")),
    "helical: k2 > z1 for >=": Variant(f"{_H}: k2 >= z1 is outside", _hl(z1_inclusive=True), _names(_HN + "rise2")),
    "helical: k2 <= z0 for <": Variant(f"{_H}: k2 < z0 is outside", _hl(z0_exclusive=True), _names(_HN + "rise2")),
    "helical: hmax from the input's nz0": Variant(f"{_HP}: hmax from the work volume", _hl(hmax_from_input=True), _names(_HN + "hmax")),
    "helical: hmax without max(1, .)": Variant(f"{_HP}: max(1, .)", _hl(hmax_unclamped=True), _names(_HN + "hmax1_")),
    "helical: crop taking n1 - n1 // 2 above the centre": Variant(f"{_HP}: crop", _hl(crop_ceil=True), _names(_HN + "size_")),
    "helical: zmid without the remainder": Variant(f"{_HP}: zmid", _hl(zmid_remainder=False), _names(_HN + "profile_")),
    "helical: half without + 0.5": Variant(f"{_HP}: half", _hl(half_round=False), _names(_HN + "fraction")),
    "helical: profile >= threshold": Variant(f"{_HP}: a slice at exactly 1 % is not above it", _hl(profile_ge=True), _names(_HN + "profile_one_percent")),
    "helical: s negated": Variant(f"{_H}: j2 = c jj + s ii, i2 = -s jj + c ii", _hl(negate_s=True), _names(_HN + "general_") + _names(_HN + "parity_")),
    "helical: new_apix / apix inverted": Variant(f"{_H}: new_apix / apix", _hl(invert_apix=True), _names(_HN + "size_", "_r0.8") + _names(_HN + "size_", "_r1.25")),
    "helical: division by the number of (hi, ci) pairs": Variant(f"{_H}: acc / cnt", _hl(divide_by_pairs=True), _names(_HN + "parity_") + _names(_HN + "hmax")),
    "projections: slab one slice late": Variant(f"{_PC}: [z_begin, z_end)", _pj(slab_late=True), _names(_PN + "amyloid_") + _names(_PN + "slab_")),
    "projections: x and y sums swapped": Variant(f"{_PS}: out_x, out_y", _pj(swap_xy=True), _names(_PN + "thin/")),
    "projections: lanes >= 64 dropped": Variant(f"{_PS}: x += 64", _pj(lanes=64), _names(_PN + "thin/")),
    "projections: rows ny % 4 dropped": Variant(f"{_PS}: y += 4", _pj(drop_tail_rows=True), _names(_PN + "thin/")),
}
# what arithmetic keeps from biting (asserted as such by the host test)
UNBITABLE = {
    "transform_map: w3 formed directly": Variant(f"{_K}: w3 = 1 - w0 - w1 - w2", _tm(w3_direct=True), _names(_T)),
    "helical: floor + 1 for ceil": Variant(f"{_H}: kc, jc, ic by ceil", _hl(ceil_as_floor_plus_1=True), _names(_HN)),
    "helical: a float64 running sum": Variant(f"{_H}: acc rounded to float32 after every term", _hl(float64_sum=True), _names(_HN)),
    "projections: a float32 running sum": Variant(f"{_PS} / {_PC}: float64 running sums", _pj(float32_sum=True), _names(_PN)),
}
