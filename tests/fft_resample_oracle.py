"""Float64 restatements of the reference's Fourier resampling, independent of helicon_amd.fft_resample's builders: the sums
and ``np.fft`` compositions written out directly.

* ``fft_rescale_3d``   lib/transforms.py:714-743 with finufft's type-2 transform as the direct sum it approximates
                       (``c[k] = sum_m f[m] exp(-i m . x_k)``, modes ``m = index - n // 2``), as oracle/path_b.py does in 2-D;
* ``fft_resample``     plugins/proc3d/fft_resample.py:97-109, ``np.abs`` (the reference) or the real part;
* ``fft_crop``         lib/transforms.py:610-660: the 2-D branch as the reference has it, the 3-D branch with ``irfftn``
                       (the reference's ``irfft2`` there leaves z untransformed: ``fft_crop_3d_as_reference``);
* ``float32_passes``   the three per-axis products in float32 NumPy with the operators rounded to float32: what float32
                       costs the restatement itself (the tolerance rule's floor).  It never sees the device's output.
"""
import numpy as np

CASES = [   # in -> out: the shapes of tests/test_gpu_fft_resample.py, also used for the builders on the host
    ((24, 24, 24), (16, 16, 16)),
    ((20, 20, 20), (30, 30, 30)),
    ((15, 18, 21), (9, 12, 14)),
    ((66, 70, 130), (34, 36, 66)),
    ((40, 40, 40), (72, 40, 40)),
    ((4, 6, 8), (2, 4, 6)),
    ((33, 64, 65), (65, 32, 33)),
]
LONGEST = [((1024, 2, 4), (512, 2, 4)), ((2, 1024, 4), (2, 512, 4)), ((2, 4, 768), (2, 4, 1024))]   # the documented maximum, each axis
CROP_CASES_3D = [((12, 14, 16), (8, 8, 10)), ((13, 15, 17), (7, 9, 8))]
CROP_CASES_2D = [((24, 20), (16, 12)), ((24, 20), (15, 11)), ((21, 17), (10, 8))]


def blob_volume(shape, seed=0):
    """An anisotropic Gaussian blob plus 0.2 sigma seeded noise, float32."""
    rng = np.random.default_rng(seed)
    grids = np.meshgrid(*[np.arange(n, dtype=np.float64) for n in shape], indexing="ij")
    r2 = sum(((g - c * n) / (w * n + 1.0)) ** 2 for g, n, c, w in zip(grids, shape, (0.45, 0.55, 0.4)[-len(shape):], (0.12, 0.2, 0.16)[-len(shape):]))
    blob = np.exp(-0.5 * r2)
    return (blob + 0.2 * blob.std() * rng.standard_normal(shape)).astype(np.float32)


def rescale_cutoffs(shape, size, apix, zoom=0.8):
    """The GPU tests' cutoff_res: 2 apix n / (zoom on) per axis."""
    return tuple(2.0 * apix * n / (zoom * on) for n, on in zip(shape, size))


def _axis_factor(n, on, apix, cutoff):
    """[on, n]: the direct sum's factor along one axis and the reference's (-1)^u."""
    freq = np.fft.fftfreq(on) * 2 * apix / cutoff
    modes = np.arange(n) - n // 2
    checker = np.where(np.arange(on) % 2, -1.0, 1.0)
    return checker[:, None] * np.exp(-2j * np.pi * freq[:, None] * modes[None, :])


def fft_rescale_3d(data, apix=1.0, cutoff_res=None, output_size=None):
    data = np.asarray(data, dtype=np.float64)
    cutoff = cutoff_res if cutoff_res else (2 * apix,) * 3
    size = output_size if output_size else data.shape
    fz, fy, fx = (_axis_factor(n, on, apix, c) for n, on, c in zip(data.shape, size, cutoff))
    return np.einsum("ai,bj,ck,ijk->abc", fz, fy, fx, data.astype(np.complex128), optimize=True)


def fft_resample(data, apix, new_size, output="abs"):
    nz, ny, nx = np.shape(data)
    new_nz, new_ny, new_nx = new_size
    fft = fft_rescale_3d(data, apix=apix, cutoff_res=(2 * apix * nz / new_nz, 2 * apix * ny / new_ny, 2 * apix * nx / new_nx),
                         output_size=(new_nz, new_ny, new_nx))
    inv = np.fft.ifftn(fft)
    out = (np.abs(inv) if output == "abs" else inv.real) * (new_nx * new_ny * new_nz / (nx * ny * nz))
    return out, round(apix * nx / new_nx, 4)


def _truncated_spectrum(data, output_size):
    data = np.asarray(data, dtype=np.float64)
    lead = tuple(range(data.ndim - 1))
    fft = np.fft.fftshift(np.fft.rfftn(data), axes=lead)
    cut = tuple(slice(n // 2 - on // 2, n // 2 + on // 2) for n, on in zip(data.shape[:-1], output_size[:-1]))
    return np.fft.fftshift(fft[cut + (slice(0, output_size[-1] // 2 + 1),)], axes=lead)


def fft_crop(data, output_size=None):
    if output_size is None or tuple(np.shape(data)) == tuple(output_size):
        return data
    assert np.ndim(data) in (2, 3) and np.ndim(data) == len(output_size)
    assert all(on <= n for on, n in zip(output_size, np.shape(data)))
    spec = _truncated_spectrum(data, output_size)
    return np.fft.irfft2(spec) if np.ndim(data) == 2 else np.fft.irfftn(spec)


def fft_crop_3d_as_reference(data, output_size):
    """What the reference's 3-D branch returns: irfft2 of the 3-D truncated spectrum (z is left in Fourier space)."""
    return np.fft.irfft2(_truncated_spectrum(data, output_size))


def float32_passes(data, ops, epilogue, scale=1.0):
    """z, y, x products in float32 NumPy, operators (complex128 [out, in], None: skipped) rounded to float32 once."""
    re, im = np.asarray(data, dtype=np.float32), None
    for ax, op in enumerate(ops):
        if op is None:
            continue
        ar, ai = op.real.astype(np.float32), op.imag.astype(np.float32)
        ap = lambda m, v, ax=ax: np.moveaxis(np.tensordot(m, v, axes=(1, ax)), 0, ax)   # noqa: E731
        if im is None:
            re, im = ap(ar, re), ap(ai, re)
        else:
            re, im = ap(ar, re) - ap(ai, im), ap(ai, re) + ap(ar, im)
        assert re.dtype == np.float32
    if im is None:
        im = np.zeros_like(re)
    if epilogue == "store":
        return re, im
    if epilogue == "abs":
        return np.sqrt(re * re + im * im) * np.float32(scale)
    return re * np.float32(scale)


def resample_ops(shape, size):
    """proc3d's per-axis operators, written from np.fft: ifft along the axis of the direct sum's factor."""
    return [np.fft.ifft(_axis_factor(n, on, 1.0, 2.0 * n / on), axis=0) for n, on in zip(shape, size)]


def rescale_ops(shape, size, apix, cutoff):
    return [_axis_factor(n, on, apix, c) for n, on, c in zip(shape, size, cutoff)]


def crop_ops(shape, size):
    """fft_crop's per-axis operators from np.fft on the identity: fft, keep the bins, inverse of size 2 (on // 2)."""
    ops = []
    for ax, (n, on) in enumerate(zip(shape, size)):
        h = on // 2
        spec = np.fft.fft(np.eye(n), axis=0)                        # [bin, j]
        if ax < len(shape) - 1:
            kept = np.concatenate([spec[:h], spec[n - h:]]) if h else spec[:0]   # bins 0 .. h-1, -h .. -1 in ifft's order
            ops.append(np.fft.ifft(kept, axis=0))
        else:
            w = np.full(h + 1, 2.0)
            w[0] = w[h] = 1.0
            u = np.arange(h + 1)
            inv = np.exp(2j * np.pi * np.outer(np.arange(2 * h), u) / (2 * h)) * (w / (2 * h))
            ops.append(inv @ spec[: h + 1])
    return ops


def tolerance(want, floor_err, label=""):
    """The project's rule for three MFMA passes (tests/test_gpu_map_input.py:89-98): 2e-6 max|want|, raised to 4 x the host
    float32 floor (and the floor printed) where the floor exceeds a quarter of it."""
    peak = float(np.abs(want).max())
    atol = 2e-6 * peak
    if floor_err > atol / 4:
        print(f"{label}: float32 floor of the restatement {floor_err / peak:.2e} max|want| exceeds a quarter of 2e-6")
        atol = 4 * floor_err
    return atol
