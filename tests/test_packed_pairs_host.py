"""One row transform for the two runs of a pair (k_fused_pass's packed pair walk): the identity it rests on, and its gate.

The identity, in NumPy float64 on the oracle's images: with one unit at azimuth 0, rot 0 and no tilt, psi or dy the lattice is
centrosymmetric about the pixel (N/2, N/2), so a row of the column-transformed image is Hermitian about column N/2 but for
column 0, whose mirror would be column N.  Its transform is then real up to the constant Im H[ky][0], and two such rows A, B
go through one transform: C = FFT_x(z), z = A + i B with the imaginary parts of column 0 taken out,
|F_A|^2 = Re(C)^2 + Im(A[0])^2, |F_B|^2 = Im(C)^2 + Im(B[0])^2.  Bounds: amplitudes reach 1e3 and a 128-point float64
transform loses a few 1e-16 of that per stage, so 1e-11 holds the identity where it holds at all; where it does not (rot 7.5,
or column 0 left in) the error is of the order of the amplitudes themselves.

The gate (`hh_lattice_centrosymmetric`, sweep_plan.h) is host arithmetic: it runs without a device.
"""
import ctypes as C

import numpy as np
import pytest

from helicon_amd import _lib
from oracle import path_b as O

N = 128
TRUTH_A, TRUTH_B = (1.20, 4.75), (1.21, 4.755)


def rows_of(csym, rot):
    """Rows ky = 1 ... N/2 - 1 of the column transform of the two images (ky = 0 and N/2 are the kernel's packed row, which
    keeps its two transforms)."""
    imgs = [O.simulate_helical_projection(1, tw, rs, csym, 0.4 * N, 2.0, 0, 0, N, N, 1.0, rot=rot) for tw, rs in (TRUTH_A, TRUTH_B)]
    return [np.fft.fft(img, axis=0)[1:N // 2] for img in imgs]


def packed_amplitudes(ha, hb, column_0=True):
    z = ha + 1j * hb
    ima, imb = ha[:, 0].imag, hb[:, 0].imag
    z[:, 0] = ha[:, 0].real + 1j * hb[:, 0].real
    if not column_0:
        ima, imb = 0 * ima, 0 * imb
    c = np.fft.fft(z, axis=1)
    return np.sqrt(c.real ** 2 + ima[:, None] ** 2), np.sqrt(c.imag ** 2 + imb[:, None] ** 2)


def worst(ha, hb, **kw):
    pa, pb = packed_amplitudes(ha, hb, **kw)
    return max(np.abs(pa - np.abs(np.fft.fft(ha, axis=1))).max(), np.abs(pb - np.abs(np.fft.fft(hb, axis=1))).max())


@pytest.mark.parametrize("csym", [1, 3])
def test_one_transform_gives_both_rows_amplitudes(csym):
    ha, hb = rows_of(csym, 0.0)
    hermitian = max(np.abs(h[:, 1:][:, ::-1] - np.conj(h[:, 1:])).max() for h in (ha, hb))
    err = worst(ha, hb)
    print(f"csym {csym}: max |H[N/2 - a] - conj H[N/2 + a]| = {hermitian:.2e}, packed against separate amplitudes {err:.2e}")
    assert hermitian < 1e-12 and err < 1e-11


def test_column_0_carries_an_imaginary_part_the_amplitudes_need():
    """Column 0 has no mirror: its imaginary part (3.0 at this size) is taken out of the transform and must come back in
    the amplitudes; dropped, it is the error."""
    ha, hb = rows_of(1, 0.0)
    im0 = max(np.abs(ha[:, 0].imag).max(), np.abs(hb[:, 0].imag).max())
    err = worst(ha, hb, column_0=False)
    print(f"max |Im H[.][0]| = {im0:.3f}, error with the column-0 term dropped = {err:.3f}")
    assert im0 == pytest.approx(3.0, abs=0.05) and err == pytest.approx(im0, rel=0.02)
    assert worst(ha, hb) < 1e-11


def test_rot_breaks_the_identity():
    ha, hb = rows_of(1, 7.5)
    err = worst(ha, hb)
    print(f"rot 7.5: packed against separate amplitudes {err:.1f}")
    assert err > 100.0


# ---------------------------------------------------------------------------- the gate
def gate(params, ny=512, nx=512, units=None, **geom):
    g = _lib.hh_geom(apix=1.0, helical_diameter=0.4 * ny, ball_radius=2.0, tilt=0.0, psi=0.0, dy=0.0, n_units=0, tail_bits=0, units=None)
    for k, v in geom.items():
        setattr(g, k, v)
    keep = None
    if units is not None:
        keep = np.ascontiguousarray(units, dtype=np.float64)
        g.n_units, g.units = len(keep), keep.ctypes.data_as(C.POINTER(C.c_double))
    p = np.ascontiguousarray(params, dtype=np.float64)
    return _lib.lib().hh_lattice_centrosymmetric(C.byref(g), ny, nx, p.ctypes.data_as(C.POINTER(C.c_double)), len(p))


def grid(csyms=(1,)):
    return np.array([(tw, rs, cs, 0.0) for cs in csyms for tw in 2.0 + 0.25 * np.arange(4) for rs in 4.0 + 0.05 * np.arange(16)])


def test_gate_takes_the_default_geometry_with_any_csym():
    assert gate(grid()) == 1
    assert gate(grid((1, 2, 3))) == 1
    assert gate(grid(), units=[(102.4, 0.0, 0.0)]) == 1          # the same unit, given explicitly
    assert gate(grid(), ball_radius=4.0) == 1


def test_gate_refuses_what_breaks_the_symmetry():
    one_rot = grid()
    one_rot[37, 3] = 7.5
    assert gate(one_rot) == 0
    assert gate(grid(), units=[(102.4, 0.0, -3.0), (80.0, 1.0, 4.5)]) == 0      # two units
    assert gate(grid(), units=[(102.4, 0.0, 0.0), (102.4, 0.0, 0.0)]) == 0      # ... whatever they are
    assert gate(grid(), units=[(102.4, 0.0, 4.5)]) == 0                         # z != 0
    assert gate(grid(), units=[(102.4, 1.0, 0.0)]) == 0                         # azimuth != 0
    assert gate(grid(), dy=0.5) == 0
    assert gate(grid(), tilt=3.0) == 0
    assert gate(grid(), psi=-2.0) == 0


def test_gate_refuses_a_lattice_that_reaches_image_row_0():
    """Row 0 has no mirror row.  rpx = 10 at ball radius 2: a ball centred on row 256 - 245 = 11 touches rows 1 ... 21, one
    centred on row 10 touches row 0."""
    assert gate(grid(), helical_diameter=2 * 245.0) == 1
    assert gate(grid(), helical_diameter=2 * 245.5) == 0
    assert gate(grid(), helical_diameter=2 * 246.0) == 0
    assert gate(grid(), helical_diameter=2 * 235.0, ball_radius=4.0) == 1     # rpx = 20
    assert gate(grid(), helical_diameter=2 * 236.0, ball_radius=4.0) == 0


def test_gate_rejects_bad_arguments():
    L = _lib.lib()
    assert L.hh_lattice_centrosymmetric(None, 512, 512, None, 0) == -1
    assert gate(grid()[:0]) == -1
