"""The app's 3-D map input on the device: the 3-D Gaussian filter (hh_low_high_pass_filter_3d), symmetrize_transform_map,
generate_xyz_projections (hh_map_projections) and denovo3DBatch --from-map (webApps/denovo3D/utils.py:336-383,
app.py:1780-1829)."""
import argparse
import json

import numpy as np
import pytest

import helicon_amd as H
from helicon_amd import denovo3DBatch as B

pytestmark = pytest.mark.gpu


def np_filter_3d(data, low_pass_fraction=0, high_pass_fraction=0):
    """lib/filters.py:349-372 restated: Re ifftn(fftn(x) * fftshift(filter)) on the centred float32 grid."""
    fft = np.fft.fftn(data)
    nz, ny, nx = fft.shape
    Z, Y, X = np.meshgrid(np.arange(nz, dtype=np.float32) - nz // 2, np.arange(ny, dtype=np.float32) - ny // 2,
                          np.arange(nx, dtype=np.float32) - nx // 2, indexing="ij")
    Z /= nz // 2
    Y /= ny // 2
    X /= nx // 2
    R2 = X**2 + Y**2 + Z**2
    if 0 < low_pass_fraction < 1:
        fft *= np.fft.fftshift(np.exp(-np.log(2) / low_pass_fraction**2 * R2))
    if 0 < high_pass_fraction < 1:
        fft *= np.fft.fftshift(1.0 - np.exp(-np.log(2) / high_pass_fraction**2 * R2))
    return np.real(np.fft.ifftn(fft))


FRACTIONS = [(0.3, 0), (0, 0.2), (0.5, 0.1), (0, 0), (1.5, -0.5)]   # low only, high only, both, neither, out of range


def circulant_f32_filter_3d(data, low_pass_fraction=0, high_pass_fraction=0):
    """The same filter as three 1-D circulant products per Gaussian term (C = F^-1 diag(w) F along each axis, the high
    pass as a difference of two Gaussians), the operators and the products in float32 NumPy: what float32 costs the
    reference itself.  It never looks at the device's output."""
    x = np.asarray(data, dtype=np.float32)
    lp, hp = 0 < low_pass_fraction < 1, 0 < high_pass_fraction < 1
    a = np.log(2) / low_pass_fraction**2 if lp else 0.0
    b = np.log(2) / high_pass_fraction**2 if hp else 0.0
    terms = [(1.0, a), (-1.0, a + b)] if lp and hp else [(1.0, a)] if lp else [(1.0, 0.0), (-1.0, b)] if hp else [(1.0, 0.0)]

    def gauss(f2):
        re, im = x, None
        for ax, n in enumerate(x.shape):
            k = np.arange(n)
            u = ((k + (n + 1) // 2) % n - n // 2).astype(np.float32) / np.float32(n // 2)      # fftshifted float32 coordinates
            c = np.fft.ifft(np.exp(-f2 * (u * u).astype(np.float64)))[(k[:, None] - k[None, :]) % n]
            cr, ci = c.real.astype(np.float32), c.imag.astype(np.float32)
            ap = lambda m, v: np.moveaxis(np.tensordot(m, v, axes=(1, ax)), 0, ax)   # noqa: E731
            if n % 2 == 0:                                                           # c is real on an even side
                re, im = ap(cr, re), None if im is None else ap(cr, im)
            elif im is None:
                re, im = ap(cr, re), ap(ci, re)
            else:
                re, im = ap(cr, re) - ap(ci, im), ap(ci, re) + ap(cr, im)
        assert re.dtype == np.float32
        return re

    out = np.zeros_like(x)
    for coef, f2 in terms:
        out += np.float32(coef) * (x if f2 == 0.0 else gauss(f2))
    return out


SHAPES = [(32, 32, 32), (33, 28, 35), (31, 31, 30), (37, 40, 44),
          # the parity orders of (z, y, x) the four above leave out: which planes carry an imaginary part into the next pass
          (12, 12, 13), (12, 13, 12), (12, 13, 13), (13, 12, 13),
          (65, 63, 64), (64, 65, 63), (63, 64, 65),                     # sides on either side of the 64-row tile, on each axis
          (2, 3, 4), (3, 2, 5), (4, 5, 2)]                              # the smallest sides
LONGEST = [(1024, 2, 3), (3, 1024, 2), (2, 3, 1024)]                    # the documented maximum on each axis in turn


# (ids as two stacked parametrize decorators over shape and dtype would give them: the 1024 sides run in float32 only)
@pytest.mark.parametrize("shape,dtype", [pytest.param(s, t, id=f"{t.__name__}-shape{i}") for i, s in enumerate(SHAPES + LONGEST)
                                         for t in (np.float32, np.float64) if t is np.float32 or s not in LONGEST])
def test_filter_3d_matches_numpy(shape, dtype):
    """Bound 2e-6 max|x|.  For a side of 1024 the bound is first checked against the reference's own float32 floor (the
    same circulant products in float32 NumPy against np_filter_3d): at most a quarter of the bound keeps it, else 4 x the
    floor would hold.  Measured floors on (1024, 2, 3), (3, 1024, 2), (2, 3, 1024): at most 1.6e-7, 1.6e-7 and 2.3e-7 of
    max|x| over the five filters, all below 0.5e-6, so the bound of every other shape stands there too."""
    x = np.random.default_rng(sum(shape)).normal(size=shape).astype(dtype)
    worst = 0.0
    for lp, hp in FRACTIONS:
        want = np_filter_3d(x, lp, hp)
        atol = 2e-6 * np.abs(x).max()
        if max(shape) == 1024:
            floor = np.abs(circulant_f32_filter_3d(x, lp, hp) - want).max()
            print(f"{shape} lp={lp} hp={hp}: float32 floor of the reference {floor / np.abs(x).max():.2e} max|x|")
            if floor > atol / 4:
                atol = 4 * floor
        got = H.low_high_pass_filter_3d(x, lp, hp)
        assert got.dtype == want.dtype == dtype and got.shape == shape
        worst = max(worst, np.abs(got - want).max() / np.abs(x).max())
        np.testing.assert_allclose(got, want, rtol=0, atol=atol, err_msg=f"{shape} lp={lp} hp={hp}")
    print(f"{shape} {np.dtype(dtype).name}: max |got - numpy| = {worst:.2e} max|x| over {len(FRACTIONS)} filters")


def test_filter_3d_many_tiles():
    """256^3: many 64 x 64 tiles along every axis, and a z product with 65536 columns."""
    x = np.random.default_rng(256).normal(size=(256, 256, 256)).astype(np.float32)
    for lp, hp in ((0.2, 0.05), (0, 0.1)):
        np.testing.assert_allclose(H.low_high_pass_filter_3d(x, lp, hp), np_filter_3d(x, lp, hp), rtol=0, atol=2e-6 * np.abs(x).max())


def test_low_high_pass_filter_still_refuses_3d():
    with pytest.raises(NotImplementedError):
        H.low_high_pass_filter(np.zeros((8, 8, 8), np.float32), 0.5)


def test_filter_3d_against_golden(golden_dir):
    g = np.load(golden_dir / "g17_map_input.npz")
    for k in range(int(g["n_filter"][0])):
        x = g[f"filter{k}_in"].astype(np.float32)
        for j, (lp, hp) in enumerate(g["filter_fractions"]):
            want = g[f"filter{k}_{j}_out"]
            got = H.low_high_pass_filter_3d(x, lp, hp)
            assert got.dtype == want.dtype
            np.testing.assert_allclose(got, want, rtol=0, atol=2e-6 * np.abs(x).max(), err_msg=f"filter {k} {j}")


def _sym_case(g, k):
    m, apix, tw, rs, cs, fr, n1, n2, n3, na, rot, tilt = g[f"sym{k}_args"]
    return g[f"map{int(m)}"].astype(np.float32), (apix, tw, rs, int(cs), fr, (int(n1), int(n2), int(n3)), na, rot, tilt)


def test_symmetrize_transform_map_against_golden_and_composition(golden_dir):
    from oracle import symmetrize as S

    g = np.load(golden_dir / "g17_map_input.npz")
    for k in range(int(g["n_sym"][0])):
        vol, (apix, tw, rs, cs, fr, ns, na, rot, tilt) = _sym_case(g, k)
        want = g[f"sym{k}_out"]
        got = H.symmetrize_transform_map(vol, apix, tw, rs, cs, fr, ns, na, rot, tilt)
        assert got.shape == want.shape and got.dtype == np.float32
        # the apply_helical_symmetry / transform_map tolerances (test_gpu_parity, test_gpu_path_a) over the map's range
        np.testing.assert_allclose(got, want, rtol=0, atol=2e-6 * np.abs(want).max(), err_msg=f"case {k}")
        work = np_filter_3d(vol, apix / na).astype(np.float32) if na > apix else vol
        comp = S.apply_helical_symmetry(work, apix, tw, rs, cs, fr, ns, na)
        if rot or tilt:
            comp = S.transform_map(comp, rot=rot, tilt=tilt)
        np.testing.assert_allclose(got, comp, rtol=0, atol=2e-6 * np.abs(want).max(), err_msg=f"case {k} (composition)")
    vol = g["map0"].astype(np.float32)
    # new_apix=None / new_size=None: unchanged, no filter
    np.testing.assert_array_equal(H.symmetrize_transform_map(vol, 1.0, 30.0, 4.75), H.apply_helical_symmetry(vol, 1.0, 30.0, 4.75))


def test_generate_xyz_projections_against_golden(golden_dir):
    g = np.load(golden_dir / "g17_map_input.npz")
    for k in range(int(g["n_proj"][0])):
        m, amy, apix = g[f"proj{k}_args"]
        vol = g[f"map{int(m)}"].astype(np.float32)
        got = H.generate_xyz_projections(vol, is_amyloid=bool(amy), apix=None if apix < 0 else apix)
        for a in range(3):
            want = g[f"proj{k}_{a}"]
            assert got[a].shape == want.shape and got[a].dtype == want.dtype == np.float32
            np.testing.assert_allclose(got[a], want, rtol=0, atol=1e-6 * np.abs(want).max(), err_msg=f"case {k} axis {a}")
    x = np.random.default_rng(5).normal(size=(9, 300, 70))
    got = H.generate_xyz_projections(x)
    for a, i in enumerate((2, 1, 0)):
        assert got[a].dtype == np.float64
        np.testing.assert_allclose(got[a], x.sum(axis=i), rtol=0, atol=1e-5 * x.shape[i] ** 0.5)


def _helix_map(shape, apix, twist, rise, radius, sigma):
    """Gaussian balls on a one-start helix about the z axis."""
    nz, ny, nx = shape
    Z, Y, X = np.meshgrid(*((np.arange(n) - n // 2) * apix for n in shape), indexing="ij")
    vol = np.zeros(shape)
    for n in range(-int(nz * apix / rise) - 2, int(nz * apix / rise) + 3):
        phi = np.deg2rad(n * twist)
        vol += np.exp(-((Z - n * rise) ** 2 + (Y - radius * np.sin(phi)) ** 2 + (X - radius * np.cos(phi)) ** 2) / (2 * sigma**2))
    return vol.astype(np.float32)


def _args(argv):
    return B.add_args(argparse.ArgumentParser()).parse_args(argv)


def test_driver_from_map_image_and_sweep_match_the_library(tmp_path):
    vol = _helix_map((80, 48, 48), 2.5, 29.0, 20.0, 30.0, 5.0)
    np.save(tmp_path / "map.npy", vol)
    argv = [str(tmp_path / "map.npy"), "--from-map", "29", "20", "1", "--apix", "2.5", "--output-size", "40", "24",
            "--axial-rotation", "10", "--output-tilt", "2", "--noise", "0", "--save-projection", str(tmp_path / "p.npy"),
            "--twist", "27", "31", "1", "--rise", "18", "22", "1", "--helical-diameter", "70", "--top", "5", "--out", str(tmp_path / "o.npz")]
    rep = B.run(_args(argv))
    m = H.symmetrize_transform_map(vol, 2.5, 29.0, 20.0, 1, 1.0, (40, 24, 24), 5.0, 10.0, 2.0)
    want = H.generate_xyz_projections(m)[0].T[:, ::-1]
    proj = np.load(tmp_path / "p.npy")
    assert proj.shape == (24, 40) and proj.dtype == np.float32
    np.testing.assert_array_equal(proj, want)
    res = H.sweep(proj, B.sweep_axis(27, 31, 1), B.sweep_axis(18, 22, 1), (1,), apix=5.0, helical_diameter=70.0, ball_radius=10.0)
    np.testing.assert_array_equal(np.load(tmp_path / "o.npz")["scores"], res.scores)
    assert rep["images"][0]["best"]["twist"] == res.best[0][0] and rep["images"][0]["best"]["rise"] == res.best[0][1]
    info = rep["map"]
    assert info["output_size"] == [40, 24] and info["output_apix"] == 5.0 and info["apix"] == 2.5
    assert (info["twist"], info["rise"], info["csym"], info["axial_rotation"], info["tilt"]) == (29.0, 20.0, 1, 10.0, 2.0)
    json.dumps(rep)
    # a seed replays the noise; an .mrc projection carries the output pixel size
    from helicon_amd.mrc import read_mrc

    for out in ("a.npy", "b.mrc"):
        B.run(_args(argv[:argv.index("--noise")] + ["--noise", "0.5", "--seed", "7", "--save-projection", str(tmp_path / out),
                                                   "--twist", "29", "29", "1", "--rise", "20", "20", "1"]))
    a = np.load(tmp_path / "a.npy")
    b, b_apix = read_mrc(tmp_path / "b.mrc")
    np.testing.assert_array_equal(a, b.reshape(a.shape))
    assert b_apix == 5.0 and not np.array_equal(a, want)


def test_driver_from_map_rescore_ranks_the_truth_first(tmp_path):
    """A one-start helix (twist 29, rise 20 Angstrom) at 2.5 Angstrom, projected at 5: the least-squares scorer puts the
    true pair first among the sweep's 25 neighbours.  Checked beforehand on the CPU oracle (oracle/path_a.py, trilinear):
    cosine 0.9955 for the truth against 0.9661 for the runner-up (28, 20)."""
    vol = _helix_map((128, 64, 64), 2.5, 29.0, 20.0, 30.0, 5.0)
    np.save(tmp_path / "map.npy", vol)
    rep = B.run(_args([str(tmp_path / "map.npy"), "--from-map", "29", "20", "1", "--apix", "2.5", "--output-size", "64", "32",
                       "--noise", "0", "--twist", "27", "31", "1", "--rise", "18", "22", "1", "--helical-diameter", "70",
                       "--top", "25", "--rescore", "25"]))
    res = rep["images"][0]["rescored"]
    assert len(res) == 25
    assert (res[0]["twist"], res[0]["rise"]) == (29.0, 20.0)
