"""Host side of the 3-D map input (no GPU): denovo3DBatch --from-map's flags, default output size and image construction
(app.py:266-273, 1780-1829), and the argument checks that come before any device call."""
import argparse

import numpy as np
import pytest

import helicon_amd as H
from helicon_amd import denovo3D as D
from helicon_amd import denovo3DBatch as B


def _args(argv):
    return B.add_args(argparse.ArgumentParser()).parse_args(argv)


def test_from_map_flags_parse_with_the_apps_defaults():
    a = _args(["m.mrc", "--twist", "28", "31", "0.5", "--rise", "4", "6", "0.1"])
    assert a.from_map is None and a.output_apix == 5.0 and a.output_size is None and a.noise == 1.0
    assert a.axial_rotation == 0.0 and a.output_tilt == 0.0 and a.seed is None and a.save_projection is None
    a = _args(["m.mrc", "--from-map", "29.4", "4.75", "2", "--output-apix", "4", "--output-size", "120", "64", "--axial-rotation",
               "12", "--output-tilt", "3", "--noise", "0.5", "--seed", "3", "--save-projection", "p.mrc",
               "--twist", "28", "31", "0.5", "--rise", "4", "6", "0.1"])
    assert a.from_map == [29.4, 4.75, 2.0] and a.output_apix == 4.0 and a.output_size == [120, 64]
    assert (a.axial_rotation, a.output_tilt, a.noise, a.seed, a.save_projection) == (12.0, 3.0, 0.5, 3, "p.mrc")


def test_default_output_size_follows_the_app():
    # app.py:266-273 with output_apix for its literal 5: width from the map's x side, length from half a pitch
    nx, apix, twist, rise = 200, 1.1, 29.4, 4.75
    pitch = 360 * rise / abs(twist)
    assert B.default_output_size(nx, apix, 5.0, twist, rise) == (int(round(0.5 * pitch / 5)) // 4 * 4, int(nx * apix / 5) // 4 * 4)
    assert B.default_output_size(nx, apix, 5.0, -twist, rise) == B.default_output_size(nx, apix, 5.0, twist, rise)
    assert B.default_output_size(256, 1.0, 2.5, 1.2, 4.75) == (int(round(0.5 * 360 * 4.75 / 1.2 / 2.5)) // 4 * 4, 100)
    assert B.default_output_size(256, 1.0, 5.0, 0.0, 4.75) == (2 * 48, 48)   # no pitch: twice the width, as for a NaN pitch


def test_map_image_is_the_apps_transposed_flipped_projection_with_seeded_noise(monkeypatch, tmp_path):
    calls = {}
    rng = np.random.default_rng(0)
    m = rng.random((12, 8, 8)).astype(np.float32)

    def fake_sym(data, apix, twist, rise, csym=1, fraction=1.0, new_size=None, new_apix=None, axial_rotation=0, tilt=0, *, device=0):
        calls["sym"] = (data.shape, apix, twist, rise, csym, fraction, new_size, new_apix, axial_rotation, tilt)
        return m

    def fake_xyz(map3d, is_amyloid=False, apix=None, *, device=0):
        return [map3d.sum(axis=i) for i in (2, 1, 0)]

    monkeypatch.setattr(D, "symmetrize_transform_map", fake_sym)
    monkeypatch.setattr(D, "generate_xyz_projections", fake_xyz)
    vol = np.zeros((30, 20, 20), np.float32)
    clean = B.map_to_image(vol, 1.5, 29.0, 20.0, 2, 5.0, (12, 8), 7.0, 3.0, noise=0)
    assert calls["sym"] == ((30, 20, 20), 1.5, 29.0, 20.0, 2, 1.0, (12, 8, 8), 5.0, 7.0, 3.0)
    want = np.transpose(m.sum(axis=-1))[:, ::-1]                                   # app.py:1805
    assert clean.shape == (8, 12) and clean.dtype == np.float32 and clean.flags.c_contiguous
    np.testing.assert_array_equal(clean, want)
    np.random.seed(11)
    noisy = B.map_to_image(vol, 1.5, 29.0, 20.0, 2, 5.0, (12, 8), 7.0, 3.0, noise=0.7)
    np.random.seed(11)
    sigma = np.std(want[want > 1e-3])                                              # app.py:1818-1821
    expect = want.copy()
    expect += np.random.normal(scale=sigma * 0.7, size=want.shape)
    np.testing.assert_array_equal(noisy, expect)
    # through the driver: the seed replays the noise, the saved projection is the swept image, the report names the map
    np.save(tmp_path / "map.npy", vol)
    seen = []
    monkeypatch.setattr(B, "sweep", lambda images, *a, **k: seen.append(np.array(images)) or _FakeResult())
    rep = B.run(_args([str(tmp_path / "map.npy"), "--from-map", "29", "20", "2", "--apix", "1.5", "--output-size", "12", "8",
                       "--axial-rotation", "7", "--output-tilt", "3", "--noise", "0.7", "--seed", "11",
                       "--save-projection", str(tmp_path / "p.npy"), "--twist", "29", "29", "1", "--rise", "20", "20", "1"]))
    np.testing.assert_array_equal(np.load(tmp_path / "p.npy"), expect)
    np.testing.assert_array_equal(seen[0], expect[None])
    assert rep["map"]["seed"] == 11 and rep["map"]["noise"] == 0.7 and rep["map"]["projection_shape"] == [8, 12]


class _FakeResult:
    def __init__(self):
        from helicon_amd.grid import build_grid

        self.grid = build_grid(np.array([29.0]), np.array([20.0]), (1,), tube_length=60.0)
        self.scores = np.zeros((1, 1, 1, 1), np.float32)
        self.best = [(29.0, 20.0, 1, 0.0)]


def test_new_entry_points_refuse_bad_input_before_the_device():
    with pytest.raises(ValueError, match="3D volume"):
        H.low_high_pass_filter_3d(np.zeros((8, 8), np.float32), 0.5)
    for shape in ((1, 8, 8), (8, 8, 1025)):
        with pytest.raises(ValueError, match="every side"):
            H.low_high_pass_filter_3d(np.zeros(shape, np.float32), 0.5)
    with pytest.raises(ValueError, match="real"):
        H.low_high_pass_filter_3d(np.zeros((4, 4, 4), np.complex64), 0.5)
    vol = np.ones((8, 8, 8), np.float32)
    with pytest.raises(ValueError):
        H.symmetrize_transform_map(vol[0], 1.0, 29.0, 4.75)
    with pytest.raises(ValueError):
        H.symmetrize_transform_map(vol, 1.0, 29.0, 0.0)
    with pytest.raises(ValueError):
        H.symmetrize_transform_map(vol, 1.0, 29.0, 4.75, csym=0)
    with pytest.raises(ValueError):
        H.symmetrize_transform_map(vol, 1.0, 29.0, 4.75, new_size=(8, 8))
    with pytest.raises(ValueError):
        H.symmetrize_transform_map(vol, 1.0, 29.0, 4.75, new_apix=-1.0)
    with pytest.raises(ValueError, match="apix"):
        H.generate_xyz_projections(vol, is_amyloid=True)
    with pytest.raises(ValueError):
        H.generate_xyz_projections(vol[0])


def test_driver_refuses_bad_map_arguments(tmp_path):
    np.save(tmp_path / "img.npy", np.zeros((16, 16), np.float32))
    np.save(tmp_path / "map.npy", np.zeros((16, 16, 16), np.float32))
    base = ["--twist", "29", "29", "1", "--rise", "20", "20", "1", "--apix", "2"]
    for image, extra, msg in [("img.npy", ["--from-map", "29", "20", "1"], "3-D map"),
                              ("map.npy", ["--from-map", "29", "20", "1.5"], "CSYM"),
                              ("map.npy", ["--from-map", "29", "0", "1"], "RISE"),
                              ("map.npy", ["--from-map", "29", "20", "1", "--index", "0"], "--index"),
                              ("map.npy", ["--from-map", "29", "20", "1", "--output-apix", "0"], "output-apix"),
                              ("map.npy", ["--from-map", "29", "20", "1", "--output-size", "4", "64"], "output size")]:
        with pytest.raises(SystemExit, match=msg):
            B.run(_args([str(tmp_path / image), *base, *extra]))


def test_amyloid_slab_is_the_references_python_slice():
    for nz in (1, 5, 25, 64):
        for apix in (0.1, 0.15, 0.5, 1.0, 1.9, 4.0, 10.0):
            nzc = int(round(4.75 / apix))
            z0 = nz // 2 - nzc // 2
            idx = np.arange(nz)[z0: z0 + nzc]
            start, stop = D._amyloid_slab(nz, apix)
            assert list(range(start, stop)) == list(idx), (nz, apix)


def test_numpy_restatement_of_the_3d_filter_matches_the_reference(golden_dir):
    """The test's NumPy form of filters.py:349-372 (tests/test_gpu_map_input.py) against the reference's outputs."""
    from tests.test_gpu_map_input import np_filter_3d

    g = np.load(golden_dir / "g17_map_input.npz")
    for k in range(int(g["n_filter"][0])):
        x = g[f"filter{k}_in"].astype(np.float32)
        for j, (lp, hp) in enumerate(g["filter_fractions"]):
            np.testing.assert_allclose(np_filter_3d(x, lp, hp), g[f"filter{k}_{j}_out"], rtol=0, atol=1e-6 * np.abs(x).max())
