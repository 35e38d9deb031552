"""Host side of the helical symmetry search of a 3-D map (no GPU): the C ABI's new entry points, the scored region, the
grid / skipped pairs / arg-max of ``helical_symmetry_search`` and the command line, the last two with a stub in place of
the device engine (as tests/fake_engine.py stands in for the 2-D sweep)."""
import argparse
import json
import re
from pathlib import Path

import numpy as np
import pytest

import helicon_amd as H
from helicon_amd import _lib
from helicon_amd import symmetry_search as SS

ROOT = Path(__file__).resolve().parents[1]
ENTRY_POINTS = {"hh_hs_create", "hh_hs_set_region", "hh_hs_set_budget", "hh_hs_search", "hh_hs_info", "hh_hs_kernel_ms",
                "hh_hs_destroy", "hh_hs_last_error"}


def test_entry_points_in_header_exports_and_library():
    hdr = (ROOT / "include" / "helicon_hip.h").read_text()
    declared = set(re.findall(r"^\s*(?:int64_t|int|void|const char\*)\s+(hh_hs_\w+)\s*\(", hdr, flags=re.M))
    assert declared == ENTRY_POINTS
    assert ENTRY_POINTS <= set(_lib.EXPORTS)
    L = _lib.lib()   # loads the library and binds every export; no GPU call
    for name in ENTRY_POINTS:
        assert hasattr(L, name)
    assert L.hh_hs_info(None, None, None, None) == -1 and b"NULL handle" in L.hh_hs_last_error(None)
    assert H.SymmetrySearch is SS.SymmetrySearch and H.helical_symmetry_search is SS.helical_symmetry_search


def numpy_region(shape, rmin, rmax, z_fraction):
    """M as the definition states it."""
    nz, ny, nx = shape
    k, j, i = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    r2 = (j - ny // 2) ** 2 + (i - nx // 2) ** 2
    m = r2 >= rmin**2
    if rmax is not None:
        m &= r2 < rmax**2
    if z_fraction < 1:
        h = max(1, int(nz * z_fraction + 0.5) // 2)
        m &= (k - nz // 2 >= -h) & (k - nz // 2 < h)
    return m


@pytest.mark.parametrize("shape,rmin,rmax,zf", [
    ((32, 24, 24), 0, 11, 0.5), ((32, 24, 24), 3, 11, 0.5), ((32, 24, 24), 0, None, 1.0), ((30, 21, 25), 0, 9, 0.5),
    ((30, 21, 25), 2.5, 9.5, 0.3), ((7, 9, 8), 0, None, 0.01), ((16, 16, 16), 0, 4, 2.0), ((5, 64, 40), 10, None, 0.5),
])
def test_region_counts(shape, rmin, rmax, zf):
    spec = SS.region_spec(shape, rmin, rmax, zf)
    m = numpy_region(shape, rmin, rmax, zf)
    planes = np.where(m.any(axis=(1, 2)))[0]
    assert spec["region_voxels"] == int(m.sum())
    assert spec["k_range"] == (int(planes[0]), int(planes[-1]) + 1)
    assert spec["plane_voxels"] == int(m[planes[0]].sum())


def test_region_defaults_and_empty_region():
    spec = SS.region_spec((32, 24, 24))
    assert (spec["rmin"], spec["rmax"], spec["z_fraction"]) == (0.0, 11.0, 0.5)     # rmax = min(ny, nx) // 2 - 1
    assert spec["k_range"] == (8, 24) and spec["region_voxels"] == 5968
    assert SS.region_spec((30, 21, 25))["rmax"] == 9.0 and SS.default_rmax((30, 21, 25)) == 9
    assert SS.region_spec((32, 24, 24), rmax=None)["rmax"] is None
    for bad in (dict(rmin=12, rmax=11), dict(rmin=40, rmax=None), dict(rmax=0), dict(rmin=0.5, rmax=0.9)):
        with pytest.raises(ValueError, match="select no voxel"):
            SS.region_spec((32, 24, 24), **bad)
    with pytest.raises(ValueError, match="select no voxel"):
        SS.region_spec((8, 2, 2))   # the default rmax is 0 there
    for bad in (dict(rmin=-1), dict(z_fraction=0), dict(rmax=-2), dict(rmax=float("nan"))):
        with pytest.raises(ValueError):
            SS.region_spec((32, 24, 24), **bad)


def stub_scores(params):
    tw, rs, cs = params[:, 0], params[:, 1], params[:, 2]
    return (np.exp(-((tw - 29.0) / 1.5) ** 2 - ((rs - 6.0) / 0.7) ** 2) / cs).astype(np.float32)


class StubEngine:
    """What helical_symmetry_search and the command line ask of SymmetrySearch, with closed-form scores."""

    def __init__(self, data, apix, *, fraction=1.0, device=0):
        self.shape, self.apix, self.fraction = tuple(np.asarray(data).shape), apix, fraction
        self.region, self.seen, self.closed = None, None, False

    def set_region(self, rmin=0, rmax=..., z_fraction=0.5):
        self.region = SS.region_spec(self.shape, rmin, rmax, z_fraction)
        return self.region

    def search(self, params):
        self.seen = np.array(params, copy=True)
        return stub_scores(self.seen)

    z_range = (1, 30)

    @property
    def region_voxels(self):
        return self.region["region_voxels"]

    def close(self):
        self.closed = True


def test_grid_order_skips_and_ties_with_a_stub_engine():
    vol = np.zeros((32, 24, 24), np.float32)
    eng = StubEngine(vol, 2.0)
    twists, rises, csyms = [0.0, 28.0, 29.0, 389.0], [0.005, 6.0, 7.0, 32.0], (1, 2)
    res = H.helical_symmetry_search(vol, 2.0, twists, rises, csyms, rmin=2, z_fraction=1.0, engine=eng)
    assert not eng.closed and eng.region["rmin"] == 2.0 and eng.region["rmax"] == 11.0 and eng.region["k_range"] == (0, 32)
    g = res.grid
    assert res.scores.shape == (1, 2, 4, 4) and g.shape == (2, 4, 4)
    # csym-major, then twist, then rise; twist wrapped to [-180, 180]
    want = [(tw, rs, float(cs)) for cs in csyms for tw in (0.0, 28.0, 29.0, 29.0) for rs in rises]
    assert [tuple(p) for p in g.params[:, :3]] == want
    # skipped: |twist| < 0.01, |rise| < 0.01, rise >= nz * apix / 2 = 32
    valid = np.array([abs(tw) >= 0.01 and 0.01 <= abs(rs) < 32.0 for tw, rs, _ in want])
    assert np.array_equal(g.valid, valid) and valid.sum() == 12
    assert np.isneginf(res.scores.reshape(-1)[~valid]).all()
    # what reached the engine: [G, 3], skipped pairs with a harmless (valid, positive) rise
    assert eng.seen.shape == (32, 3) and (eng.seen[~valid, 1] == 6.0).all()
    assert np.array_equal(eng.seen[valid], g.params[valid, :3])
    # twists 29 and 389 are the same candidate: the lowest index wins the tie
    flat = res.scores.reshape(-1)
    assert flat[2 * 4 + 1] == flat[3 * 4 + 1] == flat.max()
    assert int(res.best_index[0]) == 2 * 4 + 1 and res.best[0][:3] == (29.0, 6.0, 1)


def test_input_checks_come_before_any_device_call():
    for bad in (np.zeros((8, 8), np.float32), np.zeros((1, 8, 8), np.float32), np.zeros((4, 4, 4), np.complex64)):
        with pytest.raises(ValueError):
            H.helical_symmetry_search(bad, 2.0, [29.0], [6.0])
    nan = np.zeros((8, 8, 8), np.float32)
    nan[3, 3, 3] = np.nan
    with pytest.raises(ValueError, match="NaN or infinite"):
        H.helical_symmetry_search(nan, 2.0, [29.0], [6.0])
    with pytest.raises(ValueError, match="apix"):
        H.SymmetrySearch(np.ones((8, 8, 8), np.float32), 0.0)


def _args(argv):
    return SS.add_args(argparse.ArgumentParser()).parse_args(argv)


def test_cli_arguments():
    a = _args(["m.mrc", "--twist", "26", "32", "1", "--rise", "4.5", "7.5", "0.5"])
    assert (a.map, a.apix, a.csym, a.fraction, a.rmin, a.rmax, a.z_fraction, a.device, a.top, a.out) == \
        ("m.mrc", None, [1], 1.0, 0.0, None, 0.5, 0, 10, None)
    a = _args(["m.npy", "--apix", "2", "--twist", "26", "32", "1", "--rise", "4.5", "7.5", "0.5", "--csym", "1", "2", "--fraction",
               "0.5", "--rmin", "3", "--rmax", "9", "--z-fraction", "1", "--device", "1", "--top", "3", "--out", "s.npz"])
    assert (a.apix, a.csym, a.fraction, a.rmin, a.rmax, a.z_fraction, a.device, a.top, a.out) == (2.0, [1, 2], 0.5, 3.0, 9.0, 1.0, 1, 3, "s.npz")
    with pytest.raises(SystemExit):
        _args(["m.mrc", "--twist", "26", "32", "1"])   # --rise is required


def test_cli_report_and_out_file_with_a_stub_engine(tmp_path):
    from helicon_amd.mrc import write_mrc

    vol = np.random.default_rng(0).random((32, 24, 24)).astype(np.float32)
    write_mrc(tmp_path / "m.mrc", vol, 2.0)
    made = []

    def factory(data, apix, **kw):
        made.append(StubEngine(data, apix, **kw))
        return made[-1]

    out = tmp_path / "s.npz"
    a = _args([str(tmp_path / "m.mrc"), "--twist", "26", "32", "1", "--rise", "4.5", "7.5", "0.5", "--csym", "1", "2", "--fraction", "0.5",
               "--rmin", "3", "--top", "4", "--out", str(out)])
    rep = SS.run(a, engine_factory=factory)
    json.dumps(rep)
    assert len(made) == 1 and made[0].closed and made[0].apix == 2.0 and made[0].fraction == 0.5   # the header's voxel size
    assert rep["n_candidates"] == 98 and rep["n_skipped"] == 0
    assert rep["best"] == dict(twist=29.0, rise=6.0, csym=1, score=1.0)
    assert [t["score"] for t in rep["top"]] == sorted((t["score"] for t in rep["top"]), reverse=True) and len(rep["top"]) == 4
    assert rep["top"][0] == rep["best"]
    assert rep["fraction"] == 0.5 and rep["z_range"] == [1, 30]
    assert rep["region"] == dict(rmin=3.0, rmax=11.0, z_fraction=0.5, k_range=[8, 24])
    assert rep["region_voxels"] == SS.region_spec(vol.shape, 3)["region_voxels"]
    assert rep["map"] == dict(path=str(tmp_path / "m.mrc"), shape=[32, 24, 24], apix=2.0)
    z = np.load(out)
    assert set(z.files) == {"scores", "twists", "rises", "csyms", "params", "valid"}
    assert z["scores"].shape == (2, 7, 7) and z["params"].shape == (98, 4) and z["valid"].all()
    assert np.array_equal(z["twists"], np.arange(26.0, 32.5)) and np.array_equal(z["csyms"], [1, 2])
    assert np.array_equal(z["scores"].reshape(-1), stub_scores(z["params"]))
    # --rmax negative: no outer limit; --apix overrides the header
    a = _args([str(tmp_path / "m.mrc"), "--apix", "3", "--twist", "29", "29", "1", "--rise", "6", "6", "1", "--rmax", "-1", "--z-fraction", "1"])
    rep = SS.run(a, engine_factory=factory)
    assert made[-1].apix == 3.0 and rep["region"]["rmax"] is None and rep["region_voxels"] == vol.size and rep["n_candidates"] == 1


def test_cli_refuses_a_2d_input_and_a_missing_voxel_size(tmp_path):
    np.save(tmp_path / "img.npy", np.zeros((16, 16), np.float32))
    np.save(tmp_path / "vol.npy", np.zeros((16, 16, 16), np.float32))
    common = ["--twist", "26", "32", "1", "--rise", "4.5", "7.5", "0.5"]
    with pytest.raises(SystemExit, match="needs a 3-D map"):
        SS.run(_args([str(tmp_path / "img.npy"), "--apix", "2", *common]), engine_factory=StubEngine)
    with pytest.raises(SystemExit, match="--apix is required"):
        SS.run(_args([str(tmp_path / "vol.npy"), *common]), engine_factory=StubEngine)
    with pytest.raises(SystemExit, match="select no voxel"):
        SS.run(_args([str(tmp_path / "vol.npy"), "--apix", "2", "--rmin", "30", *common]), engine_factory=StubEngine)
