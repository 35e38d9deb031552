"""Host side of the sweep on filtered spectra (low_pass_fraction / high_pass_fraction): the filter's specification, the
public surface, the driver's flags and what a stand-in engine sees.  No GPU."""
import argparse
import inspect
from pathlib import Path

import numpy as np
import pytest

import helicon_amd as H
from helicon_amd import _lib
from helicon_amd import denovo3D as D
from helicon_amd import denovo3DBatch as B
from helicon_amd.grid import build_grid, filter_spec, zoom_spec

from tests.fake_engine import FakeEngine


def _args(argv):
    return B.add_args(argparse.ArgumentParser()).parse_args(argv)


def test_filter_spec_off_values_are_none():
    for lp, hp in ((0, 0), (0.0, 0.0), (None, None), (1, 0), (1.0, 1.0), (2.5, 0), (0, -0.1), (-3, 7), (float("inf"), 0)):
        assert filter_spec(lp, hp) is None, (lp, hp)
    assert filter_spec() is None


def test_filter_spec_combinations():
    assert filter_spec(0.3, 0) == (0.3, 0.0)
    assert filter_spec(0, 0.05) == (0.0, 0.05)
    assert filter_spec(0.3, 0.05) == (0.3, 0.05)
    assert filter_spec(0.3, 1.0) == (0.3, 0.0)            # a fraction >= 1 is off, the other pass stays
    assert filter_spec(-0.3, 0.05) == (0.0, 0.05)         # a fraction <= 0 is off
    assert filter_spec(np.float32(0.5), None) == (0.5, 0.0)
    with pytest.raises(ValueError):
        filter_spec(float("nan"), 0.05)
    with pytest.raises(ValueError):
        filter_spec(0.3, float("nan"))


def test_public_surface():
    assert "hh_set_spectrum_filter" in _lib.EXPORTS
    header = (Path(__file__).resolve().parents[1] / "include" / "helicon_hip.h").read_text()
    assert "int hh_set_spectrum_filter(hh_ctx* ctx, double low_pass_fraction, double high_pass_fraction);" in header
    sig = inspect.signature(H.sweep)
    assert sig.parameters["low_pass_fraction"].default == 0 and sig.parameters["high_pass_fraction"].default == 0
    sig = inspect.signature(H.SweepEngine.set_filter)
    assert list(sig.parameters) == ["self", "low_pass_fraction", "high_pass_fraction"]
    assert all(p.default == 0 for n, p in sig.parameters.items() if n != "self")
    assert H.filter_spec is filter_spec
    assert "filtered" in (H.SweepEngine.last_first_pass.__doc__ or "")
    # a filter never fakes a zoom: the default sampling stays None whatever the filter
    assert zoom_spec((64, 64), 2.0, None, None) is None


def test_driver_flags_parse():
    base = ["i.npy", "--twist", "25", "33", "1", "--rise", "8", "12", "1"]
    a = _args(base)
    assert a.spectrum_low_pass == 0.0 and a.spectrum_high_pass == 0.0
    a = _args(base + ["--spectrum-low-pass", "0.3", "--spectrum-high-pass", "0.05"])
    assert a.spectrum_low_pass == 0.3 and a.spectrum_high_pass == 0.05
    with pytest.raises(SystemExit):
        _args(base + ["--spectrum-high-pass"])
    with pytest.raises(SystemExit):
        _args(base + ["--spectrum-low-pass", "wide"])


class _FakeResult:
    def __init__(self):
        self.grid = build_grid(np.array([29.0]), np.array([10.0]), (1,), tube_length=128.0)
        self.scores = np.zeros((1, 1, 1, 1), np.float32)
        self.best = [(29.0, 10.0, 1, 0.0)]


def test_driver_hands_the_filter_on_and_records_it(monkeypatch, tmp_path):
    np.save(tmp_path / "img.npy", np.zeros((64, 64), np.float32))
    np.save(tmp_path / "m32.npy", np.ones((32, 48), bool))
    seen = []
    monkeypatch.setattr(B, "sweep", lambda images, *a, **k: seen.append(k) or _FakeResult())
    base = [str(tmp_path / "img.npy"), "--twist", "29", "29", "1", "--rise", "10", "10", "1", "--apix", "2"]
    rep = B.run(_args(base + ["--spectrum-high-pass", "0.05", "--out", str(tmp_path / "o.npz")]))
    assert seen[-1]["low_pass_fraction"] == 0.0 and seen[-1]["high_pass_fraction"] == 0.05
    assert seen[-1]["cutoff_res"] is None and seen[-1]["output_size"] is None      # no faked zoom
    assert rep["spectrum_filter"] == [0.0, 0.05] and rep["spectrum_size"] == [64, 64]
    assert np.load(tmp_path / "o.npz")["spectrum_filter"].tolist() == [0.0, 0.05]
    # with a zoom and a mask of the zoomed shape
    rep = B.run(_args(base + ["--spectrum-low-pass", "0.3", "--spectrum-high-pass", "0.05", "--cutoff-res", "8", "10",
                              "--spectrum-size", "32", "48", "--mask", str(tmp_path / "m32.npy"), "--out", str(tmp_path / "z.npz")]))
    assert (seen[-1]["low_pass_fraction"], seen[-1]["high_pass_fraction"]) == (0.3, 0.05)
    assert seen[-1]["output_size"] == (32, 48) and seen[-1]["mask"].shape == (32, 48)
    assert rep["spectrum_filter"] == [0.3, 0.05] and rep["spectrum_size"] == [32, 48]
    out = np.load(tmp_path / "z.npz")
    assert out["spectrum_filter"].tolist() == [0.3, 0.05] and out["spectrum_size"].tolist() == [32, 48]
    # flags that are off: sweep() is called exactly as without them, and zeros are recorded
    B.run(_args(base))
    plain = seen[-1]
    for off in (["--spectrum-low-pass", "0"], ["--spectrum-low-pass", "1.5", "--spectrum-high-pass", "-1"], ["--spectrum-high-pass", "1"]):
        rep = B.run(_args(base + off + ["--out", str(tmp_path / "p.npz")]))
        assert seen[-1].keys() == plain.keys() and "low_pass_fraction" not in seen[-1] and "high_pass_fraction" not in seen[-1]
        assert rep["spectrum_filter"] == [0.0, 0.0]
        assert np.load(tmp_path / "p.npz")["spectrum_filter"].tolist() == [0.0, 0.0]
    n = len(seen)
    with pytest.raises(SystemExit, match="spectrum-low-pass / --spectrum-high-pass"):
        B.run(_args(base + ["--spectrum-high-pass", "nan"]))
    assert len(seen) == n


class _RecordingEngine(FakeEngine):
    """FakeEngine that records the configuration calls sweep() makes (and has the zoom / filter methods)."""

    def __init__(self, n):
        super().__init__(n)
        self.calls = []
        self._filter = None

    def session(self):
        import contextlib

        return contextlib.nullcontext(self)

    def set_geometry(self, **kw):
        self.calls.append(("set_geometry",))

    def set_zoom(self, cutoff_res=None, output_size=None):
        self.calls.append(("set_zoom", cutoff_res, output_size))

    def set_filter(self, low_pass_fraction=0, high_pass_fraction=0):
        self.calls.append(("set_filter", low_pass_fraction, high_pass_fraction))
        self._filter = filter_spec(low_pass_fraction, high_pass_fraction)

    def set_reference(self, images, mask=None, log=True, key=None):
        self.calls.append(("set_reference",))
        super().set_reference(images, mask, log, key)

    def sweep(self, params):
        self.calls.append(("sweep", len(params)))
        return super().sweep(params)


def _sweep(eng, **kw):
    img = np.zeros((64, 64), np.float32)
    return H.sweep(img, np.array([29.0, 30.0]), np.array([10.0]), (1,), apix=2.0, helical_diameter=50.0, ball_radius=4.0, engine=eng, **kw)


def test_sweep_reaches_the_engine_and_off_arguments_leave_its_calls_alone():
    eng = _RecordingEngine(64)
    _sweep(eng)
    today = list(eng.calls)
    assert today == [("set_geometry",), ("set_zoom", None, None), ("set_reference",), ("sweep", 2)]
    for kw in (dict(low_pass_fraction=0, high_pass_fraction=0), dict(low_pass_fraction=1.0), dict(high_pass_fraction=-2), dict(low_pass_fraction=3, high_pass_fraction=1)):
        eng.calls.clear()
        _sweep(eng, **kw)
        assert eng.calls == today, kw                                    # the engine is not asked about a filter at all
    eng.calls.clear()
    _sweep(eng, low_pass_fraction=0.3, high_pass_fraction=0.05)
    assert eng.calls == [("set_geometry",), ("set_zoom", None, None), ("set_filter", 0.3, 0.05), ("set_reference",), ("sweep", 2)]
    # the caller's engine keeps the filter, so a sweep without one clears it first
    eng.calls.clear()
    _sweep(eng)
    assert eng.calls == [("set_geometry",), ("set_zoom", None, None), ("set_filter", 0, 0), ("set_reference",), ("sweep", 2)]
    assert eng._filter is None
    # an engine without set_filter (tests/fake_engine.py as it stands) still serves unfiltered sweeps
    plain = FakeEngine(64)
    plain.session = lambda: __import__("contextlib").nullcontext(plain)
    plain.set_zoom = lambda *a, **k: None
    assert _sweep(plain).scores.shape == (1, 1, 2, 1)


def test_shared_engine_is_returned_without_its_filter(monkeypatch):
    eng = _RecordingEngine(64)
    monkeypatch.setattr(D, "_engine", lambda shape, device: eng)
    img = np.zeros((64, 64), np.float32)
    H.sweep(img, np.array([29.0]), np.array([10.0]), (1,), apix=2.0, helical_diameter=50.0, ball_radius=4.0, high_pass_fraction=0.05)
    assert eng.calls[-2:] == [("set_zoom", None, None), ("set_filter", 0, 0)] and eng._filter is None
    eng.calls.clear()
    H.sweep(img, np.array([29.0]), np.array([10.0]), (1,), apix=2.0, helical_diameter=50.0, ball_radius=4.0)
    assert not any(c[0] == "set_filter" for c in eng.calls)
