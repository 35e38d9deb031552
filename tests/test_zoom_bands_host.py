"""The scored-plane probe of tests/zoom_bands.py, checked on the CPU with the reference alone: on every case's plane the
band masks partition the plane, a swapped line moves its band's oracle score by at least ten times the 2e-4 the GPU tests
(tests/test_gpu_zoom_bands.py) hold every band to — in every band, on both axes, in every mode, for candidate 0 against the
probe's image and for the last candidate against the second image — and no band's score is degenerate.

Measured (smallest effect of a swap over all bands and both axes, candidate 0 / last candidate):
    96 x 176 -> 136 x 264   zoom 6.2e-2 / 5.2e-2   lp 0.3 hp 0.05 1.2e-2 / 4.1e-3   hp 0.05 6.7e-2 / 5.7e-2   phase 6.3e-2 / 4.9e-3
    96 x 176 -> 129 x 130   zoom 7.2e-2 / 5.3e-2   lp 0.3 hp 0.05 1.7e-2 / 9.3e-3   hp 0.05 7.8e-2 / 5.7e-2   phase 9.6e-2 / 4.4e-3
    96 x 176 -> 130 x 129   zoom 7.3e-2 / 7.2e-2   lp 0.3 hp 0.05 1.5e-2 / 9.7e-3   hp 0.05 7.9e-2 / 7.7e-2   phase 8.4e-2 / 6.4e-3
    136 x 264, identity     zoom 5.8e-2 / 3.2e-2   lp 0.3 hp 0.05 1.0e-2 / 3.7e-3   hp 0.05 6.4e-2 / 3.4e-2   phase 8.6e-2 / 3.2e-3
    129 x 131, identity     zoom 8.3e-2 / 1.3e-1   lp 0.3 hp 0.05 1.8e-2 / 8.3e-3   hp 0.05 8.6e-2 / 1.4e-1   phase 1.7e-1 / 1.3e-2
"""
import numpy as np
import pytest

import zoom_bands as ZB


def test_cases_are_the_planes_with_the_tile_mechanisms():
    planes = {name: c.plane for name, c in ZB.CASES.items()}
    assert planes == {"zoom_136x264": (136, 264), "zoom_129x130": (129, 130), "zoom_130x129": (130, 129),
                      "identity_136x264": (136, 264), "identity_129x131": (129, 131)}
    for name, c in ZB.CASES.items():
        ony, onx = c.plane
        assert (c.size is None) == name.startswith("identity") and (c.cutoff is None) == (c.size is None)
        assert -(-ony // 128) == 2 and -(-onx // 128) >= 2 and -(-ony // 64) == 3 and -(-onx // 64) >= 3   # zoom and filter tiles
        if c.size is not None:                       # the plane oversamples the image by less than 2
            assert c.cutoff == (2 * ZB.probe_of(c.shape).apix,) * 2 and ony < 2 * c.shape[0] and onx < 2 * c.shape[1]
    assert -(-264 // 128) == 3 and -(-264 // 64) == 5
    assert {(c.plane[0] % 2, c.plane[1] % 2) for c in ZB.CASES.values()} == {(0, 0), (0, 1), (1, 0), (1, 1)}


@pytest.mark.parametrize("name", list(ZB.CASES))
def test_band_masks_partition_the_scored_plane(name):
    ony, onx = ZB.CASES[name].plane
    o = ZB.oracle(name, "zoom")
    for axis, m in enumerate(o.masks):
        assert m.shape == (16, ony, onx) and m.dtype == bool
        assert np.array_equal(m.sum(axis=0), np.ones((ony, onx), dtype=int))        # every bin in exactly one band
        assert m.any(axis=(1, 2)).all()
        lines = m.any(axis=2 - axis)                                                # [bands, n]: whole lines of the other axis
        assert np.array_equal(m, np.broadcast_to(lines[:, :, None] if axis == 0 else lines[:, None, :], m.shape))


@pytest.mark.parametrize("mode", list(ZB.MODES))
@pytest.mark.parametrize("name", list(ZB.CASES))
def test_a_swapped_line_moves_its_band_by_ten_tolerances(name, mode):
    o = ZB.oracle(name, mode)
    n_cand = len(o.probe.params)
    for image in (0, 1):
        cand = o.probe.cand2 if image else 0
        for axis in (0, 1):
            sc = o.scores[image][axis]
            assert sc.shape == (16, n_cand) and np.isfinite(sc).all()
            s = o.sensitivity(image, axis)
            print(f"{name} {mode} image {image} axis {axis}: smallest effect of a swap {s.min():.2e}, "
                  f"smallest |score| of candidate {cand} {np.abs(sc[:, cand]).min():.3f}")
            assert s.shape == (16,) and (s >= ZB.MARGIN * ZB.SCORE_TOL).all(), (name, mode, image, axis, s)
            assert (np.abs(sc[:, cand]) >= 0.5).all(), (name, mode, image, axis, sc[:, cand])       # no degenerate band
            assert int(np.argmax(sc.sum(axis=0))) == cand
