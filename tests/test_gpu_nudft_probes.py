"""The non-uniform DFT on the device (csrc/nudft.inc through helicon_amd.pixel_size) against the closed forms of
tests/nudft_probes.py: every side from 1 to 130, every seam, the compiled limit, every images-per-workgroup form and the three
forms of the ring maximum.  One bound, per image and point, on the complex and the abs output alike::

    |got - want| <= B sum |f - mean| + 2^-23 |want| + ny nx (ny + nx) 2^-53 |mean|

No probe and no point is left out, except that the 17-image stack at 32768 points is compared at the 495 point indices its
probe fixes; every test prints the largest used share of the allowance before it asserts."""
import numpy as np
import pytest

import nudft_probes as Q
from helicon_amd import pixel_size as PS

pytestmark = pytest.mark.gpu

SIDE_FAMILIES = [f for f in Q.families() if f != "ipw"]
STACKS = [p.label for p in Q.probes() if p.family == "ipw"]


def bits(a):
    return np.ascontiguousarray(a).view(np.float32 if a.dtype == np.complex64 else a.dtype)


def held(probe):
    """The device's complex and abs outputs of a probe under the bound; returns (complex, abs, used share)."""
    f, (x, y) = Q.images(probe), Q.points(probe)
    got = PS.nudft2d2(x, y, f)
    mag = PS.nudft2d2(x, y, f, output="abs")
    assert got.shape == mag.shape == (len(f), probe.n_pts) and got.dtype == np.complex64 and mag.dtype == np.float32
    idx = slice(None) if probe.pick is None else np.array(probe.pick)
    want = Q.expect(probe, None if probe.pick is None else idx)
    lim = Q.allowance(f, want)
    used = max(Q.share(got[:, idx].astype(np.complex128), want, lim), Q.share(mag[:, idx].astype(np.float64), np.abs(want), lim))
    return got, mag, used


def ring_is_the_abs_maximum(probe, mag, groups):
    f, (x, y) = Q.images(probe), Q.points(probe)
    for group in groups:
        ring = PS.ring_maximum(x, y, f, group)
        assert ring.dtype == np.float32 and np.array_equal(ring, Q.ring_of(mag, group)), (probe.label, group)     # bit for bit


@pytest.mark.parametrize("family", SIDE_FAMILIES)
def test_sides_and_seams(family):
    assert PS.nudft_chunk() == Q.CHUNK
    worst, n_img, late = (0.0, ""), 0, []
    for probe in (p for p in Q.probes() if p.family == family):
        if family == "limit":
            x, y = Q.points(probe)
            assert np.abs(x).max() > 4 and np.abs(y).max() > 4 and max(probe.shape) == 16384
        _, mag, used = held(probe)
        ring_is_the_abs_maximum(probe, mag, (1, probe.n_pts))
        n_img += mag.shape[0]
        worst = max(worst, (used, probe.label))
        if used > 1.0:
            late.append((probe.label, used))
    print(f"{family}: {n_img} images: largest used share of the allowance {worst[0]:.3e} ({worst[1]})")
    assert not late, late


@pytest.mark.parametrize("label", STACKS)
def test_images_per_workgroup(label):
    """Every row of the stack under the bound, so a row that took another image's sum shows; the whole stack equals, bit for
    bit, the same images in calls short enough for one image a workgroup, and a sample of rows the image transformed alone."""
    probe = Q.by_label(label)
    n_img, n_pts = len(probe.parts), probe.n_pts
    assert PS.nudft_chunk() == Q.CHUNK and probe.ipw == tuple(dict.fromkeys(l[4] for l in Q.launches(n_img, n_pts)))
    assert probe.ipw[0] >= 2
    f, (x, y) = Q.images(probe), Q.points(probe)
    got, mag, used = held(probe)
    print(f"{label}: ipw {probe.ipw}: largest used share of the allowance {used:.3e}")
    assert used <= 1.0
    piece = 1
    while piece * 2 <= n_img and all(l[4] == 1 for l in Q.launches(piece * 2, n_pts)):
        piece *= 2
    apart = np.concatenate([PS.nudft2d2(x, y, f[b:b + piece]) for b in range(0, n_img, piece)])
    assert -(-n_img // piece) <= 16 and np.array_equal(bits(got), bits(apart))
    for b in Q.group_edges(n_img, n_pts):
        assert np.array_equal(bits(got[b]), bits(PS.nudft2d2(x, y, f[b]))), (label, b)
        assert np.array_equal(mag[b], PS.nudft2d2(x, y, f[b], output="abs")), (label, b)
    groups = (1, n_pts) + ((probe.ring_group,) if probe.ring_group else ())
    ring_is_the_abs_maximum(probe, mag, groups)
    if probe.ring_group:                               # the closed form's ring too, under the largest allowance of its points
        want = Q.expect(probe)
        lim = Q.ring_allowance(Q.allowance(f, want), probe.ring_group)
        ring = PS.ring_maximum(x, y, f, probe.ring_group).astype(np.float64)
        assert Q.share(ring, Q.ring_of(np.abs(want), probe.ring_group), lim) <= 1.0
