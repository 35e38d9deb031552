"""The probe list of tests/nudft_probes.py without a GPU: its closed forms against the float64 direct sum, a census of the rules
it reaches, every wrong rule of its model shown to break the bound on a named probe, and, for the record, what the same wrong
rules do to the unit-noise cases of tests/test_gpu_pixel_size.py under their bound B sum |f - mean|."""
import numpy as np
import pytest

import nudft_probes as Q
import pixel_size_cases as Y

SUMMED = [p for p in Q.probes() if p.family != "ipw"]      # small enough for the direct sum at their 65 points


def _at(probe):
    """(x, y, idx) of the points a probe is compared at."""
    x, y = Q.points(probe)
    if probe.pick is None:
        return x, y, None
    idx = np.array(probe.pick)
    return x[idx], y[idx], idx


def test_closed_forms_are_the_direct_sum():
    worst = {}
    for p in SUMMED:
        f, (x, y) = Q.images(p), Q.points(p)
        want = Q.expect(p)
        lim = Q.allowance(f, want)
        for name, got in (("yardstick", Y.yardstick(x, y, f)), ("model", Q.model(x, y, f))):
            s = Q.share(got, want, lim)
            assert s <= 1.0, (p.label, name, s)
            if s > worst.get((p.family, name), (0.0, ""))[0]:
                worst[(p.family, name)] = (s, p.label)
    for (family, name), (s, label) in sorted(worst.items()):
        print(f"{family}: {name} uses {s:.2e} of the allowance at most ({label})")
    # the delta's closed form against the sum, where no mean, offset or output format plays a part
    p = Q.by_label("cross 65x129")
    deltas = [b for b, parts in enumerate(p.parts) if parts[0][0] == "delta"]
    diff = np.abs(Q.expect(p)[deltas] - Y.yardstick(*Q.points(p), Q.images(p)[deltas])).max()
    print(f"cross 65x129: delta closed form - yardstick = {diff:.1e}")
    assert diff <= 1e-10


def test_dirichlet_kernel():
    for n in (1, 2, 3, 64, 129):
        t = np.array([0.0, 2 * np.pi, 0.3, -4.1, 3.0])
        k = np.arange(n) - n // 2
        want = np.exp(-1j * np.outer(t, k)).sum(axis=1)
        assert np.abs(Q.dirichlet(t, n) - want).max() <= 1e-12 * n
        assert Q.dirichlet(0.0, n) == n


def test_probe_list_is_what_the_issue_sets():
    P = Q.probes()
    shapes = {p.shape for p in P}
    assert {(ny, 3) for ny in range(1, 131)} | {(3, nx) for nx in range(1, 131)} <= shapes
    assert {(2, nx) for nx in (255, 256, 257, 383, 385)} | {(ny, 2) for ny in (127, 128, 129, 191, 192, 193)} <= shapes
    assert {(65, 129), (129, 65), (16384, 3), (3, 16384)} <= shapes
    assert all(p.n_pts == Q.N_POINTS and p.pick is None and p.ipw == (1,) for p in SUMMED)
    x, y = Y.points(Q.N_POINTS)
    assert x[0] == 0 and y[0] == 0 and x[2] == x[1] - 2 * np.pi and np.abs(x).max() > 4 and np.abs(y).max() > 4

    def where(p):
        return {(part[1], part[2]) for parts in p.parts for part in parts if part[0] == "delta"}

    for p in SUMMED:
        ny, nx = p.shape
        at, kinds = where(p), [parts[0][0] for parts in p.parts]
        if p.family == "limit":
            long_axis = 0 if ny == Q.MAX_SIDE else 1
            assert sorted(q[long_axis] for q in at) == [0, 8191, 8192, 8193, 16383] and kinds.count("const") == 1
            continue
        assert {(0, 0), (0, nx - 1), (ny - 1, 0), (ny - 1, nx - 1)} <= at
        assert {r for r in (63, 64) if r < ny} <= {q[0] for q in at} and {c for c in (31, 32, 127, 128) if c < nx} <= {q[1] for q in at}
        assert kinds[-4:] == ["const", "row", "col", "noise"]
        if p.family in ("rows", "columns"):
            assert {r for r in Q.ACC_ROWS if r < ny} <= {q[0] for q in at}
        if p.family == "cross":
            assert {(r, c) for r in (0, 63, 64, ny - 1) for c in (0, 31, 32, 127, 128, nx - 1) if c < nx} <= at
    assert Q.seam_cols(385) == [31, 32, 127, 128, 255, 256, 383, 384] and Q.seam_rows(193) == [63, 64, 127, 128, 191, 192]


def test_images_per_workgroup_table():
    """The table of (images, points, shape) and the ipw each launch of it gets by nudft.inc's formula."""
    table = {p.label: (len(p.parts), p.n_pts, p.shape, p.ipw) for p in Q.probes() if p.family == "ipw"}
    for label, row in table.items():
        print(label, row)
    assert list(table.values()) == [
        (8192, 64, (2, 3), (2,)), (8193, 64, (2, 3), (2,)), (12288, 64, (2, 3), (3,)), (32763, 64, (1, 1), (7,)),
        (16387, 65, (1, 1), (8,)), (4097, 65, (2, 3), (2,)), (17, Q.CHUNK, (65, 129), (2,)), (17, Q.CHUNK + 1, (2, 3), (2, 1))]
    assert [Q.ipw_of(n, 64) for n in (1, 8191, 8192, 12287, 12288, 32763, 32768)] == [1, 1, 2, 2, 3, 7, 8]
    assert Q.ipw_of(4097, 65) == 2 and Q.ipw_of(17, Q.CHUNK) == 2 and Q.ipw_of(16, Q.CHUNK - 64) == 1 and Q.ipw_of(17, 1) == 1
    for n_img, n_pts, _, ipw in table.values():
        ragged = n_img % ipw[0] != 0
        assert ragged == (n_img in (8193, 32763, 16387, 4097, 17))
        edges = Q.group_edges(n_img, n_pts)
        assert edges[0] == 0 and edges[-1] == n_img - 1 and {ipw[0] - 1, ipw[0]} <= set(edges)
    carry = Q.by_label(f"ipw 2 ragged, 17 of 65x129, {Q.CHUNK} points")
    tiles = Q.CHUNK // 64
    assert {0, 63, 64, 127, 64 * (tiles - 1), Q.CHUNK - 1} <= set(carry.pick) and 480 <= len(carry.pick) <= 520
    for p in Q.probes():                      # every image of a stack differs from its neighbours
        if p.family == "ipw":
            f = Q.images(p).reshape(len(p.parts), -1)
            assert (f[1:] != f[:-1]).any(axis=1).all(), p.label


def test_census_every_rule_is_reached():
    reach = {rule: [p.label for p in Q.probes() if rule in p.rules] for rule in Q.RULES}
    for rule, labels in reach.items():
        print(f"{rule}: {len(labels)} probes, e.g. {labels[0] if labels else None}")
    assert all(reach.values())
    assert {rule for rule, _ in Q.WRONG.values()} == set(Q.RULES) and len(Q.WRONG) == 14
    assert all(set(p.rules) <= set(Q.RULES) for p in Q.probes())


def _broken(probe, wrong):
    """The largest error over allowance that the model with one wrong rule leaves on a probe."""
    f = Q.images(probe)
    x, y, idx = _at(probe)
    want = Q.expect(probe, idx)
    lim = Q.allowance(f, want)
    if wrong == "ring_local":
        g = probe.ring_group
        return Q.share(Q.ring_of(np.abs(Q.model(x, y, f)), g, local=True), Q.ring_of(np.abs(want), g), Q.ring_allowance(lim, g))
    return Q.share(Q.model(x, y, f, wrong, probe.n_pts, idx), want, lim)


@pytest.mark.parametrize("wrong", list(Q.WRONG))
def test_every_wrong_rule_breaks_the_bound(wrong):
    rule, text = Q.WRONG[wrong]
    hit = [(p.label, _broken(p, wrong)) for p in Q.probes() if rule in p.rules and (wrong != "ring_local" or p.ring_group)]
    caught = [h for h in hit if h[1] > 1.0]
    label, factor = max(hit, key=lambda h: h[1])
    print(f"{wrong} ({text}): {len(caught)} of the {len(hit)} probes that reach '{rule}' break the bound; worst {label}: {factor:.3g} x")
    assert caught, wrong
    first = caught[0]
    print(f"    first: {first[0]}: {first[1]:.3g} x")


# What the same wrong rules do to the unit-noise cases the GPU tests had before the probes (pixel_size_cases.accuracy_cases, the
# 65-point stack-of-one cases, the long sides and the offset image), under THEIR bound B sum |f - mean|: True = the case
# catches it.  Rules that need ipw > 1, and the ring's index, touch none of these cases.
EXISTING = {
    "centre": {"points 2x3": True, "points 37x50": True, "points 64x64": True, "points 65x63": False, "points 128x130": True,
               "long 4x4096": True, "long 4096x4": True, "long 3x8191": False, "offset 64x64": True},     # odd sides: n // 2 either way
    "pairing": {"points 2x3": True, "points 37x50": True, "points 64x64": True, "points 65x63": True, "points 128x130": True,
                "long 4x4096": True, "long 4096x4": True, "long 3x8191": True, "offset 64x64": True},
    "sign": {"points 2x3": True, "points 37x50": True, "points 64x64": True, "points 65x63": True, "points 128x130": True,
             "long 4x4096": True, "long 4096x4": True, "long 3x8191": True, "offset 64x64": True},
    # 1.17, 0.87 and 1.61 times the bound on the three long sides; the offset image catches it through the mean's term (40 x)
    "f32phase": {"points 2x3": False, "points 37x50": False, "points 64x64": False, "points 65x63": False, "points 128x130": False,
                 "long 4x4096": True, "long 4096x4": False, "long 3x8191": True, "offset 64x64": True},
    "row_pad": {"points 2x3": True, "points 37x50": True, "points 65x63": True, "long 4x4096": True, "long 3x8191": True},
    "col_pad": {"points 2x3": True, "points 37x50": True, "points 64x64": True, "points 65x63": True, "points 128x130": True,
                "long 4096x4": True, "long 3x8191": True, "offset 64x64": True},
    "stage_first": {"points 128x130": True, "long 4x4096": True, "long 3x8191": True},
    "slice_late": {"points 37x50": True, "points 64x64": True, "points 65x63": True, "points 128x130": True, "long 4x4096": True,
                   "long 3x8191": True, "offset 64x64": True},
    "acc_swap": {"points 37x50": True, "points 64x64": True, "points 65x63": True, "points 128x130": True, "long 4096x4": True,
                 "offset 64x64": True},
    "no_mean": {"points 2x3": True, "points 37x50": True, "points 64x64": True, "points 65x63": True, "points 128x130": True,
                "long 4x4096": True, "long 4096x4": True, "long 3x8191": True, "offset 64x64": True},
    # a noise image's mean is about 1 / sqrt(ny nx): 1.2 and 1.3 times the bound on 37 x 50 and 4 x 4096
    "mean_off_centre": {"points 2x3": True, "points 37x50": True, "points 64x64": True, "points 65x63": False,
                        "points 128x130": True, "long 4x4096": True, "long 4096x4": True, "long 3x8191": False, "offset 64x64": True},
    "skip_ragged": {}, "prev_image": {}, "ring_local": {},
}


def _existing(label):
    for name, f, x, y in Y.accuracy_cases(Q.CHUNK):
        if name in (f"{label} stack 1 n 65", label):
            return f, x, y
    raise KeyError(label)


def test_what_the_noise_cases_catch():
    for wrong, cases in EXISTING.items():
        for label, caught in cases.items():
            f, x, y = _existing(label)
            used = float((np.abs(Q.model(x, y, f, wrong) - Y.yardstick(x, y, f)) / (Y.B * Y.scale(f)[:, None])).max())
            print(f"{wrong} on {label}: {used:.3g} x B sum|f - mean|: {'caught' if used > 1 else 'PASSES'}")
            assert (used > 1.0) == caught, (wrong, label, used)
    assert set(EXISTING) == set(Q.WRONG)
    # the gap on record: float32 phases pass one of the three cases written for them
    assert EXISTING["f32phase"]["long 4096x4"] is False


def test_a_phase_error_on_one_column_hides_in_noise():
    """1e-3 radians on column 128, the first of the second stage: the 128 x 130 noise case passes it, a delta there does not."""
    f, x, y = _existing("points 128x130")
    used = float((np.abs(Q.model(x, y, f, col_phase=(128, 1e-3)) - Y.yardstick(x, y, f)) / (Y.B * Y.scale(f)[:, None])).max())
    p = Q.by_label("columns 3x130")
    want = Q.expect(p)
    probe = Q.share(Q.model(*Q.points(p), Q.images(p), col_phase=(128, 1e-3)), want, Q.allowance(Q.images(p), want))
    print(f"1e-3 rad on column 128: points 128x130 uses {used:.2f} of its bound, {p.label} {probe:.3g} of its allowance")
    assert used < 1.0 < probe
    one = np.array([[[2.0]]], np.float32)                     # a one-pixel image is its own mean: the bound is the format's
    assert Q.allowance(one, np.array([[2.0 + 0j]])).max() < 3e-7


def _origin_sum(h, col, nx, ny, slices_a_fold):
    """The kernel's float32 order at the origin point, where every factor is 1, for a delta h at (0, col): a slice's chain of 32
    terms, the slices added in float32, the sum folded into float64 every ``slices_a_fold`` slices; then the mean's term."""
    f32 = np.float32
    mean = h / (ny * nx)
    delta, floor = f32(h - mean), f32(0.0 - mean)
    total = 0.0
    for row in range(2):                               # the delta's row, and one of the others
        tile = f32(0)
        part = 0.0
        for s in range(nx // Q.NU_K):
            chain = f32(0)
            for c in range(Q.NU_K):
                chain = f32(chain + (delta if row == 0 and s * Q.NU_K + c == col else floor))
            tile = f32(tile + chain)
            if s % slices_a_fold == slices_a_fold - 1:
                part, tile = part + float(tile), f32(0)
        total += part * (1 if row == 0 else ny - 1)
    return total + mean * ny * nx


def test_the_defect_the_limit_probe_found():
    """A delta of height 1 at column 0 of 3 x 16384, seen from the origin: under its mean's floor of -1 / 49152 a pixel, the 511
    later slices each add the same -32 / 49152 to a sum near 1, and float32 rounds every one of those additions the same way.
    Summed in float32 along the whole row (the kernel before this probe) that is 8.5e-6, 1.38 times the allowance, the figure
    an MI355X gave; folded into float64 every 512 columns (16 slices) it is 4e-7."""
    p = Q.by_label("limit 3x16384")
    ny, nx = p.shape
    assert p.parts[0] == (("delta", 0, 0, 1.0),)
    lim = float(Q.allowance(Q.images(p)[:1], np.array([[1.0 + 0j]]))[0, 0])
    whole = abs(_origin_sum(1.0, 0, nx, ny, nx // Q.NU_K) - 1.0) / lim
    folded = abs(_origin_sum(1.0, 0, nx, ny, 16) - 1.0) / lim
    print(f"limit 3x16384, delta at column 0, origin: one float32 chain {whole:.3f} x the allowance, folded every 512 columns {folded:.3f} x")
    assert 1.38 < whole < 1.39 and folded < 0.1
