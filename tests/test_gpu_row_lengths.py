"""The census of row lengths: every 31-smooth nx in [8, 1024] (109 lengths on the two-step kernel k_gen_rows<R1, R2>,
326 on the Stockham kernel k_gen_fused) and a sample of the lengths with a prime factor above 31 (float64 direct path),
each swept on a 24 x nx image and compared with the float64 oracle under EVERY kx-band mask of tests/spectrum_bands.py —
masks that together see every spectrum column, on a geometry whose spectrum has no empty column — for log1p|F| and |F|;
the kernel that served each length is read back (SweepEngine.last_row_kernel), the fast kernels are compared with each
other and with the float64 direct path, and every sweep is repeated bit for bit.  Then the ny side (the column transform:
a direct sum over ny//2 + 1 rows in blocks of 8) under ky-band masks, and a tilted list longer than one launch's gridDim.z.

Tolerances (spectrum_bands): against the oracle max(2e-5, 4 x the reference's own float32 floor) per band, between device
paths 5e-6; tests/test_spectrum_bands_host.py shows that a misplaced column moves its band by >= 10 x that tolerance."""
import numpy as np
import pytest

import helicon_amd as H
import spectrum_bands as SB
from oracle import path_b as O

pytestmark = pytest.mark.gpu

TWO_STEP_BLOCKS, STOCKHAM_BLOCKS = 3, 7


def device_scores(eng, probe, masks, log, images=None):
    """[bands, candidates] of the first segment and the kernel that ran (spectrum_bands.device_scores)."""
    got, kernel = SB.device_scores(eng, probe, masks, log, images)
    return got[:, 0], kernel


class Worst:
    """Largest figures of one test item, printed at its end (pytest -s / -rP shows them)."""

    def __init__(self):
        self.v = {}

    def add(self, name, value, where):
        if value > self.v.get(name, (-1.0, None))[0]:
            self.v[name] = (float(value), where)

    def report(self, title):
        print(title + ": " + "; ".join(f"{k} {v:.2e} at {w}" for k, (v, w) in sorted(self.v.items())))


def check_length(nx, want, monkeypatch, worst, failures, logs=(True, False), probe=None, ny=SB.NY, axis=1):
    """One row length on its own kernel (`want`: the pair, "stockham" or "direct") against the oracle under every band, and
    against the other device paths."""
    probe = probe or SB.probe_for_length(nx, ny)
    with H.SweepEngine((ny, nx)) as eng:
        assert eng.general
        eng.set_geometry(**probe.geometry())
        for log in logs:
            o = SB.OracleSide(probe, log, axis)
            tag = f"{ny}x{nx} log={int(log)} units={len(probe.units)}"
            got, kernel = device_scores(eng, probe, o.masks, log)
            if want == "direct":
                assert kernel == (0, 0, 0), (tag, kernel)
            elif want == "stockham":
                assert kernel == (0, 0, probe.stockham_lds()), (tag, kernel)
            else:
                assert kernel[:2] == want and 0 < kernel[2] <= SB.LDS_LIMIT, (tag, kernel)      # ran as its pair
            err = np.abs(got - o.scores).max(axis=1)                                            # [bands]
            worst.add(f"oracle({want if isinstance(want, str) else 'two-step'})", err.max(), tag)
            worst.add("tolerance", o.tol.max(), tag)
            if (err > o.tol).any():
                failures.append(f"{tag}: |score - oracle| per band {np.array2string(err, precision=1)} > tolerance {np.array2string(o.tol, precision=1)}")
            # the second experimental image (made from the Csym 2 candidate), same kernel, against the oracle
            o2 = SB.OracleSide(probe, log, axis, image=probe.image2)
            got2, kernel2 = device_scores(eng, probe, o2.masks, log, probe.image2)
            assert kernel2 == kernel, (tag, kernel2)
            err2 = np.abs(got2 - o2.scores).max(axis=1)
            worst.add(f"oracle, second image({want if isinstance(want, str) else 'two-step'})", err2.max(), tag)
            if (err2 > o2.tol).any():
                failures.append(f"{tag}, second image: |score - oracle| per band {np.array2string(err2, precision=1)} > tolerance {np.array2string(o2.tol, precision=1)}")
            if want == "direct":
                continue
            if want != "stockham" and probe.stockham_lds() <= SB.LDS_LIMIT:                     # two-step against Stockham
                monkeypatch.setenv("HH_GEN_STOCKHAM", "1")
                st, k = device_scores(eng, probe, o.masks, log)
                monkeypatch.delenv("HH_GEN_STOCKHAM")
                assert k == (0, 0, probe.stockham_lds()), (tag, k)
                d = float(np.abs(st - got).max())
                worst.add("two-step vs Stockham", d, tag)
                if d > SB.PATHS_TOL:
                    failures.append(f"{tag}: |two-step - Stockham| {d:.2e}")
            monkeypatch.setenv("HH_GEN_DIRECT", "1")
            dr, k = device_scores(eng, probe, o.masks, log)
            monkeypatch.delenv("HH_GEN_DIRECT")
            assert k == (0, 0, 0), (tag, k)
            d = float(np.abs(dr - got).max())
            worst.add("fast vs float64 direct", d, tag)
            if d > SB.PATHS_TOL:
                failures.append(f"{tag}: |fast - direct| {d:.2e}")
            worst.add("direct vs oracle", float(np.abs(dr - o.scores).max()), tag)


@pytest.mark.parametrize("block", range(TWO_STEP_BLOCKS))
def test_every_two_step_pair_against_oracle_on_all_columns(block, monkeypatch):
    two, _, _ = SB.census()
    assert len(two) == 109
    lengths = sorted(two)[block::TWO_STEP_BLOCKS]
    worst, failures = Worst(), []
    for nx in lengths:
        check_length(nx, two[nx], monkeypatch, worst, failures)
    worst.report(f"two-step block {block}: {len(lengths)} lengths")
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("block", range(STOCKHAM_BLOCKS))
def test_every_stockham_length_against_oracle_on_all_columns(block, monkeypatch):
    """A length whose launch needs more than 160 KB of LDS under the five-subunit probe is served by the float64 direct
    path (log1p|F| checked there), and its Stockham kernel is tested with the largest probe that fits."""
    _, stockham, _ = SB.census()
    assert len(stockham) == 326
    lengths = stockham[block::STOCKHAM_BLOCKS]
    worst, failures, fell_back = Worst(), [], []
    for nx in lengths:
        full = SB.Probe(SB.NY, nx)
        if full.stockham_lds() > SB.LDS_LIMIT:
            fell_back.append(nx)
            check_length(nx, "direct", monkeypatch, worst, failures, logs=(True,), probe=full)
        check_length(nx, "stockham", monkeypatch, worst, failures)
    worst.report(f"Stockham block {block}: {len(lengths)} lengths, direct path for LDS with five subunits: {fell_back}")
    assert not failures, "\n".join(failures)


def test_direct_only_lengths_against_oracle_on_all_columns(monkeypatch):
    _, _, direct = SB.census()
    assert set(SB.DIRECT_SAMPLE) <= set(direct) and len(set(SB.DIRECT_SAMPLE)) >= 20
    worst, failures = Worst(), []
    for nx in SB.DIRECT_SAMPLE:
        check_length(nx, "direct", monkeypatch, worst, failures, logs=(True,))
    worst.report(f"direct-only sample: {len(SB.DIRECT_SAMPLE)} lengths")
    assert not failures, "\n".join(failures)


def test_no_row_length_is_refused():
    """Every nx in [8, 1024] sweeps the census's list: no length raises.  (The 31-smooth ones are swept by the tests above;
    here all 582 lengths with a prime factor above 31, two candidates under the whole plane against the oracle.)"""
    _, _, direct = SB.census()
    assert len(direct) == 582
    worst = 0.0
    for nx in direct:
        probe = SB.Probe(SB.NY, nx)
        with H.SweepEngine((SB.NY, nx)) as eng:
            eng.set_geometry(**probe.geometry())
            eng.set_reference(probe.image, np.ones((SB.NY, nx), dtype=bool))
            sc = eng.sweep(probe.params[:2])[0]
            assert eng.last_row_kernel == (0, 0, 0) and eng.last_first_pass == "transform"
        e = SB.amplitude(probe.image, True)
        ref = [O.cross_correlation_coefficient(e, SB.amplitude(probe.simulate(*p[:3]), True)) for p in probe.params[:2]]
        worst = max(worst, float(np.abs(sc - ref).max()))
        assert np.abs(sc - ref).max() <= SB.ORACLE_TOL, (nx, sc, ref)
    print(f"{len(direct)} direct-only lengths under the whole plane: worst |score - oracle| {worst:.2e}")


NY_SIDE = tuple(range(8, 41)) + (63, 64, 65, 127, 128, 255, 256, 511, 512, 1023, 1024)


@pytest.mark.parametrize("nx,want", [(40, (8, 5)), (154, "stockham")])
@pytest.mark.parametrize("part", range(2))
def test_column_transform_heights_against_oracle_on_all_rows(nx, want, part, monkeypatch):
    """The ny side: nky = ny//2 + 1 rows in blocks of 8 (every remainder, odd and even heights, one block to 65), under
    ky-band masks that together see every spectrum row."""
    worst, failures = Worst(), []
    heights = NY_SIDE[part::2]
    for ny in heights:
        check_length(nx, want, monkeypatch, worst, failures, ny=ny, axis=0)
    worst.report(f"nx {nx}, {len(heights)} heights")
    assert not failures, "\n".join(failures)


def test_tilted_list_longer_than_one_launch_on_a_small_image():
    """gen_sweep_direct's batch is the z extent of its transform launches: on an 8 x 8 image 512 MB of scratch hold about
    279,000 candidates, so a tilted list longer than 65,535 must be cut at the grid limit, not refused."""
    import torch

    ny = nx = 8
    apix, d, br, tilt = 2.0, 0.4 * 8 * 2.0, 2.0, 2.0
    clean = O.simulate_helical_projection(1, 40.0, 5.0, 1, d, br, 0, 0, ny, nx, apix, tilt=tilt)
    img = (clean + np.random.default_rng(4).normal(0, 0.3 * clean.std(), clean.shape)).astype(np.float32)
    grid = H.build_grid(20.0 + 0.5 * np.arange(70), 3.0 + 0.004 * np.arange(1000), (1,), tube_length=nx * apix)
    n = len(grid)
    assert n == 70000
    mask = np.ones((ny, nx), dtype=bool)
    with H.SweepEngine((ny, nx)) as eng:
        assert eng.general
        eng.set_geometry(apix=apix, helical_diameter=d, ball_radius=br, tilt=tilt)
        eng.set_reference(img, mask)
        got = eng.sweep(grid.params)[0]
        assert eng.last_first_pass == "transform" and eng.last_row_kernel == (0, 0, 0)
        halves = np.concatenate([eng.sweep(grid.params[: n // 2])[0], eng.sweep(grid.params[n // 2:])[0]])
        assert np.array_equal(got, halves)
        # the device entry point with a row stride, two segments: segment s of candidate i at [s * ld + i]
        eng.set_reference(np.stack([img, img[::-1].copy()]), mask)
        two = eng.sweep(grid.params)
        ld = n + 24
        dp = torch.as_tensor(grid.params, device="cuda")
        ds = torch.full((2 * ld,), -2.0, dtype=torch.float32, device="cuda")
        eng.sweep_device(dp.data_ptr(), n, ds.data_ptr(), host_params=grid.params, ld_scores=ld)
        eng.synchronize()
        strided = ds.cpu().numpy().reshape(2, ld)
    assert np.array_equal(two[0], got)
    assert np.array_equal(strided[:, :n], two) and (strided[:, n:] == -2.0).all()
    pick = np.unique(np.concatenate([[0, 1, 65534, 65535, 65536, n - 1, n // 2 - 1, n // 2],
                                     np.random.default_rng(0).integers(0, n, 24)]))
    ref = O.sweep_cpu(img, grid.params[pick, :3], mask, apix=apix, helical_diameter=d, ball_radius=br, tilt=tilt)
    print(f"8 x 8, {n} tilted candidates: worst |score - oracle| {np.abs(got[pick] - ref).max():.2e} at {len(pick)} indices")
    np.testing.assert_allclose(got[pick], ref, rtol=0, atol=SB.ORACLE_TOL)
