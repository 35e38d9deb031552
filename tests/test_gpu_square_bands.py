"""The tuned power-of-two sweep seen line by line (tests/square_bands.py): for every compiled size N = 32 ... 1024, both
spectra and both axes, the probe's 4 x 8 list is swept under each of the 16 band masks of the axis on the transform,
run-table and fused pipelines, the fused one with the walk forced to rises and to twists, against three references: the
probe's image, its second image, and both as two segments (EPI_QSTORE, the compact q and k_segment_corr under live-bin
patterns the radial band never makes: a few columns per row under a |kx| band, one or two ky blocks under a |ky| band).

After every sweep `last_first_pass`, `last_fused_walk` and `last_factor_sets` say which code ran, and the library's footprint
report must equal the helper's restatement of it with a resident workgroup for each built walk.  Every sweep is repeated
bit for bit.  The two walks are the same arithmetic: `array_equal`.  All paths agree within 2e-5, a row
of the two-segment sweep equals its single-segment sweep within 2e-6, and every band score of every picked candidate is held
to `spectrum_bands.band_scores` of the float64 projections at max(2e-5, 4 x the reference's own float32 floor) — a bound
tests/test_square_bands_host.py shows a single misplaced line to exceed at least tenfold in every band.

test_hermitian_fold: the signed quadrant masks (a band cut to ky < 0 with kx > 0, or with kx < 0), whose half-plane weights
come from mask(-k) alone, on the transform path and the fused rise walk, log1p|F|.

Figures per size and path, and what a temporary mutation of the row transform did to this file and to the older ones, are in
DESIGN.md, "Square-plane census".
"""
import numpy as np
import pytest

import helicon_amd as H
import spectrum_bands as SB
import square_bands as Q
from tests import sweep_variants as SV

pytestmark = pytest.mark.gpu


def sweep_on(eng, n, path, params, tag):
    """The list's scores on `path`, swept twice with the same bits, after asserting that this path ran."""
    mode, walk = Q.PATHS[path]
    eng.set_table_path(mode)
    eng.set_fused_walk(walk)
    scores = eng.sweep(params)
    ran = (eng.last_first_pass, eng.last_fused_walk, eng.last_factor_sets)
    assert ran == Q.expected(n, path), (tag, path, ran)
    assert np.isfinite(scores).all(), (tag, path)
    assert np.array_equal(scores, eng.sweep(params)), (tag, path, "not bit-reproducible")
    assert (eng.last_first_pass, eng.last_fused_walk, eng.last_factor_sets) == ran, (tag, path)
    return scores


def check_footprint(eng, n, probe, tag):
    """The device's report of the fused pass's shape is the helper's, and each built walk has a resident workgroup."""
    f = eng.fused_walk_footprint(float(probe.rise_column.min()))
    want = Q.footprint(n)
    print(f"{tag}: {len(probe.units)} subunits, footprint {f}")
    assert want is not None and {k: f[k] for k in want} == want, (tag, f, want)
    assert 0 < f["kg"] <= 16 and f["per_cu_rises"] > 0, (tag, f)
    if SV.twist_walk_built(n):
        assert f["per_cu_twists"] > 0, (tag, f)
    else:
        assert f["per_cu_twists"] == 0 and f["lds_twists"] == 0, (tag, f)


def sweep_masks(eng, n, probe, masks, images, log, paths, tag):
    """{path: [masks, segments, candidates] float32}."""
    got = {p: [] for p in paths}
    for b, mask in enumerate(masks):
        eng.set_reference(images, mask, log=log)
        if b == 0:
            check_footprint(eng, n, probe, tag)
        for p in paths:
            got[p].append(sweep_on(eng, n, p, probe.params, (tag, b)))
    return {p: np.stack(v) for p, v in got.items()}


def compare(got, oracles, pick, tag, failures):
    """got[reference][path]: [masks, segments, 32] for the references "image", "image2" and "both"; oracles[image] = (scores
    [masks, picks], tolerance [masks]).  Prints every figure, appends what is out of bounds to `failures`."""
    paths = list(got["both"])
    for ref, g in got.items():
        if "fused/twists" in g and not np.array_equal(g["fused/rises"], g["fused/twists"]):
            failures.append(f"{tag} {ref}: the two fused walks differ by {np.abs(g['fused/rises'] - g['fused/twists']).max():.2e}")
        d = {(p, q): float(np.abs(g[p] - g[q]).max()) for i, p in enumerate(paths) for q in paths[i + 1:]}
        worst = max(d, key=d.get)
        print(f"{tag} {ref}: largest distance between two paths {d[worst]:.2e} ({worst[0]} / {worst[1]})")
        failures += [f"{tag} {ref}: |{p} - {q}| = {v:.2e} > {Q.PATHS_TOL:.0e}" for (p, q), v in d.items() if v > Q.PATHS_TOL]
    for s, single in enumerate(("image", "image2")):
        scores, tol = oracles[s]
        for p in paths:
            seg = float(np.abs(got["both"][p][:, s] - got[single][p][:, 0]).max())
            if seg > Q.SEGMENT_TOL:
                failures.append(f"{tag} {p}: segment {s} of two differs from its single sweep by {seg:.2e} > {Q.SEGMENT_TOL:.0e}")
            for ref, rows in ((single, got[single][p][:, 0]), ("both", got["both"][p][:, s])):
                err = np.abs(rows[:, pick].astype(np.float64) - scores).max(axis=1)                  # [masks]
                b = int(np.argmax(err / tol))
                print(f"{tag} {p} {ref}[{s}]: max |score - oracle| {err.max():.2e} over {len(err)} masks x {len(pick)} candidates "
                      f"(worst against its tolerance: mask {b}, {err[b]:.2e} / {tol[b]:.1e}); segment against single {seg:.2e}")
                if (err > tol).any():
                    failures.append(f"{tag} {p} {ref}[{s}]: |score - oracle| per mask {np.array2string(err, precision=1)} > "
                                    f"tolerance {np.array2string(tol, precision=1)}")


@pytest.mark.parametrize("case", Q.CASES, ids=Q.case_id)
def test_every_band_on_every_path(case):
    n, log, axis = case
    tag = Q.case_id(case)
    assert not Q.UNREACHABLE                       # every form is swept; an entry needs its own assertion here
    probe = Q.probe_of(n)
    masks = SB.band_masks(n, n, axis)
    assert masks.shape == (16, n, n) and len(probe.params) == 32
    refs = {"image": probe.image, "image2": probe.image2, "both": np.stack([probe.image, probe.image2])}
    with H.SweepEngine(n) as eng:
        assert not eng.general
        eng.set_geometry(**probe.geometry())
        got = {ref: sweep_masks(eng, n, probe, masks, imgs, log, list(Q.PATHS), f"{tag} {ref}") for ref, imgs in refs.items()}
    for ref, g in got.items():
        for p, v in g.items():
            assert v.shape == (16, 2 if ref == "both" else 1, 32), (tag, ref, p)                  # no band, no candidate left out
    pick = Q.picks(n)
    oracles = []
    for image in (0, 1):
        o = Q.oracle_side(n, log, axis, image)
        assert o.scores.shape == (16, len(pick)) and (o.tol <= Q.SCORE_TOL).all()
        print(f"{tag} image {image}: float32 floor {o.floor.max():.2e}, tolerance {o.tol.max():.1e}")
        oracles.append((o.scores, o.tol))
    failures = []
    compare(got, oracles, pick, tag, failures)
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("n", Q.SIZES)
def test_hermitian_fold(n):
    tag = f"n{n}-fold"
    probe = Q.probe_of(n)
    f = Q.fold_side(n)
    assert len(f.masks) >= 63 and (f.tol <= Q.SCORE_TOL).all()
    refs = {"image": probe.image, "image2": probe.image2, "both": np.stack([probe.image, probe.image2])}
    with H.SweepEngine(n) as eng:
        eng.set_geometry(**probe.geometry())
        got = {ref: sweep_masks(eng, n, probe, f.masks, imgs, True, ["transform", "fused/rises"], f"{tag} {ref}") for ref, imgs in refs.items()}
    print(f"{tag}: {len(f.masks)} quadrant masks, float32 floor {f.floor.max():.2e}, tolerance {f.tol.max():.1e}")
    failures = []
    compare(got, [(f.scores[0], f.tol), (f.scores[1], f.tol)], f.picks, tag, failures)
    assert not failures, "\n".join(failures)
