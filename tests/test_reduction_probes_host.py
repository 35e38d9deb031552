"""Host side of the reduction probes (tests/reduction_probes.py; the device side is tests/test_gpu_reduction_probes.py).  No
device is needed: every probe's reference runs and the comparison accepts it, each probe reaches the seam its rule names, the
NumPy restatements of the kernels' decomposition (64 lanes, the block size, the grid cap, per-thread ascending order) reproduce
the yardstick with no rule changed, and every wrong-rule variant is bitten by a probe listed for it — it changes an exactly
compared item (an index, a bit pattern, a NaN position, an exact zero) or moves a score by at least 100 times its bound — so the
device test would notice the same defect in a kernel.  hh_argmax is host code: its rows are checked here, exactly.  Where
arithmetic rules a bite out, that is asserted too."""
import ctypes as C

import numpy as np
import pytest

import reduction_probes as Q
from helicon_amd import _lib

F32 = np.float32


def _of(*kinds):
    return [p for p in Q.PROBES if p.kind in kinds]


def test_every_reference_runs_and_the_comparison_accepts_it():
    assert len(Q.PROBES) > 1500
    kinds = {p.kind for p in Q.PROBES}
    assert kinds == {"pearson", "cosine", "argmax", "argmax_host", "argmax_refusal", "threshold"}
    for p in Q.PROBES:
        inp = p.inputs()
        ref = Q.reference(p, inp)
        v = Q.compare(p, ref, ref, inp)
        assert v.ok and not v.bitten(), p.name
        if p.kind in ("pearson", "cosine"):
            assert np.isfinite(ref) and abs(ref) <= 1 + Q.pair_bound(p.args["n"]), p.name
            assert inp["a"].size == p.args["n"] == inp["b"].size, p.name
            if p.args.get("exact_zero"):
                assert ref == 0, p.name
            if "closed" in p.args:                                   # the closed forms: +-1 and 0
                assert abs(ref - p.args["closed"]) <= Q.pair_bound(p.args["n"]), (p.name, ref)
        elif p.kind in ("argmax", "argmax_host"):
            np.testing.assert_array_equal(ref, inp["expect"], err_msg=p.name)     # the yardstick gives what each row was built to give
        elif p.kind == "threshold":
            assert ref.dtype == F32 and ref.shape == inp["data"].shape, p.name


def test_the_lengths_reach_every_seam_of_the_grid_stride_kernels():
    assert Q.TRIP == 262144 and Q.grid_of(Q.TRIP) == 1024 and Q.trips_of(Q.TRIP) == 1
    assert Q.trips_of(Q.TRIP + 1) == 2 and Q.trips_of(2 * Q.TRIP + 7) == 3          # the second and third grid-stride trips exist
    assert Q.place_of(Q.TRIP, Q.TRIP + 1) == (1, 0, 0, 0) and Q.place_of(Q.TRIP - 1, Q.TRIP + 1) == (0, 1023, 3, 63)
    assert Q.place_of(2 * Q.TRIP + 6, 2 * Q.TRIP + 7) == (2, 0, 0, 6)
    assert Q.place_of(63, 65) == (0, 0, 0, 63) and Q.place_of(64, 65) == (0, 0, 1, 0)   # the last lane of a wavefront, the first of the next
    assert Q.place_of(255, 257) == (0, 0, 3, 63) and Q.place_of(256, 257) == (0, 1, 0, 0)  # the last lane of a block, the first of the next
    assert Q.grid_of(3) == 1 and Q.place_of(2, 3) == (0, 0, 0, 2)                     # n = 3: three wavefronts of the block hold no element
    assert {n % 256 for n in Q.LENGTHS} >= {0, 1, 255, 7} and Q.chain_length(2 * Q.TRIP + 7) == 3 + 10 + 1024
    assert Q.pair_bound(2 * Q.TRIP + 7) < 1e-12 and Q.pair_bound(1) == 8 * 12 * 2.0 ** -53
    for kind, lengths in (("pearson", Q.LENGTHS), ("cosine", Q.LENGTHS), ("threshold", Q.LENGTHS)):
        assert {p.args["n"] for p in _of(kind)} >= set(lengths), kind
    # every seam index below n carries a spike (pearson) and a maximum (threshold) at every length
    for n in Q.LENGTHS:
        seams = {i for i in (0, 63, 64, 255, 256, n - 1, 262143, 262144) if i < n}
        if n >= 2:
            assert {p.args["spike"] for p in _of("pearson") if p.args["n"] == n and "spike" in p.args} == seams, n
        for tag in ("max", "negmax"):
            assert {p.args["pos"] for p in _of("threshold") if p.args["n"] == n and p.args["tag"] == tag} == seams, (n, tag)
        modes = {(p.args["mode"], p.args["thresh"]) for p in _of("threshold") if p.args["n"] == n and p.args["tag"] == "mixed"}
        assert modes == {("fraction", 0.0), ("fraction", 0.3), ("fraction", 0.5), ("fraction", 1.0), ("value", 0.5), ("value", -0.25)}


def test_the_pair_probes_reach_what_they_name():
    """A spike's score hangs on its one element: the yardstick without it, or with it twice, is far outside the bound."""
    for p in _of("pearson", "cosine"):
        if "spike" not in p.args or (p.args["n"] > 513 and p.args["spike"] < Q.TRIP - 1):
            continue
        inp, i, bound = p.inputs(), p.args["spike"], Q.pair_bound(p.args["n"])
        want = Q.reference(p, inp)
        a, b = inp["a"], inp["b"]
        assert a[i] == b[i] and a[i] >= 4 and np.abs(np.delete(a, i)).max() <= 0.5, p.name
        if a.size < 63:                                               # (two or three points: any line through them scores +-1)
            continue
        assert abs(Q.pair_yardstick(p.kind, np.delete(a, i), np.delete(b, i)) - want) > 1e6 * bound, p.name
        assert abs(Q.pair_yardstick(p.kind, np.insert(a, i, a[i]), np.insert(b, i, b[i])) - want) > 1e6 * bound, p.name
    for kind in ("pearson", "cosine"):
        inp = Q.BY_NAME[f"{kind}/noise/n{Q.TRIP + 1}/mixed"].inputs()
        assert inp["a"].dtype == F32 and inp["b"].dtype == np.float64                 # _pair sends the pair through the f64 entry
        inp = Q.BY_NAME[f"{kind}/noise/n257/f64"].inputs()
        for v in inp.values():
            assert v.dtype == np.float64 and (v.astype(F32).astype(np.float64) != v).all()   # not representable in float32
        inp = Q.BY_NAME[f"{kind}/view2d/n3840/f32"].inputs()
        assert inp["a"].shape == (48, 80) and not inp["a"].flags.c_contiguous
        masked = [p for p in _of(kind) if "/masked/" in p.name]
        assert len(masked) == 1 and masked[0].inputs()["a"].shape == (int(Q.O.radial_band_mask(64, 64).sum()),)
    for p in _of("pearson"):
        if "/constant/" in p.name:
            b = p.inputs()["b"]
            assert (b == 2.5).all() and b.dtype == p.inputs()["a"].dtype                # a float32 / dyadic constant: n * 2.5 is exact in float64
    assert Q.reference(Q.BY_NAME["pearson/noise/n1/f32"]) == 0 and Q.reference(Q.BY_NAME["pearson/noise/n1/f64"]) == 0
    assert abs(abs(Q.reference(Q.BY_NAME["cosine/noise/n1/f32"])) - 1) < 1e-15
    # where the two forms of the norm part: the product of the sums leaves the float64 range, each root does not
    assert Q.reference(Q.BY_NAME["pearson/huge/n257/f64"]) == 0 and Q.reference(Q.BY_NAME["pearson/tiny/n257/f64"]) == 0
    assert 0.1 < abs(Q.reference(Q.BY_NAME["cosine/huge/n257/f64"])) < 0.9 and 0.1 < abs(Q.reference(Q.BY_NAME["cosine/tiny/n257/f64"])) < 0.9


def test_the_argmax_probes_reach_what_they_name():
    assert {p.args["n"] for p in _of("argmax")} >= set(Q.ARG_N) and {len(p.args["cases"]) for p in _of("argmax")} == {1, 5, Q.ROW_CAP}
    assert {p.args["route"] for p in _of("argmax")} == {"d", "h"}
    for n in Q.ARG_N:
        tags = {c for p in _of("argmax") if p.args["n"] == n for c in p.args["cases"]}
        assert {c[1] for c in tags if c[0] == "max"} == {i for i in (0, 63, 64, 1023, 1024, n - 1) if i < n}, n
        ties = {c[1:] for c in tags if c[0] == "tie"}
        assert ties >= {pair for pair in ((63, 64), (5, 1029), (1023, 1024)) if pair[1] < n}, n
        assert (5 % Q.ARG_BLOCK == 1029 % Q.ARG_BLOCK) and 1023 // Q.LANES == 15 and 1024 % Q.ARG_BLOCK == 0   # one thread's trips; the block's ends
        need = {"all_nan", "ninf_all"} | ({"zeros_pm", "zeros_mp", "inf_tie", "nan0_equal", "nan_ninf", "nan_after_max"} if n >= 2 else set())
        assert {c[0] for c in tags} >= need, n
        for rows in Q.ARG_ROWS:
            assert {p.args["ld"] for p in _of("argmax") if p.args["n"] == n and len(p.args["cases"]) == rows} == ({0} if rows == 1 else {0, n + 1, n + 37})
        # the five-row probes carry every case of the length between them, under every stride
        for ld in (0, n + 1, n + 37):
            assert {c for p in _of("argmax") if p.args["n"] == n and p.args["ld"] == ld and len(p.args["cases"]) == 5 for c in p.args["cases"]} == tags
    for p in _of("argmax"):
        inp, n, ld = p.inputs(), p.args["n"], p.args["ld"]
        s = inp["scores"]
        assert s.shape == (len(p.args["cases"]), ld or n) and s.dtype == F32, p.name
        if ld:                                                        # the padding would win if it were read
            pad, row = s[:, n:], s[:, :n]
            assert np.isinf(pad[:, 0]).all() and (pad[:, 0] > 0).all() and (ld - n < 2 or np.isnan(pad[:, 1]).all()), p.name
            finite = np.where(np.isfinite(row), row, -np.inf).max(axis=1)
            assert (finite <= 9).all() and (row[np.isfinite(row)] < np.inf).all(), p.name
    for p in _of("argmax", "argmax_host"):
        scores = p.inputs()["scores"]
        for r, case in enumerate(p.args["cases"][:64]):
            row = scores[r, :p.args["n"]]
            if case[0] == "zeros_pm":
                assert row[case[1]] == 0 and not np.signbit(row[case[1]]) and np.signbit(row[case[2]]) and row[case[2]] == 0 and (np.delete(row, case[1:]) < 0).all()
            elif case[0] == "nan_ninf":
                assert np.isnan(row[:case[1]]).all() and row[case[1]] == -np.inf and set(np.unique(row[~np.isnan(row)])) == {-np.inf}
            elif case[0] == "nan_after_max":
                assert np.isnan(row[case[1] + 1]) and row[case[1]] == np.nanmax(row)
    cap = Q.BY_NAME[f"argmax/r{Q.ROW_CAP}/n3/ld4/d/cap"]
    assert cap.inputs()["scores"].shape == (65535, 4) and cap.inputs()["scores"].nbytes <= 4 << 20
    assert {p.args["bad"] for p in _of("argmax_refusal")} == {(65536, 5, 0), (2, 5, 4), (2, 0, 0)}


def test_the_threshold_probes_reach_what_they_name():
    x = Q.BY_NAME["threshold/negzero_max/n2/fraction0.5"].inputs()["data"]
    assert x.tolist() == [-1.0, -0.0] and np.signbit(x[1])
    ref = Q.reference(Q.BY_NAME["threshold/negzero_max/n2/fraction0.5"])
    assert ref.tolist() == [0.0, 0.0] and not np.signbit(ref).any()               # what NumPy gives: t = -0.0, clip to it, subtract it
    np.testing.assert_array_equal(ref, Q.O.threshold_data(x, thresh_fraction=F32(0.5)))
    for p in _of("threshold"):
        inp, a = p.inputs(), p.args
        x, ref = inp["data"], Q.reference(p, inp)
        assert x.dtype == F32 and x.size == a["n"] and x.nbytes <= 4 << 20, p.name
        tag, m = a["tag"], np.max(x)
        if tag != "nan":                                              # the yardstick is the oracle's threshold_data on float32 data
            kw = dict(thresh_fraction=F32(a["thresh"])) if a["mode"] == "fraction" else dict(thresh_value=F32(a["thresh"]))
            assert ref.tobytes() == Q.O.threshold_data(x, **kw).astype(F32).tobytes(), p.name
        if tag == "pos":
            assert x.min() > 0
        elif tag == "mixed":
            assert (x.min() < 0 < m) or a["n"] < 3
        elif tag in ("neg", "negmax"):
            assert m < 0                                              # the whole array is below zero
        elif tag == "neg_zero":
            assert m == 0 and not np.signbit(m) and (x == 0).sum() == 1 and (np.delete(x, a["n"] // 2) < 0).all()
        elif tag == "zeros":
            assert not x.any() and not np.signbit(x).any()
        elif tag == "negzero_max":
            assert m == 0 and np.signbit(x[-1]) and (x[:-1] == -1).all()
        elif tag == "all_negzero":
            assert not x.any() and np.signbit(x).all()
        elif tag == "wave_neg":
            w = Q.wavefront_maxima(x)
            assert w[0] < 0 and (w[1:] > 0).all() and w.size >= 2
        if tag in ("max", "negmax"):
            assert np.argmax(x) == a["pos"] and (np.delete(x, a["pos"]) < m - 0.9).all(), p.name
            assert ref[a["pos"]] == max(m, 0) * 0.5 and not np.delete(ref, a["pos"]).any(), p.name     # everything below the threshold but the maximum
            if a["n"] > 1:                                            # a maximum that is missed shows at its own position
                missed = Q.threshold_numpy(x, a["mode"], a["thresh"], vmax=lambda h, x=x, i=a["pos"]: np.max(np.delete(x, i)))
                assert missed[a["pos"]] != ref[a["pos"]], p.name
        if tag == "nan":
            assert np.isnan(x).sum() == 1 and np.isnan(x[a["pos"]])
            if a["mode"] == "fraction":
                assert np.isnan(ref).all(), p.name                    # np.max is NaN: NaN everywhere
            else:
                assert np.isnan(ref).sum() == 1 and np.isnan(ref[a["pos"]]), p.name
        # no probe asks for the sign of a zero that IEEE leaves open: a zero element never meets a threshold that is the other zero
        with np.errstate(invalid="ignore"):
            t = F32(m) * F32(a["thresh"]) if a["mode"] == "fraction" else F32(a["thresh"])
        if t == 0:
            assert (np.signbit(x[x == 0]) == np.signbit(t)).all(), p.name


def test_the_restatements_are_the_yardstick():
    """What the variants change one rule of: with no rule changed the kernels' decomposition gives the yardstick — the pair sums
    to the derived bound (another order of float64 additions), the arg-max and the maximum exactly."""
    worst = 0.0
    for p in _of("pearson", "cosine"):
        inp = p.inputs()
        v = Q.compare(p, Q.pair_kernel_numpy(p.kind, inp["a"], inp["b"]), Q.reference(p, inp), inp)
        worst = max(worst, v.figure / v.bound)
        assert v.ok, (p.name, v)
    print(f"pair sums in the kernel's order against math.fsum: at most {worst:.3f} of the bound")
    for p in _of("argmax"):
        inp = p.inputs()
        s = inp["scores"] if len(p.args["cases"]) <= 5 else np.concatenate([inp["scores"][:256], inp["scores"][-256:]])
        np.testing.assert_array_equal(Q.argmax_kernel_numpy(s, p.args["n"], p.args["ld"]), Q.argmax_numpy(s, p.args["n"]), err_msg=p.name)
    for p in _of("threshold"):
        inp = p.inputs()
        got = Q.threshold_numpy(inp["data"], p.args["mode"], p.args["thresh"], vmax=Q.max_by_key)
        assert Q.compare(p, got, Q.reference(p, inp), inp).ok, p.name
        if not np.isnan(inp["data"]).any():
            assert F32(Q.max_by_key(inp["data"])).tobytes() == F32(np.max(inp["data"])).tobytes(), p.name   # -0.0 stays -0.0


def _host_argmax(scores, n):
    L = _lib.lib()
    out = np.full(scores.shape[0], -7, dtype=np.int64)
    idx = C.c_int64(-7)
    for r in range(scores.shape[0]):
        row = np.ascontiguousarray(scores[r, :n])
        assert L.hh_argmax(row.ctypes.data_as(C.POINTER(C.c_float)), n, C.byref(idx)) == 0
        out[r] = idx.value
    return out


def test_hh_argmax_gives_every_row_of_its_probes_exactly():
    probes = _of("argmax_host")
    assert len(probes) > 150
    for p in probes:
        inp = p.inputs()
        v = Q.compare(p, _host_argmax(inp["scores"], p.args["n"]), Q.reference(p, inp), inp)
        assert v.ok, (p.name, p.rule, v)
    L = _lib.lib()
    row, idx = np.array([1, 3, 2], dtype=F32), C.c_int64(-7)
    ptr = row.ctypes.data_as(C.POINTER(C.c_float))
    assert L.hh_argmax(ptr, 0, C.byref(idx)) != 0 and L.hh_argmax(None, 3, C.byref(idx)) != 0 and L.hh_argmax(ptr, 3, None) != 0
    assert idx.value == -7                                            # a refused call writes nothing
    assert L.hh_argmax(ptr, 3, C.byref(idx)) == 0 and idx.value == 1  # and the next one is served


@pytest.mark.parametrize("name", list(Q.VARIANTS))
def test_every_variant_is_bitten_by_a_probe_listed_for_it(name):
    v = Q.VARIANTS[name]
    assert v.probes, name
    bitten = []
    for pname in v.probes:
        p = Q.BY_NAME[pname]
        inp = p.inputs()
        verdict = Q.compare(p, v.run(p, inp), Q.reference(p, inp), inp)
        if verdict.bitten():
            assert not verdict.ok
            bitten.append((pname, verdict.mismatches, verdict.figure, verdict.bound))
    print(f"{name}: bitten by {len(bitten)} of {len(v.probes)} listed probes, e.g. " +
          "; ".join(f"{n} (exact items {m}, moved {f:.3g} against {b:.3g})" for n, m, f, b in bitten[:3]))
    assert bitten, name


def test_what_no_probe_can_bite_by_arithmetic():
    """A dyadic fraction (0, 0.5, 1) times a float32 maximum is exact in float32 and in float64 alike: only 0.3 can tell where the
    fraction is applied.  The two forms of the norm agree to a few ulp wherever sxx syy stays inside the float64 range: only the
    huge / tiny probes tell them apart.  A stride taken as n cannot show on one row or on a dense array; a row read to ld cannot
    show where ld = 0.  The maximum itself is free of order: any decomposition of k_array_max gives the same bits."""
    v = Q.VARIANTS["threshold: the fraction applied in float64"]
    for p in _of("threshold"):
        if p.args["mode"] == "fraction" and p.args["thresh"] != 0.3 and p.args["n"] <= 1025:
            inp = p.inputs()
            assert Q.compare(p, v.run(p, inp), Q.reference(p, inp), inp).ok, p.name
    for name in ("pearson: sqrt(sxx) sqrt(syy)", "cosine: sqrt(sxx syy)"):
        v = Q.VARIANTS[name]
        for p in _of(name.split(":")[0]):
            if "/huge/" not in p.name and "/tiny/" not in p.name and p.args["n"] <= 1025:
                inp = p.inputs()
                assert Q.compare(p, v.run(p, inp), Q.reference(p, inp), inp).ok, p.name
    for p in _of("argmax"):
        if p.args["n"] <= 1025 and (len(p.args["cases"]) == 1 or not p.args["ld"]):
            inp = p.inputs()
            for name in ("argmax: ld taken as n",) + (("argmax: a row read to ld",) if not p.args["ld"] else ()):
                assert Q.compare(p, Q.VARIANTS[name].run(p, inp), Q.reference(p, inp), inp).ok, (name, p.name)
    for p in _of("threshold"):
        if p.args["tag"] in ("mixed", "neg", "negzero_max") and p.args["mode"] == "fraction" and p.args["thresh"] == 0.5 and p.args["n"] <= Q.TRIP + 1:
            x = p.inputs()["data"]
            w = Q.wavefront_maxima(x)
            assert F32(np.max(w)).tobytes() == F32(np.max(x)).tobytes() == F32(np.max(x[::-1])).tobytes(), p.name
