"""The case table of the Path A product tests (tests/path_a_product_cases.py) covers what it says it covers: no GPU.  The
device test (tests/test_gpu_path_a_products.py) runs every case of the table; this one holds the table to its axes."""
import numpy as np
import pytest

from tests import path_a_product_cases as C


def test_every_axis_value_occurs():
    for name, values, of in (("box", C.BOXES, lambda c: c.box), ("candidate", C.CANDIDATES, lambda c: c.cand),
                             ("scale", C.SCALES, lambda c: c.scale), ("dy", C.DYS, lambda c: c.dy),
                             ("min_projection_lines", (C.LOW, C.MID, C.ALL), lambda c: c.min_lines),
                             ("min_sym_pairs", C.MIN_SYMS, lambda c: c.min_sym), ("interpolation", ("nn", "linear"), lambda c: c.interp)):
        seen = {of(c) for c in C.CASES}
        assert seen == set(values), (name, seen ^ set(values))
    assert 40 <= len(C.CASES) <= 70 and len(set(C.CASES)) == len(C.CASES)
    # one half-set case per interpolation (the trilinear one with its banded twin), the two deterministic rules
    assert sorted({(c.interp, c.fsc_mode) for c in C.CASES if c.fsc_half}) == [("linear", 4), ("nn", 2)]
    assert sorted(c.fsc_half for c in C.CASES if c.fsc_half) == [1, 2, 2]
    # tilt / psi: two nearest-neighbour cases, nowhere else
    tilted = [c for c in C.CASES if c.tilt or c.psi]
    assert len(tilted) == 2 and all(c.interp == "nn" and c.form == "general" and c.tilt and c.psi for c in tilted)
    # each small box also under the forced banded form
    for box in C.SMALL_BOXES:
        assert any(c.box == box and c.form == "banded" for c in C.CASES), box
        assert any(c.box == box and c.form == "factored" for c in C.CASES), box


def test_every_form_has_its_cases():
    for form in C.FORMS:
        cases = [c for c in C.CASES if c.form == form]
        assert len(cases) >= 4, form
        assert any(c.scale != 1.0 for c in cases), form
        assert any(c.cand in C.QUARTER_TURNS for c in cases), form
    for c in C.CASES:
        assert (c.interp == "nn") == (c.form in ("sliced", "general")), c
        assert not c.force_general or (c.form == "general" and C.stays_sliced(c) and C.slice_fits(c)), c
        if c.form == "lds":
            assert c.box[0] > 128, c          # at D2d <= 128 a trilinear batch takes the separable form
        if c.form == "factored":
            assert C.separable_group(c)[1], c
        if c.form == "banded":
            assert (C.banded_by(c) == "allow") == (not C.separable_group(c)[1]), c
    # the separable form at its last D2d, with groups of four home layers and with the single-layer groups of a large disc
    assert {C.separable_group(c)[0] for c in C.CASES if c.form == "factored" and c.box[0] == 128} == {1, 4}


@pytest.mark.parametrize("c", [c for c in C.CASES if c.interp == "nn"], ids=C.case_id)
def test_nearest_neighbour_cases_name_the_form_the_cpu_derives(c):
    """"Stays sliced" from the oracle's Z: no operation in use and no image column within 1e-9 of a half-integer.  Every
    candidate of a batch must agree, or the sliceable ones would be dragged to the general form unseen."""
    assert c.form == C.expected_nn_form(c)
    if not (c.tilt or c.psi):
        Z = C.axial_coordinates(c, C.oracle_data(c)[3])
        # tilt = psi = 0: a ray has ONE axial coordinate up to the noise of Ry(90)
        assert np.abs(Z - Z[:, :, :1, :1]).max() < 1e-12


@pytest.mark.parametrize("c", C.CASES, ids=C.case_id)
def test_every_case_has_rows(c):
    s = C.oracle_system(c)
    assert s["m_data"] > 0 and s["A"].shape == (s["m_data"] + s["m_sym"], s["n"]) and s["A"].dtype == np.float64
    assert len(s["b"]) == len(s["pid"]) == s["m_data"] and s["ops"] >= 1
    if c.min_lines == C.LOW:
        assert s["ops"] == 1                     # below a single operation's rows
    if c.min_lines == C.ALL:
        tw, rs, cs = c.cand
        from oracle import path_a as A
        assert s["ops"] == len(A.hcsym_order(tw, rs, cs, c.box[4], c.box[1])) and s["m_data"] < C.ALL   # above all of them
    if c.min_lines == C.MID and not c.fsc_half:
        assert s["ops"] > 1 and s["m_data"] > C.MID


def test_the_g22_cases_are_in_the_table():
    assert len(set(C.G22)) == len(C.G22) >= 12
    for c in C.G22:
        assert c in C.CASES and max(c.box) <= 24, c
    for name, values, of in (("box", C.SMALL_BOXES, lambda c: c.box), ("candidate", C.CANDIDATES, lambda c: c.cand),
                             ("scale", C.SCALES, lambda c: c.scale), ("dy", C.DYS, lambda c: c.dy),
                             ("min_projection_lines", (C.LOW, C.MID, C.ALL), lambda c: c.min_lines),
                             ("min_sym_pairs", C.MIN_SYMS, lambda c: c.min_sym), ("interpolation", ("nn", "linear"), lambda c: c.interp)):
        assert {of(c) for c in C.G22} == set(values), name
