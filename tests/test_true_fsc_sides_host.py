"""The true-FSC side census of tests/true_fsc_sides.py, checked on the CPU with the oracle alone: the host Philox against the
published known-answer vectors, the residues SIDES reaches, the preconditions of the comparison at every side, and the
sensitivity of ``compare``: the float32 model of the device's pipeline passes every bound of tests/test_gpu_true_fsc_sides.py,
and with any one of the listed faults it exceeds the bound named here.

Measured: the smallest floor ratio over the 35 sides is 8.3e-4 (the randomised masked pair on the full spectrum at n = 30),
against the standing floor of 1e-4.  The model itself, at 10, 14 and 66: at most 3.4e-8 against the stored spectrum's 2.3e-7 ...
7.0e-7, 5.8e-8 against the map's 9.1e-7 ... 1.6e-6, 8.0e-9 against the 3e-7 and 1.4e-8 against the 9e-7.  Every fault exceeds its
named bound by a factor of 1e3 or more ("True-FSC side census", has the table)."""
import functools

import numpy as np
import pytest

import fsc_oracle as O
import true_fsc_oracle as TO
import true_fsc_sides as S


# ------------------------------------------------------------------------------------------
# the generator
# ------------------------------------------------------------------------------------------
KNOWN_ANSWERS = [     # Random123's kat_vectors, philox4x32 10 rounds: counter, key, output
    ((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
]


def test_philox_reproduces_the_known_answer_vectors():
    for counter, key, want in KNOWN_ANSWERS:
        got = S.philox4x32_10(counter, key)
        assert tuple(int(w) for w in got) == want
    # as arrays: all three at once, every word
    cs = [np.array([kat[0][i] for kat in KNOWN_ANSWERS]) for i in range(4)]
    ks = [np.array([kat[1][i] for kat in KNOWN_ANSWERS]) for i in range(2)]
    got = S.philox4x32_10(cs, ks)
    for i in range(4):
        assert [int(w) for w in got[i]] == [kat[2][i] for kat in KNOWN_ANSWERS]


def test_philox_angles_are_the_generator_of_the_counter_and_both_key_words():
    n, seed = 10, S.GENERATOR_SEED
    t1, t2 = S.philox_angles(n, seed)
    ncol = n // 2 + 1
    assert t1.shape == t2.shape == (n, n, ncol) and t1.dtype == np.float64
    assert (t1 > 0).all() and (t1 < 2 * np.pi).all() and (t2 > 0).all() and (t2 < 2 * np.pi).all()
    for kz, ky, kx, which in ((0, 0, 0, 0), (9, 9, 5, 1), (3, 7, 2, 0), (3, 7, 2, 1)):
        b = (kz * n + ky) * ncol + kx
        word = int(S.philox4x32_10((b, 0, which, 0), (seed & 0xFFFFFFFF, seed >> 32))[0])
        assert (t1, t2)[which][kz, ky, kx] == (word + 0.5) * (2 * np.pi / 2**32)
    # every part of the counter and of the key matters
    assert not np.array_equal(t1, t2)
    assert not np.array_equal(t1, S.philox_angles(n, seed ^ 1)[0]) and not np.array_equal(t1, S.philox_angles(n, seed ^ (1 << 32))[0])
    assert len(np.unique(t1)) == t1.size


# ------------------------------------------------------------------------------------------
# the sides
# ------------------------------------------------------------------------------------------
def test_sides_reach_every_residue_of_the_tiling():
    assert S.SIDES == tuple(range(8, 73, 2)) + (126, 130) and len(S.SIDES) == len(set(S.SIDES)) == 35
    assert all(n % 2 == 0 and 8 <= n <= 512 for n in S.SIDES)
    r = [S.residues(n) for n in S.SIDES]
    assert {v["rows_mod_64"] for v in r} == {0, 4, 16, 36} == {n * n % 64 for n in range(8, 514, 2)}
    assert {v["n_mod_4"] for v in r} == {0, 2}
    assert {v["ncol_side_of_32"] for v in r} == {-1, 0, 1} and {v["ncol_side_of_64"] for v in r} == {-1, 0, 1}
    assert {v["n_side_of_64"] for v in r} == {-1, 0, 1}
    assert set(range(5, 38)) <= {v["ncol"] for v in r} and {64, 66} <= {v["ncol"] for v in r}
    assert {62, 64, 66, 70} <= set(S.SIDES)
    assert {v["ka_mod_32"] for v in r} == set(range(0, 32, 4))          # 2 n mod 32: every value an even n can give
    # the 32-row sub-tile cut both ways, for both classes of n mod 4 where they exist
    assert {(v["rows_mod_64"], v["n_mod_4"]) for v in r} == {(0, 0), (16, 0), (4, 2), (36, 2)}
    # the sides of the generator test and of the sensitivity test are sides of the census
    assert set(S.GENERATOR_SIDES) <= set(S.SIDES) and set(S.FAULT_SIDES) <= set(S.SIDES)
    assert {n * n % 64 for n in S.FAULT_SIDES} == {36, 4} and max(S.FAULT_SIDES) // 2 + 1 > 32
    assert 30 * 30 % 64 == 4 and 30 % 4 == 2


def test_cutoff_rule_never_makes_a_tie():
    for n in range(8, 514, 2):
        q2 = S.q_of(n) ** 2
        assert q2 - np.floor(q2) == (0.25 if n % 4 == 0 else 0.5625 if n % 8 == 2 else 0.0625)     # exact in float64: never 0
        assert S.cutoff(n) > 2 and int(n * S.APIX / S.cutoff(n)) == n // 4
    assert ((30 / 4 + 0.5) ** 2).is_integer()              # the rule of the sides divisible by 4 would tie at n = 4 j + 2


@pytest.mark.parametrize("n", S.SIDES)
def test_preconditions_hold_at_every_side(n):
    ora = S.oracle(n)
    p = S.preconditions(ora, n)
    floors = {k: v for k, v in p.items() if k.startswith("floor_")}
    worst = min(floors, key=floors.get)
    print(f"TFSC_FIGURE sides preconditions n={n} m_cut={ora.m_cut} randomised={p['randomised']} smallest_floor={floors[worst]:.3e} ({worst})")
    assert ora.m_cut == int(np.ceil(S.q_of(n) ** 2)) and p["same_bins"] and p["m_cut_is_ceil"]
    assert min(floors.values()) >= S.FLOOR
    assert S.preconditions_hold(p)


# ------------------------------------------------------------------------------------------
# the model and the sensitivity of compare
# ------------------------------------------------------------------------------------------
def test_weighted_half_sums_are_the_full_spectrum_sums():
    for n in (10, 12):
        a, b, _ = S.inputs(n)
        want = O.sums_3d(a, b, True)
        assert np.abs(S.weighted_half_sums(a, b, n) - want).max() <= 1e-12 * np.abs(want).max()


def test_c2r_tables_are_irfftn_on_a_spectrum_that_is_not_hermitian():
    n = 10
    rng = np.random.RandomState(3)
    F = rng.standard_normal((n, n, n // 2 + 1)) + 1j * rng.standard_normal((n, n, n // 2 + 1))
    cw, sw = S.c2r_tables(n)
    G = np.fft.ifft2(F, axes=(0, 1))
    want = TO.irfftn(F)
    assert np.abs(G.real @ cw + G.imag @ sw - want).max() <= 1e-13 * np.abs(want).max()
    assert not sw[0].any() and not sw[n // 2].any() and cw[0, 0] == 1 / n and abs(cw[1, 0]) == 2 / n
    live = S.c2r_tables(n, "c2r_sine_rows_live")[1]
    assert live[0].any() and live[n // 2].any()


NAMED = {     # fault -> the figure that must exceed its bound
    "spec_last_rows": "spec0_vs_f64",
    "map_last_rows": "map0_vs_f64",
    "sums_last_rows": "unmasked",
    "column_32": "spec0_vs_f64",
    "ky_rows_swapped": "spec0_vs_f64",
    "c2r_nyquist_weight_2": "map0_vs_f64",
    "c2r_sine_rows_live": "map0_vs_f64",
    "full_sums_nyquist_weight_2": "masked_full_fsc_t",
    "angles_of_map_2_for_map_1": "spec0_vs_f64",
    "m_cut_plus_1": "spec0_vs_f64",
    "m_cut_minus_1": "spec0_vs_f64",
}


@functools.lru_cache(maxsize=None)
def _side(n):
    a, b, u = S.inputs(n)
    return n, a, b, u, S.oracle(n)


CASES = [(n, f) for n in S.FAULT_SIDES for f in S.FAULTS if f != "column_32" or n // 2 + 1 > 32]      # column 32 exists at n = 66 only


@pytest.mark.parametrize("n", S.FAULT_SIDES)
def test_the_float32_model_passes_every_bound(n):
    n, a, b, u, ora = _side(n)
    model = S.ModelTrueFSC(a, b, S.APIX, S.cutoff(n), phases=u)
    figs = S.compare(model, ora, n)
    print(f"TFSC_FIGURE sides model n={n} " + S.figure_line(figs))
    assert len(figs) == 28 and S.exceeded(figs) == []
    assert all(b > 0 for k, (v, b) in figs.items() if not k.endswith(("_bits", "_form")) and k not in ("cutoff", "true_fsc_is_corrected"))


def test_named_faults_are_the_listed_ones():
    assert set(NAMED) == set(S.FAULTS) and len(S.FAULTS) == 11
    assert {f for _, f in CASES} == set(S.FAULTS) and len(CASES) == 3 * 11 - 2


@pytest.mark.parametrize("n,fault", CASES)
def test_every_fault_exceeds_its_named_bound(n, fault):
    n, a, b, u, ora = _side(n)
    model = S.ModelTrueFSC(a, b, S.APIX, S.cutoff(n), phases=u, fault=fault)
    if fault in ("m_cut_plus_1", "m_cut_minus_1"):
        # m_cut or m_cut - 1 may be no sum of three squares (15 at n = 14, 7 at n = 10): then the fault selects the same bins,
        # there is nothing to see, and the other direction must be live
        if np.array_equal(model.sel_used, TO.m_half(n) >= ora.m_cut):
            other = "m_cut_minus_1" if fault == "m_cut_plus_1" else "m_cut_plus_1"
            twin = S.ModelTrueFSC(a, b, S.APIX, S.cutoff(n), phases=u, fault=other)
            assert not np.array_equal(twin.sel_used, TO.m_half(n) >= ora.m_cut)
            return
    figs = S.compare(model, ora, n)
    over = S.exceeded(figs)
    name = NAMED[fault]
    v, bound = figs[name]
    print(f"TFSC_FIGURE sides fault n={n} {fault}: {name}={v:.3e} bound={bound:.3e}; all exceeded: {' '.join(over)}")
    assert name in over, (fault, n, S.FAULTS[fault], figs)


def test_the_model_is_not_blind_where_the_old_checks_were():
    """A misplaced block that keeps amplitudes (two ky rows swapped in the store, the plain spectrum's too) passes the checks
    that compare the pipeline with itself; only the float64 figure of the stored spectrum and what follows the store see it."""
    n = 14
    a, b, u = S.inputs(n)
    ora = TO.OracleTrueFSC(a, b, S.APIX, S.cutoff(n), phases=u)
    figs = S.compare(S.ModelTrueFSC(a, b, S.APIX, S.cutoff(n), phases=u, fault="ky_rows_swapped"), ora, n)
    over = set(S.exceeded(figs))
    assert "spec0_vs_f64" in over and "spec1_vs_f64" in over
    assert not {"unmasked", "randomised_unmasked", "spec0_amp_rel", "spec1_amp_rel", "masked_half_fsc_t", "masked_full_fsc_t"} & over
