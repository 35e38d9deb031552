"""NumPy models of what the pair path of the fused twist walk (N = 512) does with lanes, slots and masks.  No GPU.

The register hand-over: after the build, lane t of a wavefront holds the sums of columns x = 256 h + 4 t + c in
register (h, c); two lane swaps per register pair turn that into x = 64 m + j' in register m of lane L, with
j' = 4 (L & 15) + (L >> 4).  The first exchange then keeps element o = 8 j' + r in slot(o); the model checks that the
slots are a permutation inside the row's 516 slots, that every ds_write_b64 group of 16 lanes hits 16 bank pairs, that
the two-base form of the writer and of the reader are the same map, and that the reader's groups do not collide either.

The masks of tests/test_gpu_pair_handover.py: each has weight, each has the dead 64-bin groups it is there for, and the
synthetic truth leads on the default band at that file's grid (oracle alone).

(One reduction tree for the six sums of a pair and the skipping of groups without weight were built, measured and
dropped — DESIGN.md section 4, "Register hand-over" — so there is no lane-class model of that tree here; the mask cases stay,
as inputs that send the epilogue's weights every way.)
"""
import numpy as np
import pytest

from oracle import path_b as O
from tests import pair_handover_cases as C

N, T, BROW = 512, 64, 516
LANES = np.arange(64)


# ---- the lane map ---------------------------------------------------------------------------------------------------------
def swap32(d, s):
    """v_permlane32_swap_b32: lanes 32-63 of d <-> lanes 0-31 of s."""
    d, s = d.copy(), s.copy()
    d[32:], s[:32] = s[:32].copy(), d[32:].copy()
    return d, s


def swap16(d, s):
    """v_permlane16_swap_b32: the odd 16-lane rows of d <-> the even rows of s."""
    d, s = d.copy(), s.copy()
    for row in (0, 2):
        lo, hi = slice(16 * row, 16 * row + 16), slice(16 * row + 16, 16 * row + 32)
        d[hi], s[lo] = s[lo].copy(), d[hi].copy()
    return d, s


def transposed_registers():
    """reg[4 h + c][lane] = the column the register holds, after the kernel's swaps."""
    reg = [256 * (i // 4) + 4 * LANES + (i % 4) for i in range(8)]
    for h4 in (0, 4):
        reg[h4], reg[h4 + 2] = swap32(reg[h4], reg[h4 + 2])
        reg[h4 + 1], reg[h4 + 3] = swap32(reg[h4 + 1], reg[h4 + 3])
        reg[h4], reg[h4 + 1] = swap16(reg[h4], reg[h4 + 1])
        reg[h4 + 2], reg[h4 + 3] = swap16(reg[h4 + 2], reg[h4 + 3])
    return reg


def jprime(lane):
    return 4 * (lane & 15) + (lane >> 4)


def test_two_swap_steps_give_every_lane_the_inputs_of_one_butterfly():
    reg = transposed_registers()
    for m in range(8):
        assert np.array_equal(reg[m], 64 * m + jprime(LANES))


def test_jprime_enumerates_every_butterfly_once():
    assert sorted(jprime(LANES)) == list(range(64))


# ---- the first exchange's slots -------------------------------------------------------------------------------------------
def slot(o):
    a, w = o >> 5, o & 31
    return 32 * a + (a >> 2) + (w ^ (4 * (a & 3)))


def writer_slot(lane, r):
    """The kernel's form: two lane bases, the immediates r."""
    al, u = lane & 15, lane >> 4
    base = 32 * al + (al >> 2) + 16 * (u >> 1) + 8 * ((u ^ (al >> 1)) & 1)
    return np.where(r < 4, base + 4 * (al & 1), base - 4 * (al & 1)) + r


def reader_slot(t, m):
    """Element n = t + 64 m: two lane bases, the immediates 64 m + (m >> 1)."""
    e0 = t ^ ((t >> 5) << 2)
    return (e0 ^ 8 if m & 1 else e0) + 64 * m + (m >> 1)


def test_slots_are_a_permutation_inside_the_row():
    s = slot(np.arange(N))
    assert len(set(s.tolist())) == N and s.min() >= 0 and s.max() < BROW


def test_writer_form_is_the_slot_map_and_store_groups_hit_16_bank_pairs():
    for r in range(8):
        s = writer_slot(LANES, r)
        assert np.array_equal(s, slot(8 * jprime(LANES) + r))
        for g in range(4):   # ds_write_b64: four groups of 16 consecutive lanes, bank pair = slot mod 16
            assert len(set((s[16 * g:16 * g + 16] % 16).tolist())) == 16, (r, g)


def test_reader_finds_element_n_without_conflicts():
    for m in range(8):
        s = reader_slot(LANES, m)
        assert np.array_equal(s, slot(LANES + 64 * m))
        for half in range(2):   # ds_read_b64: two groups of 32 lanes over 64 banks = 32 slots
            assert len(set((s[32 * half:32 * half + 32] % 32).tolist())) == 32, (m, half)
        for g in range(4):      # ds_read2_b64: groups of 16 lanes over 32 banks = 16 slots
            assert len(set((s[16 * g:16 * g + 16] % 16).tolist())) == 16, (m, g)


# ---- the masks ------------------------------------------------------------------------------------------------------------
def live_groups(mask):
    """[N/2 + 1, 8] bool: spectrum row ky (0 .. N/2) has a weighted bin among kx = 64 m .. 64 m + 63 (unshifted)."""
    return folded(mask).reshape(N // 2 + 1, 8, 64).any(axis=2)


def folded(mask):
    """The engine's Hermitian weights as a bool: mask(k) or mask(-k) on rows 0 < ky < N/2, mask(k) on rows 0 and N/2."""
    m = np.fft.ifftshift(np.asarray(mask, dtype=bool))
    neg = np.roll(m[::-1, ::-1], (1, 1), axis=(0, 1))       # neg[ky, kx] = m[-ky, -kx]
    w = m | neg
    w[0], w[N // 2] = m[0], m[N // 2]
    return w[: N // 2 + 1]


@pytest.mark.parametrize("name", list(C.MASKS))
def test_masks_have_weight_and_the_dead_groups_they_are_there_for(name):
    mask = C.MASKS[name]()
    assert mask.shape == (N, N) and mask.any()
    live = live_groups(mask)
    rows = live.any(axis=1)
    if name == "default":
        dead = (~live[rows]).sum() / live[rows].size
        assert 0.10 < dead < 0.16          # the eighth of the evaluated bins that sit in groups without weight
        assert live[1].all() and not live[240, 3] and not live[240, 4]
    elif name == "low_band":
        inner = np.arange(1, 57)
        assert (live[inner][:, [0, 7]]).all() and not live[inner][:, 1:7].any()
    elif name == "high_band":
        assert not live[1:100][:, [0, 7]].any() and live[1:100][:, [3, 4]].all()
    elif name == "layer_lines":
        half = folded(mask).reshape(N // 2 + 1, 8, 64)
        assert set(np.unique(half[rows].sum(axis=2)).tolist()) <= {0, 1, 2, 3}
        assert (half[rows].sum(axis=2) == 1).any()
    elif name == "kx_positive":
        w = folded(mask)
        assert not w[1:N // 2, 0].any() and w[100, 1:200].all() and w[100, -199:].all()   # the fold fills kx < 0 in
    elif name == "quadrant":
        assert live[100, :4].all() and not live[1:N // 2, 4:].any()
    elif name == "row_emptied":
        assert not live[C.EMPTIED_ROW].any() and live[C.EMPTIED_ROW - 1].any() and live[C.EMPTIED_ROW + 1].any()
    elif name == "block_0_only":
        assert rows[:8].any() and not rows[8:].any()


def test_truth_leads_on_the_default_band_at_the_tests_grid():
    twists, rises = C.TWISTS5, C.RISES8
    img = C.oracle_image()
    params = np.array([(tw, rs, 1) for tw in twists for rs in rises], dtype=np.float64)
    ref = O.sweep_cpu(img, params, O.radial_band_mask(N, N), apix=1.0, helical_diameter=0.4 * N, ball_radius=2.0)
    best = int(np.argmax(ref))
    assert (params[best, 0], params[best, 1]) == pytest.approx(C.TRUTH[:2])
