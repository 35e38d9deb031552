"""Host arithmetic of the fused sweep's twist walk (no device): the schedule with the roles swapped, the LDS footprint of
both walks, and the choice between them (hh_fused_schedule, hh_fused_lds_bytes, hh_fused_walk_choice)."""
import ctypes as C

import numpy as np
import pytest

from helicon_amd import _lib


def schedule(runs, run_len, n_kb, slots):
    out = (C.c_int32 * 6)()
    assert _lib.lib().hh_fused_schedule(runs, run_len, n_kb, slots, out) == 0
    return [int(v) for v in out]


def choice(runs, run_len, n_kb, slots_r, slots_t, mode=0):
    out = (C.c_int64 * 15)()
    assert _lib.lib().hh_fused_walk_choice(runs, run_len, n_kb, slots_r, slots_t, mode, out) == 0
    v = [int(x) for x in out]
    return dict(walk=v[0], cost_rises=v[1], rises=v[2:8], cost_twists=v[8], twists=v[9:15])


@pytest.mark.parametrize("twists, rises", [(400, 250), (50, 250)], ids=["C2", "an eighth of C2"])
def test_swapped_schedule_covers_every_rise_and_run_once(twists, rises):
    """The twist walk calls the schedule with rises as the "runs" and the number of runs as the length; the kernel's
    decoding of a layer (k_fused_pass: region, rise, first run, runs) must visit every (rise, run) exactly once."""
    n_kb, slots = 32, 512
    rises_a, groups_a, cpw_a, groups_b, cpw_b, layers = schedule(rises, twists, n_kb, slots)
    assert layers == rises_a * groups_a + (rises - rises_a) * groups_b
    seen = np.zeros((rises, twists), dtype=np.int32)
    for gy in range(layers):
        la = rises_a * groups_a
        if gy < la:
            rise, off, cpw = gy // groups_a, (gy % groups_a) * cpw_a, cpw_a
        else:
            rise, off, cpw = rises_a + (gy - la) // groups_b, ((gy - la) % groups_b) * cpw_b, cpw_b
        nc = min(cpw, twists - off) if rise < rises else 0
        assert nc > 0
        seen[rise, off:off + nc] += 1
    assert (seen == 1).all()
    if twists == 400:
        # 250 x 32 = 8000 workgroups of 400 runs: 15 whole rounds of 512 hold 240 rises, the last 10 rises go in pieces
        assert (rises_a, groups_a, cpw_a) == (240, 1, 400) and groups_b > 1 and cpw_b < 400


def test_lds_footprint_of_both_walks():
    """C2 (N = 512, 135 table rows -> 140 staged, kg 7): panel 8 x 516 x 8 = 33,024 B, a slice 8 x 140 x 8 = 8,960 B, a
    factor set 7 x 2,048 + 132 x 4 = 14,864 B.  Rises: 33,024 + 8,960 + 2 x 14,864 = 71,712; twists: 33,024 + 2 x 8,960 +
    14,864 = 65,808.  Two workgroups of either fit the 163,840 B of a compute unit."""
    L = _lib.lib()
    assert L.hh_fused_lds_bytes(512, 140, 7, 1) == 71712
    assert L.hh_fused_lds_bytes(512, 140, 7, 2) == 65808
    assert 163840 // 71712 == 2 and 163840 // 65808 == 2
    # a long, thin table (ball radius 0.8 at rise 1.85: 284 staged rows, kg 7): the doubled slice outweighs the saved set —
    # rises 33,024 + 18,176 + 29,728 = 80,928 (two per compute unit), twists 33,024 + 36,352 + 14,864 = 84,240 (one)
    assert L.hh_fused_lds_bytes(512, 284, 7, 1) == 80928 and L.hh_fused_lds_bytes(512, 284, 7, 2) == 84240
    assert 163840 // 80928 == 2 and 163840 // 84240 == 1
    # N = 256: panel 8 x 260 x 8 = 16,640, set 7 x 1,024 + 68 x 4 = 7,440
    assert L.hh_fused_lds_bytes(256, 76, 7, 1) == 16640 + 4864 + 2 * 7440
    assert L.hh_fused_lds_bytes(256, 76, 7, 2) == 16640 + 2 * 4864 + 7440
    # N = 1024 has no twist walk
    assert L.hh_fused_lds_bytes(1024, 140, 7, 2) == 0 and L.hh_fused_lds_bytes(1024, 140, 7, 1) > 0
    assert L.hh_fused_lds_bytes(500, 140, 7, 1) < 0 and L.hh_fused_lds_bytes(512, 140, 7, 3) < 0


def test_choice_of_the_walk():
    # C2: the twist walk's estimate (15 rounds of 400 + 4, then the pieces) is not above the rise walk's 25 x 254
    c2 = choice(400, 250, 32, 512, 512)
    assert c2["walk"] == 2 and c2["cost_rises"] == 25 * 254 and c2["cost_twists"] <= c2["cost_rises"]
    assert c2["twists"][:3] == [240, 1, 400]
    # fewer resident twist-walking workgroups than rise-walking ones, or none: rises, forced or not
    for slots_t in (256, 0):
        for mode in (0, 2):
            assert choice(400, 250, 32, 512, slots_t, mode)["walk"] == 1
    assert choice(400, 250, 32, 512, 512, 1)["walk"] == 1
    # a single run has nothing to walk
    assert choice(1, 250, 32, 512, 512, 2)["walk"] == 1


def test_auto_prefers_the_rise_walk_for_a_three_twist_grid():
    """3 twists x 250 rises: the twist walk would pay a set-up (about four candidates' worth) per three candidates."""
    c = choice(3, 250, 32, 512, 512)
    assert c["walk"] == 1 and c["cost_twists"] > c["cost_rises"]
    assert choice(3, 250, 32, 512, 512, 2)["walk"] == 2     # forced: it can run
    assert choice(2, 250, 32, 512, 512)["walk"] == 1
