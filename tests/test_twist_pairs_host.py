"""Pair layout of the ky-major run table (`hh_pair_table_slot`, host arithmetic only): the twist walk at N = 512 reads its
tables two runs to an entry, [pair][ky][rows][2] complex words, runs counted from the first of their table group.

The expected offsets are written out here from that definition; the library's function is the one its table kernel, its
fused pass and its allocation use.
"""
import ctypes as C

import numpy as np
import pytest

from helicon_amd import _lib


def slot(runs, run, nky, rows, ky, row):
    out = (C.c_int64 * 3)()
    rc = _lib.lib().hh_pair_table_slot(runs, run, nky, rows, ky, row, out)
    assert rc == 0
    return int(out[0]), int(out[1]), int(out[2])


@pytest.mark.parametrize("runs, nky, rows", [(1, 256, 68), (2, 256, 68), (5, 256, 532), (8, 4, 4), (400, 256, 132)])
def test_every_word_of_a_group_is_owned_once(runs, nky, rows):
    """(run, ky, row) -> ((run // 2 * nky + ky) * rows + row) * 2 + run % 2: the two runs of a pair interleave word by word,
    a wavefront's (pair, ky) row is rows * 16 contiguous bytes, and a group of an odd number of runs occupies one run more,
    whose words belong to nobody but the last run's zero partner."""
    rng = np.random.default_rng(runs)
    kys = sorted(set([0, nky - 1] + list(rng.integers(0, nky, 3))))
    rws = sorted(set([0, 1, rows - 1] + list(rng.integers(0, rows, 3))))
    words = (runs + 1) // 2 * 2 * nky * rows
    seen = set()
    for run in range(runs):
        for ky in kys:
            for row in rws:
                off, total, partner = slot(runs, run, nky, rows, int(ky), int(row))
                assert off == ((run // 2 * nky + int(ky)) * rows + int(row)) * 2 + run % 2
                assert total == words and 0 <= off < total
                assert partner == (off + 1 if runs % 2 == 1 and run == runs - 1 else -1)
                assert off not in seen
                seen.add(off)
                if partner >= 0:
                    assert partner < total and partner not in seen
    # a pair row is contiguous: (pair, ky, row 0, first run) ... (pair, ky, rows - 1, second run)
    if runs >= 2:
        a0 = slot(runs, 0, nky, rows, kys[-1], 0)[0]
        b_last = slot(runs, 1, nky, rows, kys[-1], rows - 1)[0]
        assert b_last - a0 == 2 * rows - 1 and a0 % 2 == 0


def test_allocation_grows_by_at_most_one_run():
    for runs in range(1, 12):
        total = slot(runs, 0, 256, 68, 0, 0)[1]
        assert runs * 256 * 68 <= total <= (runs + 1) * 256 * 68
        assert total == (runs + runs % 2) * 256 * 68


def test_group_bases_are_even_runs():
    """Runs are counted from their table group's first, so every group starts a pair whatever its place in the sweep: run 0
    of a group is word 0 of the group's buffer, and a launch that begins at run r of the group finds its first run in pair
    r // 2, half r % 2."""
    assert slot(7, 0, 256, 68, 0, 0)[0] == 0
    for r in range(7):
        off = slot(7, r, 256, 68, 0, 0)[0]
        assert off // (2 * 256 * 68) == r // 2 and off % 2 == r % 2


def test_bad_arguments():
    L = _lib.lib()
    out = (C.c_int64 * 3)()
    for args in [(0, 0, 256, 68, 0, 0), (3, 3, 256, 68, 0, 0), (3, -1, 256, 68, 0, 0), (3, 0, 0, 68, 0, 0),
                 (3, 0, 256, 0, 0, 0), (3, 0, 256, 68, 256, 0), (3, 0, 256, 68, 0, 68), (3, 0, 256, 68, -1, 0)]:
        assert L.hh_pair_table_slot(*args, out) == -1
    assert L.hh_pair_table_slot(3, 0, 256, 68, 0, 0, None) == -1
