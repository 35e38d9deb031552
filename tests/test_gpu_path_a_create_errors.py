"""hh_pab_create_ex's failures that Python can reach: the exception type, the exact message of hh_pab_last_error(NULL),
and that the failed create leaves nothing behind — an ordinary batch built straight afterwards solves and equals the
one built before any failure, bit for bit."""
import ctypes as C

import numpy as np
import pytest

from helicon_amd.solver import PAB_FORCE_BANDED, PathABatch, hh_pa_params

pytestmark = pytest.mark.gpu

D2, L2, L3 = 12, 32, 4


def _image():
    rng = np.random.default_rng(20260412)
    return np.ascontiguousarray(rng.standard_normal((16, 32)), dtype=np.float32)


def _param(twist=29.0, rise=2.0, csym=1, tilt=0.0, psi=0.0, d3=D2, interpolation=0, mode=0, half=0, ids=None):
    q = hh_pa_params(1.0, twist, rise, csym, tilt, psi, 0.0, D2, L2, d3, 0, L3, 100, 100, interpolation, mode, half)
    if ids is not None:
        q.n_fsc_ids = len(ids)
        q.fsc_ids = (C.c_int32 * max(1, len(ids)))(*ids)
    return q


def _good(interpolation):
    return [_param(29.0, 2.0, 1, interpolation=interpolation), _param(-31.0, 2.5, 2, interpolation=interpolation),
            _param(58.0, 3.0, 1, interpolation=interpolation)]


def _solve(interpolation):
    with PathABatch(_image(), _good(interpolation)) as B:
        x, scores, info = B.solve(1, 0)
        dims = (B.n, B.device_bytes, B.m_data.copy(), B.m_sym.copy(), B.n_ops.copy(), B.product_form)
        return dims, x, scores, info


@pytest.fixture(scope="module")
def fresh():
    """The ordinary batches, built before any create has failed in this module."""
    return {ip: _solve(ip) for ip in (0, 1)}


NO_VOXEL = "hh_pab_create: the cylinder holds no voxel"
NEEDS_FLAT = ("hh_pab_create: not sliceable — the batched trilinear projector needs tilt = psi = 0 "
              "(the single-candidate hh_pa has the general form)")
NO_RAY = "hh_pab_create: no projection ray of a candidate meets the cylinder"
UNKNOWN_FLAGS = "hh_pab_create_ex: unknown flags"

CASES = {
    # a 3-D diameter of 2 pixels: the cylinder's radius (diameter // 2 - 1) is zero
    "no_voxel_nn": (lambda: [_param(d3=2)], 0, NO_VOXEL),
    "no_voxel_linear": (lambda: [_param(d3=2, interpolation=1)], 0, NO_VOXEL),
    "no_voxel_second_of_batch": (lambda: [_param(d3=2), _param(31.0, d3=2)], 0, NO_VOXEL),
    "linear_needs_flat_tilt": (lambda: [_param(tilt=3.0, interpolation=1)], 0, NEEDS_FLAT),
    "linear_needs_flat_psi": (lambda: [_param(interpolation=1), _param(31.0, psi=-2.0, interpolation=1)], 0, NEEDS_FLAT),
    "linear_needs_flat_banded": (lambda: [_param(tilt=3.0, interpolation=1)], PAB_FORCE_BANDED, NEEDS_FLAT),
    # a half set that keeps no row (mode 1 with an empty id list, first half): fails after the rows were enumerated
    "empty_half_set_nn": (lambda: [_param(), _param(31.0, mode=1, half=1, ids=[])], 0, NO_RAY),
    "empty_half_set_linear": (lambda: [_param(interpolation=1, mode=1, half=1, ids=[])], 0, NO_RAY),
    "unknown_flags": (lambda: _good(0), 4, UNKNOWN_FLAGS),
    "unknown_flags_high_bit": (lambda: _good(1), PAB_FORCE_BANDED | 64, UNKNOWN_FLAGS),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_failed_create_reports_and_leaves_nothing_behind(case, fresh):
    make, flags, message = CASES[case]
    params = make()
    with pytest.raises(ValueError) as ei:
        PathABatch(_image(), params, flags=flags)
    assert type(ei.value) is ValueError
    assert str(ei.value) == f"hh_pab_create error -1: {message}"
    for ip in (0, 1):
        dims, x, scores, info = _solve(ip)
        want_dims, want_x, want_scores, want_info = fresh[ip]
        assert dims[0] == want_dims[0] and dims[1] == want_dims[1] and dims[5] == want_dims[5]
        for a, b in zip(dims[2:5], want_dims[2:5]):
            np.testing.assert_array_equal(a, b)
        np.testing.assert_array_equal(x, want_x)
        np.testing.assert_array_equal(scores, want_scores)
        np.testing.assert_array_equal(info, want_info)
    assert np.isfinite(fresh[0][2]).all() and np.isfinite(fresh[1][2]).all()
