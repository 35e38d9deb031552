"""The float64 optimality checker of tests/model_optimality.py on the CPU, before it judges the device: tight scikit-learn
fits of the four models on fixture G14's system (the oracle's nearest-neighbour matrices: integer hit counts, exact) meet
its KKT conditions to ~1e-9 or better, and fits of a slightly wrong problem — alpha x 1.01, rho swapped, no centring, no
symmetry rows, a float32 fit — violate them far above the bound the GPU tests hold the device to (KKT_BOUND = 1e-5)."""
import numpy as np
import pytest

from oracle import path_a as A
from tests.model_optimality import REFITS, System, model_params, sklearn_fit

KW = dict(reconstruct_diameter_2d_pixel=20, reconstruct_diameter_3d_pixel=20, reconstruct_length_2d_pixel=32,
          reconstruct_length_3d_pixel=6, sym_oversample=1)
MODELS = {"elasticnet": (1e-4, 0.5), "lasso": (1e-4, 1.0), "ridge": (1.0, 0.0), "lreg": (0.0, 0.0)}
GPU_BOUND = 1e-5     # tests/test_gpu_path_a_model_optimality.py: KKT_BOUND
FIT_BOUND = 1e-7     # what a tight float64 fit must reach (measured 6e-15 ... 3.5e-13; Ridge's L-BFGS-B 7e-9)


@pytest.fixture(scope="module")
def parts(golden_dir):
    img = np.load(golden_dir / "g14_sklearn_models.npz")["image"]
    _, _, p = A.lsq_reconstruct(img, 1.0, 29.0, 2.0, 1, interpolation="nn", return_parts=True, **KW)
    return p


@pytest.fixture(scope="module")
def system(parts):
    return System.from_parts(parts)


@pytest.fixture(scope="module")
def dense(system):
    return system.dense()


def test_the_system_is_the_oracles(parts, system):
    assert np.array_equal(parts["A_data"].data, np.round(parts["A_data"].data))     # hit counts: exact in float32
    assert system.m == parts["A_data"].shape[0] + parts["A_hsym"].shape[0] and system.n == int(parts["mask"].sum())
    assert abs(system.bc.sum()) < 1e-9 * np.abs(system.bc).sum()
    # the gradient is the objective's: a central difference along a random direction
    rng = np.random.default_rng(0)
    w, d = rng.standard_normal(system.n) * 1e-2, rng.standard_normal(system.n)
    a, rho, h = 1e-3, 0.0, 1e-4
    fd = (system.objective(w + h * d, a, rho) - system.objective(w - h * d, a, rho)) / (2 * h)
    assert abs(fd - system.gradient(w, a, rho) @ d) < 1e-8 * abs(fd)


@pytest.mark.parametrize("positive", [0, 1])
@pytest.mark.parametrize("model", list(MODELS))
def test_tight_fits_meet_the_conditions_and_wrong_problems_do_not(system, dense, parts, model, positive):
    pytest.importorskip("sklearn")
    X, y = dense
    alpha, rho0 = MODELS[model]
    a, rho = model_params(model, alpha, rho0, system.m)
    w = sklearn_fit(X, y, model, a, rho, positive)
    assert system.violation(w, a, rho, positive) < FIT_BOUND, model
    assert system.violation(w.astype(np.float32), a, rho, positive) < 1e-7     # the float32 map of it: 1.5e-8 ... 2.4e-8
    if a > 0:
        assert min(system.violation(w, a * 1.01, rho, positive), system.violation(w, a * 0.99, rho, positive)) > 10 * GPU_BOUND
    assert system.violation(w, a, rho, positive, centred=False) > 10 * GPU_BOUND        # centring dropped
    assert System.from_parts(parts, drop_sym=True).violation(w, a, rho, positive) > 10 * GPU_BOUND   # symmetry rows dropped
    if model in ("lasso", "ridge"):    # rho swapped: lasso checked as ridge and back (elasticnet below, at rho != 1/2)
        assert system.violation(w, a, 1 - rho, positive) > 10 * GPU_BOUND


def test_swapped_rho_and_a_float32_fit_are_caught(system, dense):
    pytest.importorskip("sklearn")
    import warnings

    from sklearn.exceptions import ConvergenceWarning
    from sklearn.linear_model import ElasticNet

    X, y = dense
    w = sklearn_fit(X, y, "elasticnet", 1e-4, 0.3, False)
    assert system.violation(w, 1e-4, 0.3, False) < FIT_BOUND
    assert system.violation(w, 1e-4, 0.7, False) > 10 * GPU_BOUND
    # the reference's kind of fit: scikit-learn on the float32 matrix, at its tolerance
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", ConvergenceWarning)
        w32 = ElasticNet(alpha=1e-4, l1_ratio=0.5, tol=1e-4, selection="cyclic").fit(X.astype(np.float32), y.astype(np.float32)).coef_
    assert w32.dtype == np.float32
    assert system.violation(w32, 1e-4, 0.5, False) > GPU_BOUND


def test_alpha_zero_and_the_refit_count(system, dense):
    """Above alpha_zero w = 0 is optimal and below it is not; refits() counts lsq_reconstruct_batch's alpha / 10 loop."""
    pytest.importorskip("sklearn")
    X, y = dense
    for positive in (0, 1):
        az = system.alpha_zero(0.5, positive)
        zero = np.zeros(system.n)
        assert system.violation(zero, az * 1.001, 0.5, positive) == 0
        assert system.violation(zero, az * 0.99, 0.5, positive) > 1e-3
        assert not sklearn_fit(X, y, "elasticnet", az * 1.001, 0.5, positive).any()
        assert sklearn_fit(X, y, "elasticnet", az * 0.9, 0.5, positive).any()
        assert system.refits(az * 0.5, 0.5, positive)[0] == 0
        k, al = system.refits(az * 250, 0.5, positive)
        assert k == 3 and al < az <= al * 10
        assert system.refits(az * 1e20, 0.5, positive)[0] == REFITS
        assert system.refits(0.0, 0.0, positive) == (0, 0.0)
    assert system.alpha_zero(0.0, 0) == np.inf                          # ridge: never, while the centred b is not 0
    zero_b = System(np.zeros(system.m_data), matvec=system.matvec, rmatvec=lambda v: system._rmv(v), n=system.n)
    assert zero_b.alpha_zero(0.0, 0) == 0 and zero_b.violation(np.zeros(system.n), 0.0, 0.0, False) == 0
