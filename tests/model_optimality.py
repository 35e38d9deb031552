"""Float64 optimality conditions of the scikit-learn models' common objective (solver_linear_regression.py:270-342), as
``hh_pab_solve_prox`` (csrc/path_a_batch.inc) states it:

    (1 / 2m) |(b - mean b) - (A - 1 mu^T) w|^2 + a rho |w|_1 + a (1 - rho) / 2 |w|^2,      w >= 0 where positive

with A = [A_data; A_hsym] (data rows, then symmetry rows; m counts both), b = [b_data; 0] and mu = A^T 1 / m.  Whatever
algorithm produced w, it is the minimiser exactly when every coordinate meets the KKT conditions, so these checks judge a
solution without trusting the solver that made it.  Not a product path and not the oracle: a test helper, like
``kernel_model.py``.
"""
import numpy as np

REFITS = 12   # the alpha / 10 refits of an all-zero solution (helicon_amd/solver.py, lsq_reconstruct_batch)


def model_params(model, alpha, l1_ratio, m):
    """(a, rho) of the objective for a model of ``lsq_reconstruct`` (helicon_amd.solver._model_of): ridge divides its alpha
    by m and has rho = 0; lreg has a = 0."""
    if model in ("elasticnet",):
        return float(alpha), float(l1_ratio)
    if model == "lasso":
        return float(alpha), 1.0
    if model == "ridge":
        return float(alpha) / m, 0.0
    if model == "lreg":
        return 0.0, 0.0
    raise ValueError(model)


class System:
    """The centred least-squares system of one candidate.  ``A`` is a SciPy sparse matrix (data rows, then symmetry rows)
    or ``None`` with ``matvec`` / ``rmatvec`` callables of that matrix; ``b_data`` the data rows' right-hand side."""

    def __init__(self, b_data, A=None, matvec=None, rmatvec=None, n=None):
        self.b_data = np.asarray(b_data, dtype=np.float64)
        if A is not None:
            A = A.tocsr().astype(np.float64)
            self.m, self.n = A.shape
            self._mv, self._rmv = (lambda x: A @ x), (lambda y: A.T @ y)
        else:
            self._mv, self._rmv = matvec, rmatvec
            self.m = len(matvec(np.zeros(int(n))))
            self.n = int(n)
        self.m_data = len(self.b_data)
        b = np.concatenate((self.b_data, np.zeros(self.m - self.m_data)))
        self.bc = b - b.mean()
        self.mu = self._rmv(np.ones(self.m)) / self.m
        self.c0 = self.centred_rmatvec(self.bc) / self.m      # (1 / m) (A - 1 mu^T)^T bc: -gradient of the fit at w = 0

    @classmethod
    def from_parts(cls, parts, drop_sym=False):
        """From ``oracle.path_a.lsq_reconstruct(..., return_parts=True)``'s matrices."""
        from scipy.sparse import vstack

        Ad, Ah = parts["A_data"], parts["A_hsym"]
        A = Ad if Ah is None or drop_sym else vstack((Ad, Ah))
        return cls(parts["b_data"], A=A)

    def matvec(self, x):
        return self._mv(np.asarray(x, dtype=np.float64))

    def centred_matvec(self, x):
        x = np.asarray(x, dtype=np.float64)
        return self._mv(x) - self.mu @ x

    def centred_rmatvec(self, y):
        y = np.asarray(y, dtype=np.float64)
        return self._rmv(y) - self.mu * y.sum()

    def gradient(self, w, a, rho):
        """-(1/m) (A - 1 mu^T)^T (bc - (A - 1 mu^T) w) + a (1 - rho) w: the gradient of the smooth part."""
        w = np.asarray(w, dtype=np.float64)
        r = self.bc - self.centred_matvec(w)
        return -self.centred_rmatvec(r) / self.m + a * (1 - rho) * w

    def objective(self, w, a, rho):
        w = np.asarray(w, dtype=np.float64)
        r = self.bc - self.centred_matvec(w)
        return r @ r / (2 * self.m) + a * rho * np.abs(w).sum() + 0.5 * a * (1 - rho) * (w @ w)

    def lambda_max(self, positive):
        """max_j |(1/m) (A - 1 mu^T)^T bc|_j (its positive part with positivity): the scale the violation is measured in."""
        return float(np.maximum(self.c0, 0).max() if positive else np.abs(self.c0).max())

    def kkt(self, w, a, rho, positive, centred=True):
        """Per-coordinate KKT violation of w (``centred=False``: the conditions of the uncentred problem, a negative control)."""
        w = np.asarray(w, dtype=np.float64)
        if centred:
            g = self.gradient(w, a, rho)
        else:
            b = np.concatenate((self.b_data, np.zeros(self.m - self.m_data)))
            g = -self._rmv(b - self._mv(w)) / self.m + a * (1 - rho) * w
        t = a * rho
        v = np.where(w > 0, np.abs(g + t), np.where(w < 0, np.abs(g - t), 0.0))
        zero = w == 0
        v[zero] = np.maximum(0.0, -g[zero] - t) if positive else np.maximum(0.0, np.abs(g[zero]) - t)
        if positive:
            v[w < 0] = np.inf
        return v

    def violation(self, w, a, rho, positive, centred=True):
        """The largest KKT violation, normalised by ``lambda_max`` (the absolute value when lambda_max is 0)."""
        lam = self.lambda_max(positive)
        v = float(self.kkt(w, a, rho, positive, centred).max())
        return v / lam if lam > 0 else v

    def alpha_zero(self, rho, positive):
        """The smallest alpha at which w = 0 is optimal (inf when none is: rho = 0 and a non-zero fit at 0)."""
        lam = self.lambda_max(positive)
        if lam == 0:
            return 0.0
        return lam / rho if rho > 0 else np.inf

    def refits(self, alpha, rho, positive):
        """How many alpha / 10 refits lsq_reconstruct_batch makes before w = 0 stops being optimal (its loop: the same
        multiplications by 0.1, at most ``REFITS``; none for alpha = 0)."""
        if alpha == 0:
            return 0, alpha
        az = self.alpha_zero(rho, positive)
        k, al = 0, float(alpha)
        while al >= az and k < REFITS:
            al = al * 0.1
            k += 1
        return k, al

    def score(self, w, clip=False):
        """cosine(A_data w, b_data) of the reference's scorer (lib/analysis.py:802-821), clipped at 0 with thresh_fraction >= 0."""
        pred = self.matvec(w)[: self.m_data]
        if clip:
            pred = np.clip(pred, 0, None)
        norm = np.linalg.norm(pred) * np.linalg.norm(self.b_data)
        return 0.0 if norm == 0 else float(pred @ self.b_data / norm)

    def dense(self):
        """A as a dense array and b = [b_data; 0]: scikit-learn's input (it centres both itself) on the small boxes."""
        eye = np.eye(self.n)
        A = np.stack([self.matvec(eye[:, j]) for j in range(self.n)], axis=1)
        return A, np.concatenate((self.b_data, np.zeros(self.m - self.m_data)))


def sklearn_fit(X, y, model, a, rho, positive, tol=1e-12, max_iter=200000):
    """A tight float64 scikit-learn fit of the objective at (a, rho) on dense X (fit_intercept=True, cyclic selection):
    ElasticNet / Lasso by coordinate descent; ridge without positivity by its normal equations; lreg by LinearRegression;
    ridge and lreg under positivity by Ridge's L-BFGS-B (alpha = a m; coordinate descent and NNLS take minutes there)."""
    import warnings

    from sklearn.exceptions import ConvergenceWarning
    from sklearn.linear_model import ElasticNet, Lasso, LinearRegression, Ridge

    m, n = X.shape
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", ConvergenceWarning)
        warnings.simplefilter("ignore", UserWarning)
        if model in ("ridge", "lreg") and positive:
            est = Ridge(alpha=a * m, fit_intercept=True, positive=True, solver="lbfgs", tol=1e-14, max_iter=max_iter)
            return est.fit(X, y).coef_.astype(np.float64)
        if model == "lreg":
            return LinearRegression(fit_intercept=True, positive=bool(positive)).fit(X, y).coef_.astype(np.float64)
        if model == "ridge" and not positive:
            Xc, yc = X - X.mean(axis=0), y - y.mean()
            return np.linalg.solve(Xc.T @ Xc / m + a * np.eye(n), Xc.T @ yc / m)
        if model == "lasso":
            est = Lasso(alpha=a, fit_intercept=True, positive=bool(positive), tol=tol, max_iter=max_iter, selection="cyclic")
        else:
            est = ElasticNet(alpha=a, l1_ratio=rho, fit_intercept=True, positive=bool(positive), tol=tol, max_iter=max_iter,
                             selection="cyclic")
        return est.fit(X, y).coef_.astype(np.float64)
