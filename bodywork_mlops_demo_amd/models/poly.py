"""Polynomial ridge regressor on MI355X — the third model family.

The k-feature generalisation of the closed-form OLS path (SURVEY.md §2.2
mapping table: "fused XᵀX + Xᵀy reduction ... generalizes"): the fit is
one fused HIP pass (`ops.poly_stats`) that expands the normalised
polynomial basis ``phi_j = ((x-50)/50)^j`` on the fly — the design
matrix never exists in memory — followed by a host-side
ridge-regularised normal-equation solve; scoring is a Horner kernel
whose coefficients live in a device buffer (captured serving graphs
follow redeploys, like the linear model).

Drift rationale: the generator's concept drift moves the intercept
sinusoidally; between retrains a curved fit tracks residual structure a
line cannot, and the ridge term keeps the high-order terms tame on
1440-row days.

Artefact: a stock sklearn ``Pipeline(PolynomialFeatures, Ridge)`` whose
RAW-x coefficients are computed from the normalised fit by exact fp64
change of basis — ``joblib.load`` + ``predict`` work with stock sklearn.
"""
from __future__ import annotations

import numpy as np
import torch

from bodywork_mlops_demo_amd.utils.device import canonical_device

from bodywork_mlops_demo_amd import ops
from bodywork_mlops_demo_amd.models import conformal


class GPUPolyRegressor:
    X_MU = 50.0
    X_SIGMA = 50.0  # scale to t in [-1, 1] for U(0,100) inputs
    #: optional split-conformal calibration (models/conformal.py)
    conformal_: "conformal.Calibration | None" = None

    def __init__(self, degree: int = 3, l2: float = 1e-6, device="cpu"):
        if not 1 <= degree <= 5:
            raise ValueError("degree must be in [1, 5]")
        self.degree = degree
        self.l2 = float(l2)
        self.device = canonical_device(device)
        self.coef_t_: list[float] = [0.0] * (degree + 1)  # normalised basis
        self._coef_dev: torch.Tensor | None = None

    # -- training ----------------------------------------------------------
    def fit(self, X: torch.Tensor, y: torch.Tensor, process_group=None):
        stats = ops.poly_stats(X, y, self.degree, self.X_MU, self.X_SIGMA)
        if process_group is not None:
            import torch.distributed as dist

            dist.all_reduce(stats, group=process_group)
        self.coef_t_ = ops.solve_poly(stats, self.degree, self.l2)
        self._sync_dev()
        return self

    # -- inference ----------------------------------------------------------
    def _coef_tensor(self) -> torch.Tensor:
        if self._coef_dev is None or self._coef_dev.device != self.device:
            self._coef_dev = torch.tensor(self.coef_t_, device=self.device,
                                          dtype=torch.float32)
        return self._coef_dev

    def _sync_dev(self) -> None:
        if self._coef_dev is not None:
            self._coef_dev.copy_(torch.tensor(self.coef_t_,
                                              dtype=torch.float32))

    def predict(self, X: torch.Tensor) -> torch.Tensor:
        if X.device.type == "cuda":
            return ops.poly_score(X, self._coef_tensor(), self.X_MU,
                                  self.X_SIGMA)
        return ops.poly_score(X, self.coef_t_, self.X_MU, self.X_SIGMA)

    def to(self, device):
        self.device = canonical_device(device)
        self._coef_dev = None
        return self

    def copy_weights_from(self, other: "GPUPolyRegressor") -> bool:
        """In-place coefficient swap (serving hot-redeploy)."""
        if (not isinstance(other, GPUPolyRegressor)
                or other.degree != self.degree):
            return False
        self.coef_t_ = list(other.coef_t_)
        self.l2 = other.l2
        self.conformal_ = other.conformal_
        self._sync_dev()
        return True

    # -- basis change (exact, fp64) -----------------------------------------
    def _raw_coefs(self) -> np.ndarray:
        """q(x) = p((x - mu)/s) expanded in powers of x."""
        from numpy.polynomial import polynomial as P

        p = np.asarray(self.coef_t_, dtype=np.float64)
        sub = np.array([-self.X_MU / self.X_SIGMA, 1.0 / self.X_SIGMA])
        q = np.array([p[-1]])
        for c in p[-2::-1]:  # Horner in polynomial arithmetic
            q = P.polyadd(P.polymul(q, sub), [c])
        return np.pad(q, (0, self.degree + 1 - len(q)))

    @classmethod
    def _from_raw_coefs(cls, raw: np.ndarray, degree: int, l2: float,
                        device) -> "GPUPolyRegressor":
        from numpy.polynomial import polynomial as P

        sub = np.array([cls.X_MU, cls.X_SIGMA])  # x = mu + s*t
        p = np.array([raw[-1]])
        for c in raw[-2::-1]:
            p = P.polyadd(P.polymul(p, sub), [c])
        self = cls(degree=degree, l2=l2, device=device)
        self.coef_t_ = np.pad(p, (0, degree + 1 - len(p))).tolist()
        return self

    # -- artefact compatibility ---------------------------------------------
    def to_sklearn(self):
        from sklearn.linear_model import Ridge
        from sklearn.pipeline import Pipeline
        from sklearn.preprocessing import PolynomialFeatures

        raw = self._raw_coefs()
        poly = PolynomialFeatures(degree=self.degree, include_bias=False)
        poly.fit(np.zeros((1, 1)))
        ridge = Ridge(alpha=self.l2)
        ridge.coef_ = raw[1:].copy()
        ridge.intercept_ = float(raw[0])
        ridge.n_features_in_ = self.degree
        return conformal.attach(Pipeline([("poly", poly), ("ridge", ridge)]),
                                self.conformal_)

    @classmethod
    def from_sklearn(cls, pipe, device="cpu") -> "GPUPolyRegressor":
        ridge = pipe.named_steps["ridge"]
        degree = pipe.named_steps["poly"].degree
        raw = np.concatenate([[float(ridge.intercept_)],
                              np.asarray(ridge.coef_, dtype=np.float64)])
        return cls._from_raw_coefs(raw, degree, float(ridge.alpha), device)

    def __repr__(self) -> str:
        return (f"Pipeline(PolynomialFeatures(degree={self.degree}), "
                f"Ridge(alpha={self.l2}))")


class GPUPolyRegressorCV(GPUPolyRegressor):
    """:class:`GPUPolyRegressor` that picks ``degree`` and ``l2`` itself by
    K-fold cross-validation — the ``RidgeCV`` / ``GridSearchCV`` of this
    family, at the cost of ONE statistics pass.

    ``ops.poly_fold_stats`` reduces (X, y) to 18 sums per fold; from those
    ``ops.select_poly`` scores every (degree <= ``max_degree``, l2 in
    ``l2_grid``) candidate on every held-out fold and solves the winner
    from all rows.  After ``fit`` the object IS a fitted
    ``GPUPolyRegressor`` of the chosen degree: scoring, the sklearn
    artefact and hot-redeploy are inherited (a redeploy onto a scorer of
    another degree is refused by ``copy_weights_from``, so the caller
    builds a fresh scorer).

    ``best_params_`` is ``{"degree", "l2"}``, ``best_score_`` the winner's
    held-out MSE and ``cv_results_`` the whole grid as parallel lists
    ``degree`` / ``l2`` / ``mean_test_mse`` (``inf``: not solvable).
    """

    def __init__(self, max_degree: int = 5,
                 l2_grid=(0.0, 1e-6, 1e-4, 1e-2, 1.0), folds: int = 5,
                 seed: int = 42, device="cpu"):
        if not 1 <= max_degree <= 5:
            raise ValueError("max_degree must be in [1, 5]")
        if not 2 <= folds <= 5:
            raise ValueError("folds must be in [2, 5]")
        l2_grid = tuple(float(v) for v in l2_grid)
        if not l2_grid or min(l2_grid) < 0:
            raise ValueError("l2_grid needs at least one value, all >= 0")
        super().__init__(degree=max_degree, l2=l2_grid[0], device=device)
        self.max_degree = max_degree
        self.l2_grid = l2_grid
        self.folds = folds
        self.seed = seed
        self.best_params_: dict | None = None
        self.best_score_: float | None = None
        self.cv_results_: dict | None = None

    def fit(self, X: torch.Tensor, y: torch.Tensor, process_group=None):
        stats = ops.poly_fold_stats(X, y, self.folds, self.seed, self.X_MU,
                                    self.X_SIGMA)
        if process_group is not None:
            import torch.distributed as dist

            dist.all_reduce(stats, group=process_group)
        return self._select(stats)

    def _select(self, fold_stats: torch.Tensor):
        degrees = list(range(1, self.max_degree + 1))
        sel = ops.select_poly(fold_stats, degrees, self.l2_grid)
        if sel.degree != self.degree:
            self._coef_dev = None  # another length: rebuilt on next use
        self.degree, self.l2, self.coef_t_ = sel.degree, sel.l2, sel.coef
        self._sync_dev()
        self.best_params_ = {"degree": sel.degree, "l2": sel.l2}
        self.best_score_ = float(
            sel.scores[degrees.index(sel.degree),
                       self.l2_grid.index(sel.l2)])
        self.cv_results_ = {
            "degree": [d for d in degrees for _ in self.l2_grid],
            "l2": [v for _ in degrees for v in self.l2_grid],
            "mean_test_mse": sel.scores.reshape(-1).tolist(),
        }
        return self
