"""Compute ops: hand-written CDNA4 HIP kernels with CPU torch oracles.

The reference delegates all math to libraries (sklearn ``fit``/``predict``
at ``stage_1:105-106``/``stage_2:78``, numpy RNG at ``stage_3:39-40``);
here every computational primitive is a first-class gfx950 kernel
(SURVEY.md §2.2 mapping table):

- ``datagen``        — on-GPU philox4x32 synthetic-drift generator with
                       in-kernel y>=0 stream compaction (stage_3:28-43)
- ``linreg_stats``   — fused XtX/Xty statistics reduction for the
                       closed-form OLS fit (stage_1:105-106)
- ``poly_fold_stats`` — per-fold power sums: K-fold cross-validation of
                       every polynomial degree and l2 from one pass (no
                       reference counterpart; ``select_poly`` is the host
                       side)
- ``linear_score``   — batched linear scoring (stage_2:78)
- ``regression_metrics`` — single-pass fused MAPE/R^2/max-residual
                       reduction (stage_1:79-90, stage_4:101-113)
- ``drift_histograms`` — fused histograms of features, labels, scores and
                       residuals for the drift monitor (no reference
                       counterpart)
- ``residual_quantiles`` — exact order statistics of |label - score| by a
                       three-pass device radix select, the half-widths of
                       split-conformal prediction intervals; and
                       ``interval_coverage``, the rows inside such bands
                       (no reference counterpart)
- ``gemm_bf16``      — MFMA (v_mfma_f32_16x16x32_bf16) LDS-tiled dense
                       GEMM with fused bias+ReLU epilogue for the MLP path

Dispatch policy: on a CUDA/HIP device the in-tree ``_hipcore`` extension
is REQUIRED — if it is missing the ops raise instead of silently falling
back to eager PyTorch.  On CPU the pure-torch reference implementations
(:mod:`bodywork_mlops_demo_amd.ops.reference`) run; they double as the
numerics oracles in the test suite.
"""
from __future__ import annotations

import glob
import os
from typing import NamedTuple

import numpy as np
import torch

from bodywork_mlops_demo_amd.ops import reference

_HIPCORE = None
_HIPMOD = None  # the same library as a Python module (its bound classes)
_HIPCORE_ERR: str | None = None


def _load_extension():
    global _HIPCORE, _HIPMOD, _HIPCORE_ERR
    if _HIPCORE is not None or _HIPCORE_ERR is not None:
        return _HIPCORE
    here = os.path.dirname(__file__)
    cands = sorted(glob.glob(os.path.join(here, "_hipcore*.so")))
    if not cands:
        _HIPCORE_ERR = (
            "in-tree HIP extension _hipcore*.so not found under "
            f"{here}; build it with `python setup.py build_ext --inplace` "
            "(PYTORCH_ROCM_ARCH=gfx950)"
        )
        return None
    try:
        torch.ops.load_library(cands[0])
        import importlib

        _HIPMOD = importlib.import_module(__name__ + "._hipcore")
        _HIPCORE = torch.ops.bodywork_hip
    except Exception as e:  # loud: a broken build must not silently fall back
        _HIPCORE_ERR = f"failed to load {cands[0]}: {e}"
        raise RuntimeError(_HIPCORE_ERR) from e
    return _HIPCORE


def hip_available() -> bool:
    """True when the _hipcore extension is importable (CPU box included)."""
    try:
        return _load_extension() is not None
    except RuntimeError:
        return False


def _core(device: torch.device):
    """Return the HIP extension for a CUDA tensor op; raise loudly if absent."""
    if device.type != "cuda":
        return None
    ext = _load_extension()
    if ext is None:
        raise RuntimeError(
            "GPU tensor passed but the _hipcore HIP extension is not built: "
            + str(_HIPCORE_ERR)
        )
    return ext


# --------------------------------------------------------------------------
# native artefact writer — ops/hip/artefact_writer.cpp, artefact_stage.cpp
# --------------------------------------------------------------------------

def _hipmod():
    if _load_extension() is None:
        raise RuntimeError(
            "the _hipcore HIP extension is not built: " + str(_HIPCORE_ERR))
    return _HIPMOD


def npy_header(n: int) -> bytes:
    """The header bytes ``np.save`` writes for a 1-D little-endian float32
    array of ``n`` elements, as the native writer builds them."""
    return _hipmod().npy_header(int(n))


def dataset_persister(workers: int, slots: int):
    """A native ``DatasetPersister``: ``submit(y, X, path)`` stages a day's
    1-D float32 CUDA tensors as one complete ``.npy``-pair file image in a
    ring of ``slots`` pinned buffers (D2H on a side stream) and ``workers``
    GIL-free threads write ``<dir>/.tmp-*`` and rename it to ``path``.
    ``submit`` returns a handle with ``done()`` / ``result()``; ``drain()``
    waits for everything and raises the first write error."""
    return _hipmod().DatasetPersister(int(workers), int(slots))


# --------------------------------------------------------------------------
# datagen — reference stage_3:28-43 semantics
# --------------------------------------------------------------------------

def datagen(
    n: int,
    day_of_year: int,
    seed: int,
    f: float = 6.0,
    kappa: float = 1.0,
    A: float = 0.5,
    beta: float = 0.5,
    sigma: float = 10.0,
    device: str | torch.device = "cpu",
    stream_offset: int = 0,
) -> tuple[torch.Tensor, torch.Tensor]:
    """Generate ``y = alpha(d) + beta*X + sigma*eps`` rows with ``y >= 0``.

    ``alpha(d) = kappa + A*sin(2*pi*f*(d-1)/364)`` (reference stage_3:31-33).
    X ~ U(0,100), eps ~ N(0,1) via counter-based philox4x32-10, so the
    stream is reproducible for a (seed, stream_offset) pair on any device
    count — rank r of a DP world passes its row offset as stream_offset.
    Returns (y, X) float32 tensors on ``device`` (length <= n after the
    y>=0 cull, reference stage_3:43).
    """
    device = torch.device(device)
    alpha = reference.alpha(day_of_year, f, kappa, A)
    if device.type == "cuda":
        core = _core(device)
        y, X = core.datagen(n, seed, stream_offset, alpha, beta, sigma)
        return y, X
    return reference.datagen_cpu(n, seed, stream_offset, alpha, beta, sigma)


def alpha(day_of_year: int, f: float = 6.0, kappa: float = 1.0, A: float = 0.5) -> float:
    return reference.alpha(day_of_year, f, kappa, A)


# --------------------------------------------------------------------------
# OLS fit statistics — reference stage_1:105-106 (LinearRegression.fit)
# --------------------------------------------------------------------------

def linreg_stats(X: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
    """Single-pass fused sufficient statistics for 1-feature OLS.

    Returns a float64 tensor ``[n, sum_x, sum_y, sum_xx, sum_xy]`` (on the
    same device).  The closed-form solve is host-side (2x2).  In DP
    training these five scalars are the entire all-reduce payload.
    """
    if X.device.type == "cuda":
        core = _core(X.device)
        return core.linreg_stats(X.contiguous(), y.contiguous())
    return reference.linreg_stats_cpu(X, y)


def linreg_split_stats(
    X: torch.Tensor, y: torch.Tensor, test_frac: float = 0.2, seed: int = 42
) -> torch.Tensor:
    """:func:`linreg_stats` over the TRAIN rows of
    ``random_split(X, y, test_frac, seed)`` without materialising the
    split: the philox flag is evaluated in the reduction kernel.  Element
    0 of the result is the train-row count."""
    if X.device.type == "cuda":
        core = _core(X.device)
        return core.linreg_split_stats(X.contiguous().float(),
                                       y.contiguous().float(),
                                       test_frac, seed)
    X_tr, y_tr, _, _ = reference.random_split_cpu(X, y, test_frac, seed)
    return reference.linreg_stats_cpu(X_tr, y_tr)


def solve_ols(stats: torch.Tensor) -> tuple[float, float]:
    """Closed-form (intercept, coef) from fused stats (2x2 normal equations)."""
    n, sx, sy, sxx, sxy = stats.tolist()
    denom = n * sxx - sx * sx
    if abs(denom) < 1e-30:
        return float(sy / max(n, 1.0)), 0.0
    coef = (n * sxy - sx * sy) / denom
    intercept = (sy - coef * sx) / n
    return intercept, coef


def poly_stats(
    X: torch.Tensor,
    y: torch.Tensor,
    degree: int,
    mu: float = 50.0,
    s: float = 50.0,
) -> torch.Tensor:
    """Fused sufficient statistics for polynomial ridge/OLS.

    The k-feature generalisation of :func:`linreg_stats` (SURVEY §2.2
    mapping table): one pass over (X, y) producing fp64
    ``[n, upper-tri(PhiT Phi), PhiT y]`` over the IMPLICIT normalised
    basis ``phi_j = ((x-mu)/s)^j`` — the design matrix never touches
    HBM.  These scalars are the whole DP all-reduce payload.
    """
    nf = degree + 1
    if X.device.type == "cuda":
        core = _core(X.device)
        return core.poly_stats(X.contiguous().float(),
                               y.contiguous().float(), nf, mu, s)
    return reference.poly_stats_cpu(X, y, nf, mu, s)


def solve_poly(
    stats: torch.Tensor, degree: int, l2: float = 0.0
) -> list[float]:
    """Normalised-basis coefficients from fused stats (host-side solve;
    the intercept term is not penalised)."""
    nf = degree + 1
    tri = nf * (nf + 1) // 2
    vals = stats.cpu().numpy()
    A = np.zeros((nf, nf))
    k = 1
    for a in range(nf):
        for b in range(a, nf):
            A[a, b] = A[b, a] = vals[k]
            k += 1
    bvec = vals[1 + tri:1 + tri + nf]
    if l2 > 0:
        reg = np.eye(nf) * l2 * vals[0]
        reg[0, 0] = 0.0  # do not penalise the intercept
        A = A + reg
    return np.linalg.solve(A, bvec).tolist()


def poly_fold_stats(
    X: torch.Tensor,
    y: torch.Tensor,
    folds: int = 5,
    seed: int = 42,
    mu: float = 50.0,
    s: float = 50.0,
) -> torch.Tensor:
    """Per-fold sufficient statistics for K-fold cross-validation of every
    polynomial degree 1..5 and every ``l2``, in ONE 8 B/row pass.

    Returns fp64 ``[folds, 18]`` on the inputs' device; row f is
    ``[S_0..S_10, T_0..T_5, Q]`` over the rows of fold f with ``S_p = sum
    t^p`` (``S_0`` is the fold's row count), ``T_q = sum y t^q``, ``Q =
    sum y^2`` and ``t = (x-mu)/s`` as in :func:`poly_stats`.  Row i is in
    fold ``(philox(seed, i).x * folds) >> 32`` (a stream of its own).  The
    rows add, so this tensor is the whole DP all-reduce payload;
    :func:`select_poly` turns it into a model.  ``2 <= folds <= 5``.
    """
    if not 2 <= int(folds) <= 5:
        raise ValueError("poly_fold_stats: folds must be in [2, 5]")
    if X.device.type == "cuda":
        core = _core(X.device)
        return core.poly_fold_stats(X.contiguous().float(),
                                    y.contiguous().float(), int(folds),
                                    int(seed), mu, s)
    return reference.poly_fold_stats_cpu(X, y, int(folds), int(seed), mu, s)


class PolySelection(NamedTuple):
    """What :func:`select_poly` returns."""

    degree: int
    l2: float
    coef: list[float]      # normalised basis, solved from all rows
    scores: np.ndarray     # [len(degrees), len(l2_grid)] held-out MSE


def select_poly(fold_stats: torch.Tensor, degrees, l2_grid) -> PolySelection:
    """K-fold model selection over ``degrees`` x ``l2_grid`` from
    :func:`poly_fold_stats` output — host-side, a few batched small solves.

    For the basis ``t^j`` the Gram matrix is the Hankel matrix ``H[a, b] =
    S_{a+b}`` and the squared error of coefficients b on a row set is ``Q
    - 2 bT T + bT H b``.  Per candidate and fold f the training system is
    total minus fold f with :func:`solve_poly`'s ridge convention (penalty
    ``l2 * n_train``, intercept unpenalised); the score is ``sum_f SSE_f /
    sum_f n_f``.  A candidate with a singular training system, or one with
    fewer rows than coefficients, scores ``inf``; if all do, ValueError.
    The smallest score wins; exact ties go to the lower degree, then the
    larger ``l2``.  The chosen candidate is then solved from the total.
    """
    fs = np.asarray(fold_stats.detach().cpu().numpy(), dtype=np.float64)
    max_deg = reference.POLY_FOLD_MAXDEG
    if fs.ndim != 2 or fs.shape[1] != reference.POLY_FOLD_K:
        raise ValueError("select_poly: fold_stats must be [folds, 18]")
    degrees = [int(d) for d in degrees]
    l2s = np.asarray([float(v) for v in l2_grid], dtype=np.float64)
    if (not degrees or l2s.size == 0 or (l2s < 0).any()
            or not all(1 <= d <= max_deg for d in degrees)):
        raise ValueError("select_poly: needs degrees in [1, 5] and l2 >= 0")
    ns = 2 * max_deg + 1
    total = fs.sum(axis=0)
    train = total[None, :] - fs  # [F, 18]
    n_val, n_train = fs[:, 0], train[:, 0]

    def system(rows, nf):
        # Hankel Gram matrices [.., nf, nf], moments [.., nf]
        idx = np.arange(nf)[:, None] + np.arange(nf)[None, :]
        return rows[..., :ns][..., idx], rows[..., ns:ns + nf]

    def ridge(H, n, nf):
        # [L, .., nf, nf]: H + l2 * n * diag(0, 1, .., 1)
        pen = np.eye(nf)
        pen[0, 0] = 0.0
        scale = l2s.reshape((-1,) + (1,) * (H.ndim - 2)) * n
        return H[None] + scale[..., None, None] * pen

    scores = np.full((len(degrees), l2s.size), np.inf)
    for i, d in enumerate(degrees):
        nf = d + 1
        H_tr, T_tr = system(train, nf)
        H_va, T_va = system(fs, nf)
        A = ridge(H_tr, n_train, nf)                       # [L, F, nf, nf]
        rhs = np.broadcast_to(T_tr[None, :, :, None], A.shape[:-1] + (1,))
        ok = np.broadcast_to(n_train >= nf, A.shape[:2]).copy()
        b = np.zeros(A.shape[:-1])
        try:
            b[:] = np.linalg.solve(A, rhs)[..., 0]
        except np.linalg.LinAlgError:
            # some system is singular: find which, one by one
            for li, f in np.ndindex(*A.shape[:2]):
                try:
                    b[li, f] = np.linalg.solve(A[li, f], rhs[li, f, :, 0])
                except np.linalg.LinAlgError:
                    ok[li, f] = False
        sse = (fs[None, :, -1] - 2.0 * np.einsum("lfa,fa->lf", b, T_va)
               + np.einsum("lfa,fab,lfb->lf", b, H_va, b))
        with np.errstate(invalid="ignore"):
            score = sse.sum(axis=1) / n_val.sum()
        score[~ok.all(axis=1) | ~np.isfinite(score)] = np.inf
        scores[i] = score
    if not np.isfinite(scores).any():
        raise ValueError(
            "select_poly: no candidate has a solvable training system in "
            "every fold (too few rows?)")
    best = min(
        ((scores[i, j], degrees[i], -l2s[j], i, j)
         for i in range(len(degrees)) for j in range(l2s.size)))
    _, degree, _, i, j = best
    H, T = system(total, degree + 1)
    coef = np.linalg.solve(ridge(H, total[0], degree + 1)[j], T)
    return PolySelection(degree, float(l2s[j]), coef.tolist(), scores)


def poly_score(
    X: torch.Tensor,
    coef: torch.Tensor | list[float],
    mu: float = 50.0,
    s: float = 50.0,
) -> torch.Tensor:
    """Horner evaluation of the normalised-basis polynomial (fp32).

    ``coef`` may be a device tensor (read in-kernel, so captured serving
    graphs follow redeployed coefficients)."""
    if X.device.type == "cuda":
        core = _core(X.device)
        if not torch.is_tensor(coef):
            coef = torch.tensor(coef, device=X.device, dtype=torch.float32)
        return core.poly_score(X.contiguous().float(), coef.float(), mu, s)
    return reference.poly_score_cpu(X, coef, mu, s)


# --------------------------------------------------------------------------
# scoring — reference stage_2:78 (model.predict)
# --------------------------------------------------------------------------

def linear_score(
    X: torch.Tensor,
    intercept: float | None = None,
    coef: float | None = None,
    ab: torch.Tensor | None = None,
    n_dev: torch.Tensor | None = None,
) -> torch.Tensor:
    """Batched linear scoring ``yhat = intercept + coef * X`` (fp32).

    On GPU, coefficients live in a 2-element device tensor ``ab`` read by
    the kernel, so captured serving graphs track redeployed weights
    without recapture; pass either ``ab`` or the python floats.

    ``n_dev`` (int64[1] tensor on X's device) is a live row count read by
    the kernel: only the first ``n_dev`` rows are scored and the rest of
    the result is unspecified — a captured replay over a padded buffer
    then costs what the live rows cost.
    """
    if X.device.type == "cuda":
        core = _core(X.device)
        if ab is None:
            ab = torch.tensor([intercept, coef], device=X.device,
                              dtype=torch.float32)
        return core.linear_score(X.contiguous(), ab, n_dev)
    if ab is not None:
        intercept, coef = float(ab[0]), float(ab[1])
    return reference.linear_score_cpu(X, intercept, coef)


# --------------------------------------------------------------------------
# metrics — reference stage_1:79-90 and stage_4:101-113
# --------------------------------------------------------------------------

def regression_metric_sums(y: torch.Tensor, yhat: torch.Tensor) -> torch.Tensor:
    """The fused pass behind :func:`regression_metrics`: float64
    ``[n, sum_ape, ss_res, sum_y, sum_yy, max_resid]`` on ``y``'s device."""
    if y.device.type == "cuda":
        core = _core(y.device)
        return core.regression_metrics(y.contiguous(), yhat.contiguous())
    return torch.tensor(reference.metric_sums_cpu(y, yhat),
                        dtype=torch.float64)


def linear_split_metric_sums(
    X: torch.Tensor,
    y: torch.Tensor,
    ab,
    test_frac: float = 0.2,
    seed: int = 42,
) -> torch.Tensor:
    """:func:`regression_metric_sums` of the linear model ``ab =
    [intercept, coef]`` (a float32[2] tensor or a pair of floats) over
    the TEST rows of ``random_split(X, y, test_frac, seed)`` — split,
    predict and metric reduction as one pass; element 0 is the test-row
    count."""
    if X.device.type == "cuda":
        core = _core(X.device)
        if not torch.is_tensor(ab):
            ab = torch.tensor([float(ab[0]), float(ab[1])])
        return core.linear_split_metrics(
            X.contiguous().float(), y.contiguous().float(),
            ab.to(X.device, torch.float32), test_frac, seed)
    _, _, X_te, y_te = reference.random_split_cpu(X, y, test_frac, seed)
    yhat = reference.linear_score_cpu(X_te, float(ab[0]), float(ab[1]))
    return torch.tensor(reference.metric_sums_cpu(y_te, yhat),
                        dtype=torch.float64)


def metrics_from_sums(sums) -> dict:
    """MAPE / R^2 / max residual from ``regression_metric_sums`` output."""
    n, s_ape, ss_res, s_y, s_yy, max_res = (
        sums.tolist() if torch.is_tensor(sums) else sums)
    mape = s_ape / n
    ss_tot = s_yy - s_y * s_y / n
    r2 = 1.0 - ss_res / ss_tot if ss_tot > 0 else 0.0
    return {"MAPE": mape, "r_squared": r2, "max_residual": max_res}


def regression_metrics(y: torch.Tensor, yhat: torch.Tensor) -> dict:
    """Offline model metrics in one fused pass: MAPE, R^2, max residual.

    Matches sklearn's definitions used by the reference
    (``mean_absolute_percentage_error``, ``r2_score``, ``max_error`` —
    stage_1:79-90): MAPE uses |y - yhat| / max(|y|, eps).
    """
    return metrics_from_sums(regression_metric_sums(y, yhat))


def linear_split_metrics(
    X: torch.Tensor,
    y: torch.Tensor,
    ab,
    test_frac: float = 0.2,
    seed: int = 42,
) -> dict:
    """:func:`regression_metrics` of a linear model on the test partition
    of the philox split, without materialising split or predictions."""
    return metrics_from_sums(
        linear_split_metric_sums(X, y, ab, test_frac, seed))


def score_label_metrics(scores: torch.Tensor, labels: torch.Tensor) -> dict:
    """Online (live-service) metrics in one fused pass.

    Matches reference stage_4:101-113: MAPE = mean |score/label - 1|,
    r_squared = Pearson correlation(score, label), max_residual = max APE.
    """
    if scores.device.type == "cuda":
        core = _core(scores.device)
        out = core.score_label_metrics(scores.contiguous(), labels.contiguous())
        n, s_ape, max_ape, s_s, s_l, s_ss, s_ll, s_sl = out.tolist()
    else:
        (n, s_ape, max_ape, s_s, s_l, s_ss, s_ll, s_sl) = (
            reference.score_label_sums_cpu(scores, labels)
        )
    mape = s_ape / n
    cov = s_sl - s_s * s_l / n
    var_s = s_ss - s_s * s_s / n
    var_l = s_ll - s_l * s_l / n
    corr = cov / (var_s * var_l) ** 0.5 if var_s > 0 and var_l > 0 else 0.0
    return {"MAPE": mape, "r_squared": corr, "max_residual": max_ape}


# --------------------------------------------------------------------------
# drift histograms — the monitoring side's one pass over stage 4's tensors
# --------------------------------------------------------------------------

def drift_histograms(
    X: torch.Tensor, labels: torch.Tensor, scores: torch.Tensor, spec
) -> torch.Tensor:
    """Histograms of ``X``, ``labels``, ``scores`` and the residual
    ``labels - scores`` in one fused 12 B/row pass.

    ``spec`` is a :class:`monitoring.drift.HistSpec`; its ``bin_params()``
    is the one place the fp32 ``(lo, scale)`` pairs are computed.  Returns
    int64 ``[4, bins + 3]`` on the inputs' device: rows x / labels /
    scores / residual; slot 0 underflow, ``1..bins`` the bins, ``bins + 1``
    overflow, ``bins + 2`` NaN.  Counts are exact and bitwise
    reproducible; the slot rule is in ``ops/hip/drift_hist.h`` and
    mirrored by the CPU oracle.
    """
    lo, scale = spec.bin_params()
    if X.device.type == "cuda":
        core = _core(X.device)
        return core.drift_histograms(
            X.contiguous().float(), labels.contiguous().float(),
            scores.contiguous().float(), int(spec.bins), lo, scale)
    return reference.drift_histograms_cpu(X, labels, scores, int(spec.bins),
                                          lo, scale)


# --------------------------------------------------------------------------
# conformal intervals — exact residual order statistics and band coverage
# --------------------------------------------------------------------------

#: levels per call (one LDS table per level in the later select passes)
MAX_CONFORMAL_LEVELS = 4
_RESID_SELECT_PASSES = 3   # RS_PASSES in ops/hip/resid_select.h
_RESID_SELECT_STATE = 14   # RS_STATE


def check_levels(levels) -> tuple[float, ...]:
    """``levels`` as a tuple of 1..4 floats, each in (0, 1); ValueError
    otherwise."""
    try:
        lv = tuple(float(v) for v in levels)
    except TypeError:
        lv = (float(levels),)
    if not 1 <= len(lv) <= MAX_CONFORMAL_LEVELS:
        raise ValueError(
            f"conformal levels: between 1 and {MAX_CONFORMAL_LEVELS} levels "
            f"(got {len(lv)})")
    for v in lv:
        if not 0.0 < v < 1.0:
            raise ValueError(f"conformal levels lie in (0, 1) (got {v})")
    return lv


def allreduce_counts(t: torch.Tensor, process_group) -> torch.Tensor:
    """SUM ``t`` over the group (through host memory unless the backend is
    nccl, as the drift monitor does) and hand it back on its device."""
    import torch.distributed as dist

    if t.device.type == "cuda" and dist.get_backend(process_group) != "nccl":
        h = t.cpu()
        dist.all_reduce(h, op=dist.ReduceOp.SUM, group=process_group)
        return h.to(t.device)
    dist.all_reduce(t, op=dist.ReduceOp.SUM, group=process_group)
    return t


def _resid_select(a, b, levels, process_group, ab=None, test_frac=0.0,
                  seed=0):
    """The device select: per pass one histogram sweep, an optional
    all-reduce of the histogram (histograms of row shards add) and the
    one-block pick.  Nothing is read back before the last pick."""
    core = _core(a.device)
    state = torch.zeros(_RESID_SELECT_STATE, dtype=torch.int64,
                        device=a.device)
    hw = None
    for p in range(_RESID_SELECT_PASSES):
        hist = core.resid_select_pass(a, b, state, p, len(levels), ab,
                                      float(test_frac), int(seed))
        if process_group is not None:
            hist = allreduce_counts(hist, process_group)
        hw = core.resid_select_pick(hist, state, p, list(levels))
    m, n_nan = state[:2].tolist()
    return hw, int(m), int(n_nan)


def _select_cpu(r: np.ndarray, levels, process_group):
    if process_group is not None:
        import torch.distributed as dist

        parts = [None] * dist.get_world_size(process_group)
        dist.all_gather_object(parts, r, group=process_group)
        r = np.concatenate(parts)
    return reference.select_residuals_cpu(r, levels)


def residual_quantiles(
    labels: torch.Tensor, scores: torch.Tensor, levels, process_group=None
) -> tuple[torch.Tensor, int, int]:
    """Split-conformal half-widths: exact order statistics of
    ``|labels - scores|``.

    Returns ``(halfwidths, m, n_nan)``: ``halfwidths`` is fp32 ``[Q]`` on
    the inputs' device, ``m`` the number of non-NaN residuals, ``n_nan``
    the number left out as NaN.  Level L gets the k-th smallest residual,
    ``k = ceil((m + 1) * L)``, or +inf when ``k > m`` — so a fresh
    exchangeable row lies within ``prediction ± halfwidth`` with
    probability at least L.  On the GPU this is a three-pass radix select
    (``ops/hip/resid_select.h``): no sort, and one host read at the end.
    With a ``process_group`` every rank passes its row shard, the pass
    histograms are all-reduced and every rank gets the quantiles of the
    union.  Up to four levels, each in (0, 1).
    """
    levels = check_levels(levels)
    if labels.device.type == "cuda":
        return _resid_select(labels.contiguous().float(),
                             scores.contiguous().float(), levels,
                             process_group)
    return _select_cpu(reference.abs_residuals_cpu(labels, scores), levels,
                       process_group)


def linear_split_residual_quantiles(
    X: torch.Tensor,
    y: torch.Tensor,
    ab,
    levels,
    test_frac: float = 0.2,
    seed: int = 42,
    process_group=None,
) -> tuple[torch.Tensor, int, int]:
    """:func:`residual_quantiles` of the linear model ``ab = [intercept,
    coef]`` over the TEST rows of ``random_split(X, y, test_frac, seed)``,
    without materialising split or predictions: the philox flag and the
    score are evaluated inside the select passes."""
    levels = check_levels(levels)
    if X.device.type == "cuda":
        if not torch.is_tensor(ab):
            ab = torch.tensor([float(ab[0]), float(ab[1])])
        return _resid_select(
            y.contiguous().float(), X.contiguous().float(), levels,
            process_group, ab=ab.to(X.device, torch.float32).contiguous(),
            test_frac=test_frac, seed=seed)
    _, _, X_te, y_te = reference.random_split_cpu(X, y, test_frac, seed)
    yhat = reference.linear_score_cpu(X_te, float(ab[0]), float(ab[1]))
    return _select_cpu(reference.abs_residuals_cpu(y_te, yhat), levels,
                       process_group)


def interval_coverage(
    scores: torch.Tensor, labels: torch.Tensor, halfwidths
) -> torch.Tensor:
    """How many rows lie inside each constant band: float64 ``[n, c_0 ..
    c_3]`` on the inputs' device, ``c_q`` the count of rows with ``|label -
    score| <= halfwidths[q]`` — exact integers, one fused 8 B/row pass.
    ``halfwidths`` holds up to four fp32 values (a tensor or floats);
    missing ones are padded with -1 and count nothing, as does a NaN
    residual."""
    h = torch.as_tensor(halfwidths, dtype=torch.float32).reshape(-1)
    if h.numel() > MAX_CONFORMAL_LEVELS:
        raise ValueError(
            f"interval_coverage: at most {MAX_CONFORMAL_LEVELS} half-widths")
    pad = h.new_full((MAX_CONFORMAL_LEVELS - h.numel(),), -1.0)
    h = torch.cat([h, pad])
    if scores.device.type == "cuda":
        core = _core(scores.device)
        return core.interval_coverage(scores.contiguous().float(),
                                      labels.contiguous().float(),
                                      h.to(scores.device))
    return reference.interval_coverage_cpu(scores, labels, h)


# --------------------------------------------------------------------------
# train/test split — reference stage_1:98-103 (train_test_split, seed 42)
# --------------------------------------------------------------------------

def random_split(
    X: torch.Tensor,
    y: torch.Tensor,
    test_frac: float = 0.2,
    seed: int = 42,
) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """Seeded random split into (X_train, y_train, X_test, y_test).

    Row i is a test row iff ``philox(seed, i).x < test_frac * 2^32``
    (E[test share] = test_frac exactly; count is binomial), both
    partitions stable-ordered — a single fused GPU pass instead of the
    reference's host-side permutation (``train_test_split`` at
    stage_1:98-103, which cost 2/3 of the GPU train phase).  Same philox
    stream on CPU, so splits are device-independent.
    """
    if X.device.type == "cuda":
        core = _core(X.device)
        return core.random_split(X.contiguous().float(),
                                 y.contiguous().float(), test_frac, seed)
    return reference.random_split_cpu(X, y, test_frac, seed)


def train_test_split_indices(
    n: int, test_size: float = 0.2, seed: int = 42, device: str | torch.device = "cpu"
) -> tuple[torch.Tensor, torch.Tensor]:
    """Random permutation split: ``(train_idx, test_idx)`` from a seeded
    ``torch.randperm`` drawn on the CPU, the first ``round(n * test_size)``
    indices being the test rows; the index tensors are then moved to
    ``device``.  Unrelated to the philox split of :func:`random_split`."""
    device = torch.device(device)
    g = torch.Generator(device="cpu").manual_seed(seed)
    perm = torch.randperm(n, generator=g)
    n_test = int(round(n * test_size))
    test_idx, train_idx = perm[:n_test], perm[n_test:]
    if device.type == "cuda":
        return train_idx.to(device), test_idx.to(device)
    return train_idx, test_idx


# --------------------------------------------------------------------------
# MFMA GEMM — MLP path
# --------------------------------------------------------------------------

def linear_bf16(
    x: torch.Tensor,
    w: torch.Tensor,
    bias: torch.Tensor | None = None,
    relu: bool = False,
    mask: torch.Tensor | None = None,
    out_fp32: bool = False,
) -> torch.Tensor:
    """C[M,N] = x[M,K] @ w[N,K]^T with a fused epilogue — bf16 MFMA GEMM.

    torch.nn.functional.linear convention: both operands K-contiguous in
    memory, so LDS staging is coalesced and fragment reads are single
    ds_read_b128s (ops/hip/gemm.hip).  Epilogue (fused into the C-write):
    ``+bias`` then ``relu``, or ``* (mask > 0)`` (ReLU backward).
    CPU oracle: fp32 torch matmul.
    """
    if x.device.type == "cuda":
        core = _core(x.device)
        return core.linear_bf16(
            x.contiguous(), w.contiguous(),
            bias.contiguous() if bias is not None else None,
            relu,
            mask.contiguous() if mask is not None else None,
            out_fp32,
        )
    return reference.linear_bf16_cpu(x, w, bias, relu, mask, out_fp32)


def linear_relu_mask_bf16(
    x: torch.Tensor, w: torch.Tensor, bias: torch.Tensor | None = None
) -> tuple[torch.Tensor, torch.Tensor]:
    """relu(x @ w^T + bias) AND its 1-bit activation mask in one pass
    (the MLP forward hot path; the mask feeds the masked backward GEMM)."""
    if x.device.type == "cuda":
        core = _core(x.device)
        return core.linear_relu_mask_bf16(
            x.contiguous(), w.contiguous(),
            bias.contiguous() if bias is not None else None)
    return reference.linear_relu_mask_cpu(x, w, bias)


def gemm_tn_bf16(
    a: torch.Tensor, b: torch.Tensor, out_fp32: bool = False
) -> torch.Tensor:
    """C[M,N] = a[R,M]^T @ b[R,N] — the dW = dY^T @ X backward shape.

    When R is a tile multiple, this routes through two bandwidth-bound
    LDS-tiled transposes + the glds NT kernel (the transposes cost ~3% of
    the GEMM; the direct transpose-staged TN kernel runs at ~1/7th the NT
    rate).  Odd R falls back to the TN kernel.
    """
    if a.device.type == "cuda":
        core = _core(a.device)
        a = a.contiguous()
        b = b.contiguous()
        if a.shape[0] % 64 == 0 and a.shape[0] >= 256:
            at_ = core.transpose_bf16(a)  # [M,R]
            bt_ = core.transpose_bf16(b)  # [N,R]
            return core.linear_bf16(at_, bt_, None, False, None, out_fp32)
        return core.gemm_tn_bf16(a, b, out_fp32)
    return reference.gemm_tn_bf16_cpu(a, b, out_fp32)


def e4m3_exponent(amax: float) -> int:
    """Per-tensor shared exponent for e4m3: smallest e with amax/2^e <= 448
    (no saturation), clamped to the E8M0 range."""
    import math

    if not math.isfinite(amax) or amax <= 0.0:
        return 0
    e = math.ceil(math.log2(amax / 448.0))
    while amax / (2.0 ** e) > 448.0:  # guard float fuzz at the boundary
        e += 1
    return max(-127, min(127, e))


def quantize_e4m3(x: torch.Tensor, e: int) -> torch.Tensor:
    """x -> OCP e4m3 byte codes with value = 2^e * stored (RNE, saturating).

    GPU path: packed v_cvt_pk_fp8_f32 (ops/hip/gemm_mx8.hip); CPU oracle:
    nearest-value-on-grid (ops/reference.py).
    """
    if x.device.type == "cuda":
        core = _core(x.device)
        return core.quantize_e4m3(x.contiguous(), int(e))
    return reference.quantize_e4m3_cpu(x, int(e))


def expand1d_e4m3(
    x: torch.Tensor,
    w: torch.Tensor,
    b: torch.Tensor | None,
    e: int,
    n_dev: torch.Tensor | None = None,
) -> torch.Tensor:
    """h = relu(x*w + b) emitted DIRECTLY as e4m3 bytes (value = 2^e *
    stored) — the MLP fp8 scoring forward's fused layer 1.  Unfused the
    path costs 5 HBM bytes per element (bf16 write + re-read + fp8
    write); fused it costs 1.  CPU oracle: quantize_e4m3_cpu of the
    bf16-rounded activation.

    ``n_dev`` (int64[1] tensor on x's device) is a live row count read by
    the kernel: only the first ``n_dev`` rows (clamped to [0, n]) are
    written, the rest of the result is unspecified.  The CPU oracle
    computes every row."""
    if x.device.type == "cuda":
        core = _core(x.device)
        return core.expand1d_e4m3(
            x.contiguous(), w.contiguous(),
            b.contiguous() if b is not None else None, int(e), n_dev)
    h = reference.expand1d_cpu(x, w, b, relu=True).float()
    return reference.quantize_e4m3_cpu(h, int(e))


def gemm_mx8_nt(
    a8: torch.Tensor,
    ea: int,
    b8: torch.Tensor,
    eb: int,
    bias: torch.Tensor | None = None,
    relu: bool = False,
    out_fp32: bool = False,
) -> torch.Tensor:
    """C[M,N] = 2^(ea+eb) * (a8[M,K] . b8[N,K]^T) over e4m3 operands —
    the 2x-rate MX path.

    Uses the gfx950 block-scaled K=128 MFMA
    (__builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4) with the
    per-tensor shared exponents passed as uniform E8M0 scale operands, so
    dequantisation is exact (power-of-two) and free (HW-fused).  The
    non-scaled fp8 MFMAs run at the BF16 rate on CDNA4 — this instruction
    is the only 2x fp8 path.  Requires M%256==0, N%256==0, K%128==0.
    Fused bias+relu epilogue available (the MLP serving forward).
    CPU oracle: decode + fp32 matmul.
    """
    if a8.device.type == "cuda":
        core = _core(a8.device)
        return core.gemm_mx8_nt(
            a8.contiguous(), int(ea), b8.contiguous(), int(eb),
            bias.contiguous() if bias is not None else None, relu, out_fp32)
    return reference.gemm_mx8_nt_cpu(a8, ea, b8, eb, bias, relu, out_fp32)


def gemm_mx8_relu_dot(
    a8: torch.Tensor,
    ea: int,
    b8: torch.Tensor,
    eb: int,
    b2: torch.Tensor,
    w3: torch.Tensor,
    n_dev: torch.Tensor | None = None,
) -> torch.Tensor:
    """y[M] = Σ_col relu(2^(ea+eb)·(a8·b8ᵀ) + b2) * w3 — the MLP scoring
    forward's hot GEMM and the rowdot head fused into ONE kernel.

    The [M,N] activation tensor is never written to HBM (saves its bf16
    write + the rowdot re-read ≈ 16 GB per 1M rows at N=4096): each
    wave butterfly-reduces its 64-column strip in registers and fl==0
    lanes accumulate per-row partials with fp32 atomics.  Caller adds
    the scalar output bias.  CPU oracle: decode + matmul + relu + dot.

    ``n_dev`` (int64[1] tensor on a8's device) is a live row count read
    by the kernel and clamped to [0, M]: row tiles past it return before
    staging anything, rows ``>= n_dev`` of y are exactly 0 and whatever
    their a8 rows hold (NaN bytes included) reaches no live row — a
    captured replay over a padded bucket costs what the live tiles cost.
    """
    if a8.device.type == "cuda":
        core = _core(a8.device)
        return core.gemm_mx8_relu_dot(a8.contiguous(), int(ea),
                                      b8.contiguous(), int(eb),
                                      b2.contiguous(), w3.contiguous(),
                                      n_dev)
    h2 = reference.gemm_mx8_nt_cpu(a8, ea, b8, eb, bias=b2, relu=True,
                                   out_fp32=True)
    return _zero_dead_rows(h2 @ w3.float(), n_dev)


def _zero_dead_rows(y: torch.Tensor, n_dev: torch.Tensor | None):
    """CPU oracle of the fused heads' live row count: rows at or past
    ``n_dev`` (clamped to [0, M]) are 0."""
    if n_dev is None:
        return y
    n = min(max(int(n_dev.reshape(-1)[0]), 0), y.shape[0])
    y = y.clone()
    y[n:] = 0.0
    return y


def gemm_mx8_relu_mask(
    a8: torch.Tensor,
    ea: int,
    b8: torch.Tensor,
    eb: int,
    bias: torch.Tensor | None = None,
) -> tuple[torch.Tensor, torch.Tensor]:
    """relu(2^(ea+eb)·(a8·b8ᵀ) + bias) as bf16 AND its 1-bit activation
    mask (uint8 [M, N/8]) in one pass — the MX-fp8 twin of
    :func:`linear_relu_mask_bf16` for the opt-in fp8 training forward.

    The mask tests the fp32 epilogue value (strict ``> 0``); the bf16
    output is bit-identical to ``gemm_mx8_nt(..., relu=True)``.  ``bias``
    is fp32 [N].  Requires M%256==0, N%256==0, K%128==0 on GPU.
    CPU oracle: decode + fp32 matmul + pack_relu_mask.
    """
    if a8.device.type == "cuda":
        core = _core(a8.device)
        return core.gemm_mx8_relu_mask(
            a8.contiguous(), int(ea), b8.contiguous(), int(eb),
            bias.contiguous().float() if bias is not None else None)
    c = reference.gemm_mx8_nt_cpu(a8, ea, b8, eb, bias, relu=True,
                                  out_fp32=True)
    return c.to(torch.bfloat16), reference.pack_relu_mask(c > 0)


def expand1d_bf16_e4m3(
    x: torch.Tensor,
    w: torch.Tensor,
    b: torch.Tensor | None,
    e: int,
) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """h = relu(x*w + b) emitted in ONE pass as (bf16 activation, 1-bit
    mask, e4m3 bytes with value = 2^e * stored) — the fp8 training
    forward's layer 1: the backward needs the bf16 copy and the mask, the
    MX GEMM needs the e4m3 copy.  Each output is bit-identical to the
    single-output op (``expand1d_bf16(relu=True, emit_mask=True)`` /
    ``expand1d_e4m3``).  CPU oracle: composition of those two ops."""
    if x.device.type == "cuda":
        core = _core(x.device)
        return core.expand1d_bf16_e4m3(
            x.contiguous().float(), w.contiguous(),
            b.contiguous() if b is not None else None, int(e))
    h, mask = reference.expand1d_cpu(x, w, b, relu=True, emit_mask=True)
    return h, mask, expand1d_e4m3(x, w, b, e)


# --------------------------------------------------------------------------
# MX-fp8 training backward: e5m2 gradients, device exponents, mask-mul
# --------------------------------------------------------------------------

_MX_FMT = {"e4m3": 0, "e5m2": 1}


def e5m2_exponent(amax: float) -> int:
    """Per-tensor shared exponent for e5m2: smallest e with amax/2^e <=
    57344 (no saturation), clamped to [-127, 127]; 0 for a zero or
    non-finite amax.  Exact at the boundary (float field arithmetic)."""
    return reference.e5m2_exponent(amax)


def _split_exp(e, device: torch.device) -> tuple[int, torch.Tensor | None]:
    """An exponent argument (Python int | int32[1] tensor) as the op's
    (host int, optional device tensor) pair."""
    if torch.is_tensor(e):
        if e.dtype != torch.int32 or e.numel() != 1:
            raise TypeError("a tensor exponent must be int32 with 1 element")
        return 0, e.reshape(1).to(device)
    return int(e), None


def amax_exponent_e5m2(x: torch.Tensor, w: torch.Tensor) -> torch.Tensor:
    """int32[1] e5m2 exponent of the bound ``max|x| * max|w|`` (fp32) on
    every element of ``outer(x, w)`` — the per-step gradient scale of the
    fp8 backward, computed ON THE DEVICE (one launch, no atomics, bitwise
    deterministic, capturable) so a captured step never syncs.  Same rule
    as :func:`e5m2_exponent`.  ``x`` fp32 [n], ``w`` bf16 [H]."""
    if x.device.type == "cuda":
        core = _core(x.device)
        return core.amax_exponent_e5m2(x.contiguous().float(),
                                       w.contiguous())
    return reference.amax_exponent_e5m2_cpu(x, w)


def quantize_e5m2(x: torch.Tensor, e) -> torch.Tensor:
    """x -> OCP e5m2 byte codes with value = 2^e * stored (RNE, saturating
    at +-57344 by an explicit clamp).  ``e`` is a Python int or an
    int32[1] device tensor (read in-kernel).  CPU oracle: nearest value
    on the finite grid, ties to the even code."""
    if x.device.type == "cuda":
        core = _core(x.device)
        eh, ed = _split_exp(e, x.device)
        return core.quantize_e5m2(x.contiguous(), eh, ed)
    return reference.quantize_e5m2_cpu(x, e)


def expand1d_bf16_e5m2(
    x: torch.Tensor,
    w: torch.Tensor,
    mask: torch.Tensor,
    e_dev: torch.Tensor,
) -> tuple[torch.Tensor, torch.Tensor]:
    """dz = outer(x, w) * bit(mask) emitted in ONE pass as (bf16 [n,H],
    e5m2 bytes [n,H] with value = 2^e * stored) — the fp8 backward's
    ``dz2``.  The bf16 output is bit-identical to
    ``expand1d_bf16(x, w, None, relu=False, mask=mask)``; the bytes
    quantise that bf16-rounded value; ``e_dev`` (int32[1]) is read
    in-kernel.  CPU oracle: composition of those two ops."""
    if x.device.type == "cuda":
        core = _core(x.device)
        return core.expand1d_bf16_e5m2(
            x.contiguous().float(), w.contiguous(), mask.contiguous(),
            _split_exp(e_dev, x.device)[1])
    out = reference.expand1d_cpu(x, w, None, False, mask)
    return out, reference.quantize_e5m2_cpu(out.float(), e_dev)


def transpose_u8(src: torch.Tensor) -> torch.Tensor:
    """[C,R] uint8 = [R,C] uint8 transposed (LDS-tiled, 16-B global I/O)
    — makes the fp8 wgrad operands K-contiguous over the batch.  R and C
    must be multiples of 16."""
    if src.dim() != 2 or src.shape[0] % 16 or src.shape[1] % 16:
        raise RuntimeError(
            "transpose_u8 requires a 2-d tensor with rows%16==0 and "
            f"cols%16==0 (got {tuple(src.shape)})")
    if src.device.type == "cuda":
        core = _core(src.device)
        return core.transpose_u8(src.contiguous())
    return src.t().contiguous()


def gemm_mx8_nt_fmt(
    a8: torch.Tensor,
    ea,
    b8: torch.Tensor,
    eb,
    a_fmt: str = "e4m3",
    b_fmt: str = "e4m3",
    mask: torch.Tensor | None = None,
    out_fp32: bool = False,
) -> torch.Tensor:
    """C[M,N] = 2^(ea+eb) * (a8[M,K] . b8[N,K]^T) [* bit(mask)] with each
    operand e4m3 or e5m2 — :func:`gemm_mx8_nt` generalised for the
    training backward.

    ``ea`` / ``eb`` are each a Python int or an int32[1] device tensor;
    a tensor is read by the kernel at run time (clamped to the E8M0
    range there), so a captured graph follows a per-step gradient scale.
    ``mask`` is the 1-bit ReLU mask (uint8 [M, N/8]) of the dgrad
    epilogue.  With the defaults the result is bit-identical to
    ``gemm_mx8_nt``.  Requires M%256==0, N%256==0, K%128==0 on GPU.
    CPU oracle: decode + fp32 matmul + mask."""
    if a_fmt not in _MX_FMT or b_fmt not in _MX_FMT:
        raise ValueError(f"fp8 format must be one of {sorted(_MX_FMT)}")
    if a8.device.type == "cuda":
        core = _core(a8.device)
        eah, ead = _split_exp(ea, a8.device)
        ebh, ebd = _split_exp(eb, a8.device)
        return core.gemm_mx8_nt_fmt(
            a8.contiguous(), eah, ead, b8.contiguous(), ebh, ebd,
            _MX_FMT[a_fmt], _MX_FMT[b_fmt],
            mask.contiguous() if mask is not None else None, out_fp32)
    return reference.gemm_mx8_nt_fmt_cpu(a8, ea, b8, eb, a_fmt, b_fmt, mask,
                                         out_fp32)


def linear_relu_dot_bf16(
    x: torch.Tensor,
    w: torch.Tensor,
    b2: torch.Tensor,
    w3: torch.Tensor,
    n_dev: torch.Tensor | None = None,
) -> torch.Tensor:
    """y[M] = Σ_col relu(x[M,K] @ w[N,K]ᵀ + b2) * w3 — the bf16 MLP
    scoring forward's hot GEMM and rowdot head fused into one kernel
    (the bf16 twin of gemm_mx8_relu_dot: the [M,N] activation never
    reaches HBM).  Requires M%256==0, N%256==0, K%128==0.
    ``n_dev``: live row count, same contract as gemm_mx8_relu_dot's.
    CPU oracle: fp32 matmul + relu + dot."""
    if x.device.type == "cuda":
        core = _core(x.device)
        return core.gemm8_relu_dot_bf16(x.contiguous(), w.contiguous(),
                                        b2.contiguous(), w3.contiguous(),
                                        n_dev)
    h2 = torch.relu(x.float() @ w.float().t() + b2.float())
    return _zero_dead_rows(h2 @ w3.float(), n_dev)


def transpose_bf16(src: torch.Tensor) -> torch.Tensor:
    """[C,R] bf16 = [R,C] bf16 transposed (64x64 LDS tiles, 16-B I/O)."""
    if src.device.type == "cuda":
        core = _core(src.device)
        return core.transpose_bf16(src.contiguous())
    return src.t().contiguous()


def expand1d_bf16(
    x: torch.Tensor,
    w: torch.Tensor,
    b: torch.Tensor | None = None,
    relu: bool = False,
    mask: torch.Tensor | None = None,
    emit_mask: bool = False,
    n_dev: torch.Tensor | None = None,
):
    """Fused rank-1 expansion: out[i,j] = act(x[i]*w[j] + b[j]).

    The MLP's 1-feature input layer (and its backward dh = outer(dy, w))
    as a single bandwidth-bound kernel instead of a degenerate K=1 MFMA
    GEMM.  ``mask`` is a 1-BIT relu mask (uint8 [n, H/8], bit e of byte c
    = column 8c+e active) — 16x less backward mask traffic than re-reading
    activations; ``emit_mask`` additionally returns that bitmask for the
    produced activations.  Returns bf16 (n, H) (or a (out, maskbits)
    pair when ``emit_mask``).

    ``n_dev`` (int64[1] tensor on x's device; plain ``relu=True`` scoring
    use only, no ``mask``/``emit_mask``) is a live row count read by the
    kernel: only the first ``n_dev`` rows (clamped to [0, n]) are written,
    the rest of the result is unspecified.  The CPU oracle computes every
    row.
    """
    if n_dev is not None and (mask is not None or emit_mask or not relu):
        raise ValueError(
            "expand1d_bf16: n_dev serves the plain relu scoring use only "
            "(relu=True, no mask, no emit_mask)")
    if x.device.type == "cuda":
        core = _core(x.device)
        out, mbits = core.expand1d_bf16(
            x.contiguous().float(), w.contiguous(),
            b.contiguous() if b is not None else None,
            relu,
            mask.contiguous() if mask is not None else None,
            emit_mask,
            n_dev,
        )
        return (out, mbits) if emit_mask else out
    return reference.expand1d_cpu(x, w, b, relu, mask, emit_mask)


def rowdot_bf16(
    h: torch.Tensor, w: torch.Tensor, b: torch.Tensor | float = 0.0
) -> torch.Tensor:
    """out[i] = sum_j h[i,j] * w[j] + b — the MLP output head (GEMV).

    One wave per row, vectorised bf16x8 loads, shuffle reduction;
    fp32 output (scoring precision — BASELINE "bf16 fit + fp32 scoring").
    ``b`` may be a 1-element device tensor (read on-device, so the whole
    forward is hipGraph-capturable) or a python float.
    """
    if h.device.type == "cuda":
        core = _core(h.device)
        if not torch.is_tensor(b):
            b = torch.full((1,), float(b), device=h.device,
                           dtype=torch.float32)
        return core.rowdot_bf16(h.contiguous(), w.contiguous(),
                                b.reshape(1).float())
    return reference.rowdot_cpu(h, w, float(b) if not torch.is_tensor(b)
                                else float(b.reshape(-1)[0]))


def coldot_bf16(
    m: torch.Tensor, v: torch.Tensor, also_colsum: bool = False
):
    """dw[j] = sum_i m[i,j] * v[i] (fp32), optionally fused with
    cs[j] = sum_i m[i,j] in the same pass (bias gradients)."""
    if m.device.type == "cuda":
        core = _core(m.device)
        out = core.coldot_bf16(m.contiguous(), v.contiguous().float(), also_colsum)
        return (out[0], out[1]) if also_colsum else out[0]
    return reference.coldot_cpu(m, v, also_colsum)


def colsum_bf16(m: torch.Tensor) -> torch.Tensor:
    """cs[j] = sum_i m[i,j] (fp32)."""
    if m.device.type == "cuda":
        core = _core(m.device)
        return core.colsum_bf16(m.contiguous())
    return reference.colsum_cpu(m)


def adam_step(
    p: torch.Tensor,
    g: torch.Tensor,
    m: torch.Tensor,
    v: torch.Tensor,
    p_bf16: torch.Tensor | None,
    lr: float,
    t: int,
    beta1: float = 0.9,
    beta2: float = 0.999,
    eps: float = 1e-8,
    bc: torch.Tensor | None = None,
) -> None:
    """Fused in-place Adam update, optionally writing the bf16 shadow
    weight in the same pass (one HBM traversal per parameter per step).
    ``bc`` (device tensor [1/(1-b1^t), 1/(1-b2^t)]) overrides the host
    bias correction so a captured training-step graph stays valid across
    steps."""
    if p.device.type == "cuda":
        core = _core(p.device)
        core.adam_step(p.view(-1), g.reshape(-1).float(), m.view(-1),
                       v.view(-1),
                       p_bf16.view(-1) if p_bf16 is not None else None,
                       lr, beta1, beta2, eps, t, bc)
        return
    reference.adam_step_cpu(p, g, m, v, p_bf16, lr, t, beta1, beta2, eps)


def batch_indices(
    ctr: torch.Tensor, n_dev: torch.Tensor, bs: int, seed: int
) -> torch.Tensor:
    """Device-side philox minibatch sampling; ``ctr`` (int64 [1], device)
    advances on-device and the data size ``n_dev`` (int64 [1], device) is
    read in-kernel, so a captured step stays valid across days whose row
    counts differ."""
    core = _core(ctr.device)
    return core.batch_indices(ctr, n_dev, bs, seed)


def transpose_to_bf16(src: torch.Tensor) -> torch.Tensor:
    """dst[C,R] bf16 = src[R,C] fp32 transposed (LDS-tiled on GPU)."""
    if src.device.type == "cuda":
        core = _core(src.device)
        return core.transpose_to_bf16(src.contiguous())
    return src.t().contiguous().bfloat16()
