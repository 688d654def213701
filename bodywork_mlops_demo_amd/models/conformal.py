"""Split-conformal calibration carried by a regressor.

A :class:`Calibration` holds what stage 1 learnt from its hold-out: per
confidence level the half-width ``h`` such that ``prediction ± h`` covers a
fresh exchangeable row with at least that probability
(:func:`ops.residual_quantiles`).  The band has constant width, so serving
an interval costs one add and one subtract per row on top of the
prediction.  A BINNED calibration (``conformal_bins``) also holds one
half-width per level for each of up to 16 equal cells of X (:class:`Cells`,
:func:`ops.binned_residual_quantiles`): the band then follows X, chosen per
row by :meth:`Calibration.halfwidth_at`, and the coverage guarantee holds
within each cell (Mondrian conformal).

Every regressor has an optional ``conformal_`` attribute.  In the joblib
artefact it sits on the sklearn object as a PLAIN DICT (:meth:`as_dict`), so
``joblib.load`` needs nothing but stock sklearn.
"""
from __future__ import annotations

from dataclasses import dataclass, replace

import numpy as np

#: the attribute name on the regressors and on the sklearn artefact
ATTR = "conformal_"


def level_name(level: float) -> str:
    """``0.9 -> "90"``, ``0.975 -> "97.5"``: the ``<pct>`` of the metric
    columns ``pi<pct>_halfwidth`` / ``pi<pct>_coverage`` / ``pi<pct>_ok``."""
    return format(float(level) * 100, "g")


@dataclass(frozen=True)
class Cells:
    """``n`` (1..16) equal cells of ``[lo, hi)``; X outside clamps to an edge
    cell.  The cell rule is the one in ``ops/hip/resid_select_binned.h``."""
    n: int
    lo: float = 0.0
    hi: float = 100.0

    def __post_init__(self):
        object.__setattr__(self, "n", int(self.n))
        object.__setattr__(self, "lo", float(self.lo))
        object.__setattr__(self, "hi", float(self.hi))
        if not 1 <= self.n <= 16:
            raise ValueError(f"Cells: between 1 and 16 cells (got {self.n})")
        if not np.float32(self.hi) > np.float32(self.lo):
            raise ValueError("Cells: fp32(hi) > fp32(lo)")

    def params(self) -> tuple:
        """``(n, lo, scale)`` as fp32 values held as Python floats, ``scale
        = fp32(n) / (fp32(hi) - fp32(lo))``: the one place it is computed."""
        lo = np.float32(self.lo)
        scale = np.float32(self.n) / (np.float32(self.hi) - lo)
        return self.n, float(lo), float(scale)

    def cell_of(self, x) -> np.ndarray:
        """The cell of each ``x`` (int64, -1 for NaN), in numpy float32."""
        from bodywork_mlops_demo_amd.ops import reference

        cell = reference.cells_of_cpu(np.asarray(x, dtype=np.float32),
                                      *self.params())
        return cell.reshape(np.shape(x))


@dataclass(frozen=True)
class Calibration:
    levels: tuple          # confidence levels, each in (0, 1)
    halfwidths: tuple      # fp32 values held as Python floats, one per level
    m: int                 # calibration rows (non-NaN residuals)
    n_nan: int = 0         # hold-out rows left out as NaN
    date: str | None = None  # newest dataset date of the calibrated model
    # binned only; levels / halfwidths / m keep their marginal meaning
    cells: "Cells | None" = None
    cell_halfwidths: tuple | None = None  # [cells][levels]
    cell_m: tuple | None = None           # calibration rows of each cell

    def __post_init__(self):
        lv = tuple(float(v) for v in self.levels)
        hw = tuple(float(np.float32(v)) for v in self.halfwidths)
        if len(lv) != len(hw) or not lv:
            raise ValueError("Calibration: one half-width per level")
        object.__setattr__(self, "levels", lv)
        object.__setattr__(self, "halfwidths", hw)
        object.__setattr__(self, "m", int(self.m))
        object.__setattr__(self, "n_nan", int(self.n_nan))
        if self.date is not None:
            object.__setattr__(self, "date", str(self.date))
        if self.cells is not None:
            chw = tuple(tuple(float(np.float32(v)) for v in row)
                        for row in self.cell_halfwidths)
            cm = tuple(int(v) for v in self.cell_m)
            if (len(chw) != self.cells.n or len(cm) != self.cells.n
                    or any(len(row) != len(lv) for row in chw)):
                raise ValueError(
                    "Calibration: one half-width per cell and level")
            object.__setattr__(self, "cell_halfwidths", chw)
            object.__setattr__(self, "cell_m", cm)

    def _index(self, level: float) -> int:
        level = float(level)
        for q, lv in enumerate(self.levels):
            if abs(lv - level) <= 1e-12:
                return q
        raise ValueError(
            f"no interval calibrated for confidence {level:g}; available "
            f"levels: {', '.join(format(v, 'g') for v in self.levels)}")

    def halfwidth(self, level: float) -> float:
        """The half-width calibrated for ``level``; ValueError naming the
        available levels otherwise."""
        return self.halfwidths[self._index(level)]

    def halfwidth_at(self, level: float, x) -> np.ndarray:
        """The half-width for ``level`` at each ``x`` (float64, the shape of
        ``x``): the cell's own when binned (the marginal one for a NaN
        ``x``, which has no cell), the constant one otherwise."""
        q = self._index(level)
        if self.cells is None:
            return np.full(np.shape(x), self.halfwidths[q])
        col = np.array([row[q] for row in self.cell_halfwidths]
                       + [self.halfwidths[q]])
        return col[self.cells.cell_of(x)]  # -1, no cell: the last entry

    def as_dict(self) -> dict:
        d = {"levels": list(self.levels),
             "halfwidths": list(self.halfwidths),
             "m": self.m, "n_nan": self.n_nan, "date": self.date}
        if self.cells is not None:
            d["cells"] = [self.cells.n, self.cells.lo, self.cells.hi]
            d["cell_halfwidths"] = [list(r) for r in self.cell_halfwidths]
            d["cell_m"] = list(self.cell_m)
        return d

    @classmethod
    def from_dict(cls, d: dict) -> "Calibration":
        binned = {}
        if d.get("cells") is not None:
            binned = {"cells": Cells(*d["cells"]),
                      "cell_halfwidths": d["cell_halfwidths"],
                      "cell_m": d["cell_m"]}
        return cls(tuple(d["levels"]), tuple(d["halfwidths"]), d["m"],
                   d.get("n_nan", 0), d.get("date"), **binned)

    @classmethod
    def from_select(cls, levels, result, date=None) -> "Calibration":
        """From ``ops.residual_quantiles`` output ``(halfwidths, m,
        n_nan)``."""
        hw, m, n_nan = result
        return cls(tuple(levels), tuple(hw.tolist()), m, n_nan, date)

    def with_cells(self, cells: Cells, result) -> "Calibration":
        """This calibration plus ``ops.binned_residual_quantiles`` output
        ``(halfwidths [cells, Q], m [cells], n_nan)`` over ``cells``."""
        hw, m, _ = result
        return replace(self, cells=cells, cell_halfwidths=hw.tolist(),
                       cell_m=m.tolist())


def attach(sk_model, calibration: "Calibration | None"):
    """Store ``calibration`` on an sklearn artefact as a plain dict; an
    uncalibrated model's artefact is left as it is."""
    if calibration is not None:
        setattr(sk_model, ATTR, calibration.as_dict())
    return sk_model


def restore(obj) -> "Calibration | None":
    """The calibration an artefact (or a regressor) carries, or None."""
    c = getattr(obj, ATTR, None)
    if c is None or isinstance(c, Calibration):
        return c
    return Calibration.from_dict(c)
