"""Split-conformal calibration carried by a regressor.

A :class:`Calibration` holds what stage 1 learnt from its hold-out: per
confidence level the half-width ``h`` such that ``prediction ± h`` covers a
fresh exchangeable row with at least that probability
(:func:`ops.residual_quantiles`).  The band has constant width, so serving
an interval costs one add and one subtract per row on top of the
prediction.

Every regressor has an optional ``conformal_`` attribute.  In the joblib
artefact it sits on the sklearn object as a PLAIN DICT (:meth:`as_dict`), so
``joblib.load`` needs nothing but stock sklearn.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

#: the attribute name on the regressors and on the sklearn artefact
ATTR = "conformal_"


def level_name(level: float) -> str:
    """``0.9 -> "90"``, ``0.975 -> "97.5"``: the ``<pct>`` of the metric
    columns ``pi<pct>_halfwidth`` / ``pi<pct>_coverage`` / ``pi<pct>_ok``."""
    return format(float(level) * 100, "g")


@dataclass(frozen=True)
class Calibration:
    levels: tuple          # confidence levels, each in (0, 1)
    halfwidths: tuple      # fp32 values held as Python floats, one per level
    m: int                 # calibration rows (non-NaN residuals)
    n_nan: int = 0         # hold-out rows left out as NaN
    date: str | None = None  # newest dataset date of the calibrated model

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

    def halfwidth(self, level: float) -> float:
        """The half-width calibrated for ``level``; ValueError naming the
        available levels otherwise."""
        level = float(level)
        for lv, hw in zip(self.levels, self.halfwidths):
            if abs(lv - level) <= 1e-12:
                return hw
        raise ValueError(
            f"no interval calibrated for confidence {level:g}; available "
            f"levels: {', '.join(format(v, 'g') for v in self.levels)}")

    def as_dict(self) -> dict:
        return {"levels": list(self.levels),
                "halfwidths": list(self.halfwidths),
                "m": self.m, "n_nan": self.n_nan, "date": self.date}

    @classmethod
    def from_dict(cls, d: dict) -> "Calibration":
        return cls(tuple(d["levels"]), tuple(d["halfwidths"]), d["m"],
                   d.get("n_nan", 0), d.get("date"))

    @classmethod
    def from_select(cls, levels, result, date=None) -> "Calibration":
        """From ``ops.residual_quantiles`` output ``(halfwidths, m,
        n_nan)``."""
        hw, m, n_nan = result
        return cls(tuple(levels), tuple(hw.tolist()), m, n_nan, date)


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
