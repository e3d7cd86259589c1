"""Metrics of a polygenic score against a measured continuous phenotype (the reference's ``viprs.eval.continuous_metrics``)."""
import numpy as np

__all__ = ["pearson_r", "r2"]


def pearson_r(true_val, pred_val):
    """Pearson correlation of the two (n,) vectors in float64 (NaN when either is constant)."""
    y = np.asarray(true_val, dtype=np.float64).ravel()
    p = np.asarray(pred_val, dtype=np.float64).ravel()
    if y.shape != p.shape:
        raise ValueError(f"{y.shape[0]} phenotypes against {p.shape[0]} predictions")
    yc, pc = y - y.mean(), p - p.mean()
    den = np.sqrt(np.dot(yc, yc) * np.dot(pc, pc))
    return float(np.dot(yc, pc) / den) if den > 0 else float("nan")


def r2(true_val, pred_val):
    """The squared Pearson correlation in float64 -- the ``rvalue ** 2`` of ``scipy.stats.linregress(pred, true)`` that the
    reference's ``r2`` returns (viprs/eval/continuous_metrics.py)."""
    return pearson_r(true_val, pred_val) ** 2
