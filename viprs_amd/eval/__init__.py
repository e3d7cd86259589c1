"""Evaluation of fitted effects from summary statistics (the reference's ``viprs.eval``)."""
from .pseudo_metrics import pseudo_pearson_r, pseudo_r2, _streamlined_pseudo_r2  # noqa: F401
