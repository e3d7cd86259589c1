"""Evaluation of fitted effects: from summary statistics (pseudo-validation) and against measured phenotypes (the
reference's ``viprs.eval``)."""
from .pseudo_metrics import pseudo_pearson_r, pseudo_r2, _streamlined_pseudo_r2  # noqa: F401
from .continuous_metrics import pearson_r, r2  # noqa: F401
