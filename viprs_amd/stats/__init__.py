"""Statistics of the inputs computed on the device (the reference gets them from magenpy)."""
from .spectrum import (UnpinnedLambdaMinError, annotate_spectrum, lambda_min_from_extremes,  # noqa: F401
                       ld_spectrum)
