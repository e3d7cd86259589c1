"""Statistics of the inputs computed on the device (the reference gets them from magenpy)."""
from .spectrum import (UnpinnedLambdaMinError, annotate_spectrum, lambda_min_from_extremes,  # noqa: F401
                       ld_spectrum)
from .ldsc import annotate_ld_scores, ld_scores, ld_scores_host, simple_ldsc  # noqa: F401
from .clump import clump_host, clump_order  # noqa: F401  (`stats.clump` stays the module: its `clump` is `stats.clump.clump`)
from .enet import enet_objective, enet_sums_host, enet_sweep_host, lambda_path  # noqa: F401
from .gibbs import gibbs_draws_host, gibbs_sweep_host, philox4x32_10  # noqa: F401  (`stats.gibbs.gibbs_route` stays in the module)
from .cs import cs_sums_host, cs_update_host, cs_variates_host, gig_half_from_variates  # noqa: F401
from .susie import credible_sets, pips, susie_elbo, susie_host  # noqa: F401
