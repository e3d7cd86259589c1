from .VIPRS import VIPRS
from .VIPRSMix import VIPRSMix
from .LDPredInf import LDPredInf
from .ClumpThreshold import ClumpThreshold
from .Lassosum import Lassosum
from .LDpred2 import LDpred2
from .PRSCS import PRSCS
from .PRSCSx import PRSCSx
from .SBayesR import SBayesR
from .SuSiE import SuSiE
from .VIPRSPerChromosome import VIPRSPerChromosome
from .VIPRSMixPerChromosome import VIPRSMixPerChromosome
from .gridsearch import (HyperparameterGrid, VIPRSGrid, VIPRSGridPathwisePerChromosome, VIPRSGridPerChromosome,
                         bayesian_model_average, bayesian_model_average_per_chromosome, select_best_model,
                         select_best_model_per_chromosome)

__all__ = ["VIPRS", "VIPRSMix", "LDPredInf", "ClumpThreshold", "Lassosum", "LDpred2", "PRSCS", "PRSCSx", "SBayesR", "SuSiE", "VIPRSPerChromosome", "VIPRSMixPerChromosome", "VIPRSGrid", "VIPRSGridPerChromosome",
           "VIPRSGridPathwisePerChromosome",
           "HyperparameterGrid", "select_best_model", "bayesian_model_average", "select_best_model_per_chromosome",
           "bayesian_model_average_per_chromosome"]
