from .HyperparameterGrid import HyperparameterGrid
from .VIPRSGrid import VIPRSGrid
from .VIPRSGridPerChromosome import VIPRSGridPerChromosome
from .VIPRSGridPathwisePerChromosome import VIPRSGridPathwisePerChromosome
from .grid_utils import (bayesian_model_average, bayesian_model_average_per_chromosome, select_best_model,
                         select_best_model_per_chromosome)

__all__ = ["HyperparameterGrid", "VIPRSGrid", "VIPRSGridPerChromosome", "VIPRSGridPathwisePerChromosome",
           "select_best_model", "bayesian_model_average",
           "select_best_model_per_chromosome", "bayesian_model_average_per_chromosome"]
