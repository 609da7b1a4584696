from . import base                                             # noqa: F401
from .base import BaseDistribution, DiagGaussian, ClassCondDiagGaussian, GlowBase, GaussianMixture, StudentT, GeneralizedGaussian, MultivariateGaussian, MultivariateStudentT    # noqa: F401
