from . import base                                             # noqa: F401
from . import target                                           # noqa: F401
from . import prior                                            # noqa: F401
from . import mh_proposal                                      # noqa: F401
from . import linear_interpolation                             # noqa: F401
from . import encoder                                          # noqa: F401
from . import decoder                                          # noqa: F401
from .base import BaseDistribution, DiagGaussian, ClassCondDiagGaussian, GlowBase, GaussianMixture, StudentT, GeneralizedGaussian, MultivariateGaussian, MultivariateStudentT, UniformGaussian    # noqa: F401
from .target import Target, TwoMoons, CircularGaussianMixture, RingMixture    # noqa: F401
from .prior import PriorDistribution, TwoModes, Sinusoidal, Sinusoidal_gap, Sinusoidal_split, Smiley    # noqa: F401
from .mh_proposal import MHProposal, DiagGaussianProposal    # noqa: F401
from .linear_interpolation import LinearInterpolation    # noqa: F401
from .encoder import BaseEncoder, Dirac, Uniform, ConstDiagGaussian, NNDiagGaussian    # noqa: F401
from .decoder import BaseDecoder, NNDiagGaussianDecoder, NNBernoulliDecoder    # noqa: F401
