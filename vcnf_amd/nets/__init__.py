from .mlp import MLP                                   # noqa: F401
from .resnet import ResidualBlock, ResidualNet, ConvResidualNet         # noqa: F401
from .cnn import ConvNet2d                             # noqa: F401
from .made import MADE                                 # noqa: F401
# last: varquant runs its flows with the model container's walks (vcnf_amd.core), which imports the nets above
from .varquant import Dequantization, VariationalDequantization         # noqa: F401
