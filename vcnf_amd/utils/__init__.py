from . import masks, splines, preprocessing, eval                # noqa: F401
from .masks import (create_alternating_binary_mask, create_mid_split_binary_mask,   # noqa: F401
                    create_random_binary_mask)
from .nn import sum_except_batch                                 # noqa: F401
from .preprocessing import Logit, Jitter, Scale                  # noqa: F401
from .eval import bits_per_dim                                   # noqa: F401
