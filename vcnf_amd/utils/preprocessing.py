"""Data preprocessing callables (normflow 1.2 utils/preprocessing.py): plain objects over torch ops, so that they work
inside a dataloader on CPU tensors.  The image recipe is ``Jitter`` (uniform dequantisation of x / 255), ``Scale`` (into
[0, 1)) and a logit; inside a model that last step, with its log-det, is ``vcnf_amd.transforms.Logit``, whose
``inverse_u8`` does all three from the bytes in one kernel launch."""
import torch


class Logit:
    """``log(x_ / (1 - x_))`` with ``x_ = alpha + (1 - alpha) x``; ``inverse`` maps back."""

    def __init__(self, alpha=0):
        self.alpha = alpha

    def __call__(self, x):
        x_ = self.alpha + (1 - self.alpha) * x
        return torch.log(x_ / (1 - x_))

    def inverse(self, x):
        return (torch.sigmoid(x) - self.alpha) / (1 - self.alpha)


class Jitter:
    """Adds uniform noise on [0, scale): dequantises data with steps of ``scale``."""

    def __init__(self, scale=1. / 256):
        self.scale = scale

    def __call__(self, x):
        return x + torch.rand_like(x) * self.scale


class Scale:
    def __init__(self, scale=255. / 256):
        self.scale = scale

    def __call__(self, x):
        return x * self.scale
