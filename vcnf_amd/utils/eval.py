"""Evaluation helpers."""
import math


def bits_per_dim(log_prob, dims, levels=256):
    """Bits per dimension of data with ``dims`` elements per item and ``levels`` quantisation levels, from the model's
    log density (in nats) of the data dequantised to [0, 1): ``-log_prob / (dims ln 2) + log2(levels)``.  The first term
    is the density's code length per element in bits; the second accounts for the factor ``levels`` between a unit
    step of the data and a step of the [0, 1) scale.  ``log_prob`` is a tensor or a number.

    This is this project's own helper with the standard definition: it does not restate the reference's
    ``utils/eval.py`` (``bitsPerDim`` / ``bitsPerDimDataset``), whose dataset loop is out of scope."""
    return -log_prob / (dims * math.log(2)) + math.log2(levels)
