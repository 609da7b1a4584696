"""Dequantisation of categorical columns restated in plain torch: what the varquant tests compare vcnf_amd with.

The fork's normflow/nets/varquant.py is not available to this project.  This is the published algorithm (Ho et al. 2019,
"Flow++", in the Dequantization / VariationalDequantization form) written per column, as the specification states it:
one torch op per step, Python scalars as operands, sums over the categorical columns in column order.

Rows x [B, D]; ``columns`` the C categorical column indices, ``levels`` their numbers of levels K_c >= 1; a categorical
column holds the codes k = 0 .. K_c - 1 as floating values; a = alpha in [0, 1)."""
import math

import torch
from torch.nn import functional as F

ADULT = ([1, 3, 5, 6, 7, 8, 9, 13], [9, 16, 7, 15, 6, 5, 2, 42])
WIDE = ([1, 3, 5, 6, 7, 8, 9, 13], [9, 16, 7, 15, 6, 1, 2, 1000])


def column_sum(t):
    """Sum of t [B, C] over its columns, in column order."""
    total = torch.zeros(len(t), dtype=t.dtype, device=t.device)
    for c in range(t.shape[1]):
        total = total + t[:, c]
    return total


def level_row(levels, like):
    return torch.tensor(list(levels), dtype=like.dtype, device=like.device)


def prepare(x, columns, levels, u, alpha=1e-5):
    """(v, ctx, ld) for the uniform draws u [B, C]."""
    k, big_k = x[:, columns], level_row(levels, x)
    s = alpha / 2 + (1 - alpha) * u
    log_s, log_t = torch.log(s), torch.log(1 - s)
    v = log_s - log_t
    ld = column_sum(math.log(1 - alpha) - log_s - log_t)
    ctx = torch.where(big_k > 1, 2 * k / (big_k - 1) - 1, torch.zeros_like(k))
    return v, ctx, ld


def merge_s(x, columns, levels, w, noise_is_logit, alpha=1e-5):
    """The s of merge [B, C]: the point of (0, 1) whose logit is written."""
    k, big_k = x[:, columns], level_row(levels, x)
    n = torch.sigmoid(w) if noise_is_logit else w
    y = (k + n) / big_k
    return alpha / 2 + (1 - alpha) * y


def merge(x, columns, levels, w, noise_is_logit, alpha=1e-5):
    """(out, ld) for w [B, C]: logit noise (``noise_is_logit``) or the noise itself."""
    big_k = level_row(levels, x)
    if noise_is_logit:
        ld_n = column_sum(F.logsigmoid(w) + F.logsigmoid(-w))
    else:
        ld_n = 0
    s = merge_s(x, columns, levels, w, noise_is_logit, alpha)
    log_s, log_t = torch.log(s), torch.log(1 - s)
    out = x.clone()
    out[:, columns] = log_s - log_t
    ld = ld_n + column_sum(math.log(1 - alpha) - torch.log(big_k) - log_s - log_t)
    return out, ld


def merge_terms(x, columns, levels, w, noise_is_logit, alpha=1e-5):
    """Per row: the sum of the magnitudes of the terms of merge's ld, and the sum over the columns of cond = 1/s + 1/(1-s):
    what an error bound on ld weighs."""
    big_k = level_row(levels, x)
    s = merge_s(x, columns, levels, w, noise_is_logit, alpha)
    mags = torch.log(s).abs() + torch.log(1 - s).abs() + torch.log(big_k)
    if noise_is_logit:
        mags = mags + (F.logsigmoid(w) + F.logsigmoid(-w)).abs()
    return mags.sum(1), (1 / s + 1 / (1 - s)).sum(1)


def quantize(z, columns, levels, alpha=1e-5):
    """(codes, ld): the categorical columns of z as integer codes (floating values), and the log-det of t -> y K_c."""
    t, big_k = z[:, columns], level_row(levels, z)
    y = (torch.sigmoid(t) - alpha / 2) / (1 - alpha)
    code = torch.minimum(torch.maximum(torch.floor(y * big_k), torch.zeros_like(big_k)), big_k - 1)
    out = z.clone()
    out[:, columns] = code
    ld = column_sum(F.logsigmoid(t) + F.logsigmoid(-t) - math.log(1 - alpha) + torch.log(big_k))
    return out, ld


def rows(batch, features, columns, levels, seed, dtype=torch.float64, device="cpu"):
    """Test rows [batch, features] in fp64 rounded to ``dtype``: standard-normal continuous columns, uniform random codes
    in the categorical ones, the rows 0 - 3 holding the codes K - 1, 0, K - 1, 0."""
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(batch, features, generator=gen, dtype=torch.float64)
    for c, k in zip(columns, levels):
        x[:, c] = torch.randint(0, k, (batch,), generator=gen).double()
        for r in range(min(4, batch)):
            x[r, c] = (k - 1) if r % 2 == 0 else 0
    return x.to(dtype).to(device)


def cases():
    """name -> (B, D, columns, levels) of the shapes the tests run."""
    every_second = list(range(0, 130, 2))
    return {
        "lane_per_row": (7, 1, [0], [3]),
        "one_of_three": (5, 3, [1], [2]),
        "first_and_last": (64, 14, [0, 13], [4, 11]),
        "adult": (1031, 14) + ADULT,
        "wide": (1031, 14) + WIDE,
        "long_rows": (3, 130, every_second, [2 + i % 8 for i in range(len(every_second))]),
        "empty": (0, 14) + ADULT,
    }
