"""Plain-torch restatement of the three 2-D targets of normflow 1.2 (normflows/distributions/target.py), written as the
reference writes them: torch.norm, torch.abs, the torch.cat of per-component columns, torch.logsumexp, log(1 + exp(.)).
The score is autograd's.  It computes in the dtype of ``z`` on the device of ``z``; the tests run it on the CPU in fp32
and fp64 and compare the kernels of csrc/target_density.hip against it."""
import functools
import zlib

import numpy as np
import torch

FAMILIES = ("two_moons", "circular", "ring")
MAX_LOG_PROB = 0.0                   # of TwoMoons and RingMixture; the circular mixture samples its modes directly
PROP_SCALE, PROP_SHIFT = 6.0, -3.0   # the proposal box [-3, 3]^2 of Target
TIE_BAND = 1e-3                      # |log p - max_log_prob - log u| below which a draw counts as near a tie
DRAWS = 20000
FIXED_ROWS = ((0.0, 0.0), (0.0, 2.0), (2.0, 0.0), (-2.0, 0.0), (0.0, -1e-3), (6.0, 6.0), (-0.0, 1.0))


def scale_of(family, n):
    """The mixture's standard deviation as the reference creates it: an fp64 0-dim tensor / a Python float."""
    if family == "circular":
        return torch.tensor(2 / 3 * np.sin(np.pi / n))
    if family == "ring":
        return 1 / 4 / n
    return None


def log_prob(family, n, z, scale=None):
    """``scale``: the circular mixture's buffer where the caller keeps it on the device of z, as the reference's module
    does; otherwise scale_of(family, n)."""
    if family == "two_moons":
        a = torch.abs(z[:, 0])
        return (-0.5 * ((torch.norm(z, dim=1) - 2) / 0.2) ** 2
                - 0.5 * ((a - 2) / 0.3) ** 2
                + torch.log(1 + torch.exp(-4 * a / 0.09)))
    if scale is None:
        scale = scale_of(family, n)
    d = torch.zeros((len(z), 0), dtype=z.dtype, device=z.device)
    if family == "circular":
        scale = scale.to(z.device)
        for i in range(n):
            d_ = ((z[:, 0] - 2 * np.sin(2 * np.pi / n * i)) ** 2
                  + (z[:, 1] - 2 * np.cos(2 * np.pi / n * i)) ** 2) / (2 * scale ** 2)
            d = torch.cat((d, d_[:, None]), 1)
        return -torch.log(2 * np.pi * scale ** 2 * n) + torch.logsumexp(-d, 1)
    for i in range(n):
        d_ = ((torch.norm(z, dim=1) - 2 / n * (i + 1)) ** 2) / (2 * scale ** 2)
        d = torch.cat((d, d_[:, None]), 1)
    return torch.logsumexp(-d, 1)


def score(family, n, z):
    """d log p / d z by autograd: torch's gradients of norm and abs are 0 at 0."""
    x = z.detach().clone().requires_grad_(True)
    return torch.autograd.grad(log_prob(family, n, x).sum(), x)[0]


def gradients(family, n, z, g, dtype):
    """(log p [B], score [B, 2], d (g . log p) / d z [B, 2]) of the restatement in ``dtype``."""
    x = z.to(dtype).clone().requires_grad_(True)
    lp = log_prob(family, n, x)
    grad = torch.autograd.grad((lp * g.to(dtype)).sum(), x)[0]
    return lp.detach(), score(family, n, z.to(dtype)), grad


def proposals(eps):
    return PROP_SCALE * eps + PROP_SHIFT


def accept(family, n, eps, u):
    """(proposals z_, accept mask, near-tie mask) of one rejection step of Target with the uniform draws eps, u."""
    z_ = proposals(eps)
    lp = log_prob(family, n, z_) - MAX_LOG_PROB
    return z_, torch.exp(lp) > u, (lp - torch.log(u)).abs() < TIE_BAND


def seed_of(*case):
    return zlib.crc32(repr(case).encode())


def nan_row(z):
    """z with one NaN row appended, for forward-only comparisons."""
    return torch.cat([z, torch.tensor([[float("nan"), 1.0]], dtype=z.dtype, device=z.device)], 0)


@functools.lru_cache(maxsize=None)
def inputs(family, n_comp, b):
    """(z [b, 2], g [b], eps [DRAWS, 2], u [DRAWS]) in fp64.  z starts with the first min(b, 7) of FIXED_ROWS - r == 0,
    on the moons' and rings' crest, either side of z0 == 0 including -0., next to r == 0, far out - and goes on with
    randn * 1.5 for one half of the other rows and randn * 3 for the other half, none of them with r < 1e-3 (r == 0 is
    the only kink).  eps and u are uniform draws for the acceptance tests.  Shared between tests: do not modify."""
    g = torch.Generator().manual_seed(seed_of("target", family, n_comp, b))
    fixed = torch.tensor(FIXED_ROWS[:b], dtype=torch.float64)
    rest = b - len(fixed)
    z = torch.randn(rest, 2, generator=g, dtype=torch.float64)
    z[:rest // 2] *= 1.5
    z[rest // 2:] *= 3.0
    while True:
        near = torch.norm(z, dim=1) < 1e-3
        if not near.any():
            break
        z[near] = torch.randn(int(near.sum()), 2, generator=g, dtype=torch.float64)
    z = torch.cat([fixed, z], 0)
    cot = torch.randn(b, generator=g, dtype=torch.float64)
    eps = torch.rand(DRAWS, 2, generator=g, dtype=torch.float64)
    u = torch.rand(DRAWS, generator=g, dtype=torch.float64)
    return z, cot, eps, u
