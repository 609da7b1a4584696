"""Plain-torch restatement of the full-covariance bases (MultivariateGaussian, MultivariateStudentT), for any dtype and
device: what a user without the vcnf_mvn_* kernels would write.  With L = tril(lower, -1) + diag(exp(log_diag)),
x = z - loc, y the solution of L y = x (torch.linalg.solve_triangular in the working precision: the restatement never
forms the inverse, so it is independent of the build's route) and q = |y|^2,

    Gaussian   -D/2 log 2 pi - sum log_diag - q / 2
    Student-t  lgamma((nu+D)/2) - lgamma(nu/2) - D/2 log(nu pi) - sum log_diag - (nu+D)/2 log1p(q / nu),  nu = exp(log_df)

The parameters p are a dict loc, log_diag [1, D], lower [D, D] and, for the t, log_df [1].  The normaliser is computed in
fp64 whatever the dtype of p and then cast.  Sampling maps a standard-normal draw eps [B, D] and, for the t, a gamma draw
[B] ~ Gamma(nu/2, 1) to z = loc + s L eps, s = sqrt(nu / (2 gamma)) (Gaussian: s = 1), with the density evaluated at
q = s^2 |eps|^2.

Also the seeded inputs the tests share: loc ~ 2 N(0, 1), log_diag ~ 0.3 N(0, 1), strictly lower entries ~ 0.5 N(0, 1) /
sqrt(D), nu log-uniform on [1.5, 30], z the distribution's own draw with the first B / 8 rows multiplied by 5."""
import functools
import math
import zlib

import torch

FAMILIES = ("gaussian", "student_t")


def scale_tril(p):
    return torch.tril(p["lower"], -1) + torch.diag(torch.exp(p["log_diag"][0]))


def normaliser(family, p):
    """The terms of log p that do not depend on z, in fp64, cast to the dtype of p."""
    d = p["loc"].shape[-1]
    c = -p["log_diag"].double().sum()
    if family == "student_t":
        l64 = p["log_df"].double()[0]
        nu = torch.exp(l64)
        c = c + torch.lgamma(0.5 * (nu + d)) - torch.lgamma(0.5 * nu) - 0.5 * d * (l64 + math.log(math.pi))
    else:
        c = c - 0.5 * d * math.log(2.0 * math.pi)
    return c.to(p["loc"].dtype)


def _tail(family, q, p):
    if family == "student_t":
        nu = torch.exp(p["log_df"][0])
        return -0.5 * (nu + p["loc"].shape[-1]) * torch.log1p(q / nu)
    return -0.5 * q


def mahalanobis(z, p):
    """q [B] = |L^-1 (z - loc)|^2 by a triangular solve"""
    y = torch.linalg.solve_triangular(scale_tril(p), (z - p["loc"]).t(), upper=False)
    return (y * y).sum(0)


def log_prob(family, z, p):
    return normaliser(family, p) + _tail(family, mahalanobis(z, p), p)


def sample(family, eps, gamma, p):
    s = torch.ones_like(eps[:, 0])
    if family == "student_t":
        s = torch.sqrt(torch.exp(p["log_df"][0]) / (2.0 * gamma))
    z = p["loc"] + s[:, None] * (eps @ scale_tril(p).t())
    q = s * s * (eps * eps).sum(1)
    return z, normaliser(family, p) + _tail(family, q, p)


# ---------------------------------------------------------------- seeded inputs, one set per case
def seed_of(*case):
    return zlib.crc32(repr(case).encode())


def cast(t, dtype):
    if isinstance(t, dict):
        return {k: cast(v, dtype) for k, v in t.items()}
    return t.to(dtype) if t is not None and t.is_floating_point() else t


@functools.lru_cache(maxsize=32)
def inputs(family, d, b=1000):
    """(params, eps, gamma or None, z) in fp64; z = the distribution's own draw, the first b // 8 rows x 5.
    Shared between tests: do not modify."""
    g = torch.Generator().manual_seed(seed_of("mvn", family, d))
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    p = {"loc": 2.0 * r(1, d), "log_diag": 0.3 * r(1, d), "lower": torch.tril(0.5 * r(d, d) / math.sqrt(d), -1)}
    gamma = None
    un = torch.rand(1, generator=g, dtype=torch.float64)
    if family == "student_t":
        p["log_df"] = math.log(1.5) + un * (math.log(30.0) - math.log(1.5))
    eps = r(b, d)
    if family == "student_t":
        gamma = torch._standard_gamma((0.5 * torch.exp(p["log_df"])).expand(b).contiguous(), generator=g)
    z, _ = sample(family, eps, gamma, p)
    z = z.clone()
    z[: b // 8] *= 5.0
    return p, eps, gamma, z
