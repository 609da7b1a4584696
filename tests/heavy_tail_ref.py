"""Plain-torch restatement of the heavy-tailed product bases (StudentT, GeneralizedGaussian), for any dtype and device:
what a user without the vcnf_tail_* kernels would write.  With u = (z - loc) / exp(log_scale), per feature

    Student-t             c(nu) - log_scale - (nu + 1) / 2 log1p(u^2 / nu),  c = lgamma((nu+1)/2) - lgamma(nu/2) - log(nu pi) / 2
    generalised Gaussian  c(beta) - log_scale - |u|^beta,                    c = log beta - log 2 - lgamma(1 / beta)

The parameters p are a dict loc, log_scale and log_df / log_beta, each [1, *shape].  The normaliser c is computed in fp64
whatever the dtype of p and then cast (in fp32 the two lgamma terms cancel for large nu).  Sampling maps a standard-normal
draw eps and a gamma draw to u = eps sqrt(nu / (2 gamma)), gamma ~ Gamma(nu/2, 1), or u = sign(eps) gamma^(1/beta),
gamma ~ Gamma(1/beta, 1), where |u|^beta = gamma is used as is.

Also the seeded inputs the tests share: loc ~ 2 N(0, 1), log_scale ~ 0.3 N(0, 1), nu log-uniform on [1.5, 30], beta uniform
on [0.6, 2.5], z the distribution's own draw with the first B / 8 rows multiplied by 25."""
import functools
import math
import zlib

import torch

FAMILIES = ("student_t", "gen_gaussian")
TAIL = {"student_t": "log_df", "gen_gaussian": "log_beta"}
# part of every seed.  Chosen so that the restatement itself is finite on every case of the tests, gradients and fp32
# included: among the 17 million elements of the largest case an fp32 z can round onto its loc, and at u == 0 torch's
# autograd gives NaN for beta < 1 (the tests cover u == 0 on inputs of their own)
SALT = 0


def normaliser(family, log_tail):
    """c of the family, in fp64, cast to the dtype of log_tail."""
    l64 = log_tail.double()
    if family == "student_t":
        nu = torch.exp(l64)
        c = torch.lgamma(0.5 * (nu + 1.0)) - torch.lgamma(0.5 * nu) - 0.5 * (l64 + math.log(math.pi))
    else:
        c = l64 - math.log(2.0) - torch.lgamma(torch.exp(-l64))
    return c.to(log_tail.dtype)


def concentration(family, log_tail):
    tail = torch.exp(log_tail)
    return 0.5 * tail if family == "student_t" else 1.0 / tail


def _sum(t):
    return t.reshape(len(t), -1).sum(1)


def log_prob(family, z, p):
    log_tail = p[TAIL[family]]
    tail = torch.exp(log_tail)
    u = (z - p["loc"]) / torch.exp(p["log_scale"])
    if family == "student_t":
        f = -0.5 * (tail + 1.0) * torch.log1p(u * u / tail)
    else:
        f = -torch.abs(u) ** tail
    return _sum(normaliser(family, log_tail) - p["log_scale"] + f)


def sample(family, eps, gamma, p):
    log_tail = p[TAIL[family]]
    tail = torch.exp(log_tail)
    if family == "student_t":
        u = eps * torch.sqrt(tail / (2.0 * gamma))
        f = -0.5 * (tail + 1.0) * torch.log1p(u * u / tail)
    else:
        u = torch.sign(eps) * gamma ** (1.0 / tail)
        f = -gamma
    z = p["loc"] + torch.exp(p["log_scale"]) * u
    return z, _sum(normaliser(family, log_tail) - p["log_scale"] + f)


# ---------------------------------------------------------------- seeded inputs, one set per case
def seed_of(*case):
    return zlib.crc32(repr(case).encode())


def cast(t, dtype):
    if isinstance(t, dict):
        return {k: cast(v, dtype) for k, v in t.items()}
    return t.to(dtype) if t.is_floating_point() else t


@functools.lru_cache(maxsize=8)
def inputs(family, shape, b=4096, tails=True):
    """(params, eps, gamma, z) in fp64; z = the distribution's own draw, the first b // 8 rows x 25 with ``tails``.
    Shared between tests: do not modify."""
    shape = (shape,) if isinstance(shape, int) else tuple(shape)
    g = torch.Generator().manual_seed(seed_of("heavy_tail", SALT, family, shape))
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    un = torch.rand(1, *shape, generator=g, dtype=torch.float64)
    if family == "student_t":
        log_tail = math.log(1.5) + un * (math.log(30.0) - math.log(1.5))
    else:
        log_tail = torch.log(0.6 + un * (2.5 - 0.6))
    p = {"loc": 2.0 * r(1, *shape), "log_scale": 0.3 * r(1, *shape), TAIL[family]: log_tail}
    eps = r(b, *shape)
    gamma = torch._standard_gamma(concentration(family, log_tail).expand(b, *shape).contiguous(), generator=g)
    z, _ = sample(family, eps, gamma, p)
    if tails:
        z = z.clone()
        z[: b // 8] *= 25.0
    return p, eps, gamma, z
