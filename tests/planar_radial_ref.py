"""Plain-torch restatement of the Planar and Radial flows of normflow 1.2 (flows/planar.py, flows/radial.py), for any
dtype and device: what a user without the vcnf_planar_radial_* kernels would write.  z is [B, *shape], D = prod(shape),
sums run over the D features of a sample, a layer is a dict with its ``kind`` ("tanh", "leaky_relu" or "radial") and its
parameters under the modules' names (u, w [1, *shape], b [1]; z_0 [1, *shape], alpha, beta [1]).

    planar   lin = sum(w z) + b,  inner = sum(w u),  u_hat = u + (log(1 + exp(inner)) - 1 - inner) w / sum(w^2)
             z' = z + u_hat h(lin),  log_det = log|1 + sum(w u_hat) h'(lin)|
             inverse (leaky_relu): a = 1 or the slope where lin < 0, s = sum(w a u_hat),
             z' = z - a u_hat lin / (1 + s),  log_det = -log|1 + s|
    radial   beta_eff = log(1 + exp(beta)) - |alpha|,  dz = z - z_0,  r = |dz|,  h = beta_eff / (|alpha| + r),
             h' = -beta_eff r / (|alpha| + r)^2,  z' = z + h dz,  log_det = (D - 1) log(1 + h) + log(1 + h + h')

Also the seeded inputs the tests share: z ~ N(0, 1); planar u ~ U(-sqrt 2, sqrt 2), w ~ U(-sqrt(2 / D), sqrt(2 / D)),
b ~ 0.5 N(0, 1); radial alpha ~ 0.5 + U(-1 / D, 1 / D), beta ~ U(-1 / D - 1, 1 / D - 1), z_0 ~ N(0, 1).  Near the kinks
(lin = 0 of a leaky_relu layer, r = 0 of a radial layer) an fp32 result depends on one rounding: ``kink_rows`` marks the
rows whose fp64 trace comes within 1e-4 of one, which the comparisons leave out."""
import functools
import math
import zlib

import torch

SLOPE = 0.2
KINDS = ("tanh", "leaky_relu", "radial")
KINK = 1e-4


def _sum(t):
    return t.reshape(len(t), -1).sum(1)


def _col(t, like):
    return t.reshape((-1,) + (1,) * (like.dim() - 1))


def u_hat(p):
    inner = torch.sum(p["w"] * p["u"])
    return p["u"] + (torch.log(1 + torch.exp(inner)) - 1 - inner) * p["w"] / torch.sum(p["w"] ** 2)


def planar_forward(z, p):
    """(z', log_det [B], lin [B])"""
    lin = _sum(p["w"] * z) + p["b"]
    u = u_hat(p)
    if p["kind"] == "tanh":
        h, h_ = torch.tanh(lin), 1 / torch.cosh(lin) ** 2
    else:
        h_ = torch.where(lin < 0, torch.full_like(lin, SLOPE), torch.ones_like(lin))
        h = h_ * lin
    return z + u * _col(h, z), torch.log(torch.abs(1 + torch.sum(p["w"] * u) * h_)), lin


def planar_inverse(z, p):
    """(z', log_det [B]) of a leaky_relu layer, z on the layer's output side."""
    assert p["kind"] == "leaky_relu"
    lin = _sum(p["w"] * z) + p["b"]
    a = torch.where(lin < 0, torch.full_like(lin, SLOPE), torch.ones_like(lin))
    u = _col(a, z) * u_hat(p)
    s = _sum(p["w"] * u)
    return z - u * _col(lin / (1 + s), z), -torch.log(torch.abs(1 + s))


def radial_forward(z, p):
    """(z', log_det [B], r [B])"""
    d = z[0].numel()
    alpha = torch.abs(p["alpha"])
    beta = torch.log(1 + torch.exp(p["beta"])) - alpha
    dz = z - p["z_0"]
    r = torch.sqrt(_sum(dz * dz))
    h = beta / (alpha + r)
    h_ = -beta * r / (alpha + r) ** 2
    return z + _col(h, z) * dz, (d - 1) * torch.log(1 + h) + torch.log(1 + h + h_), r


def layer_forward(z, p):
    return radial_forward(z, p) if p["kind"] == "radial" else planar_forward(z, p)


def forward(z, layers):
    """(z', summed log_det [B], trace [K, B]) of the layers applied first to last."""
    log_det = torch.zeros(len(z), dtype=z.dtype, device=z.device)
    trace = []
    for p in layers:
        z, ld, t = layer_forward(z, p)
        log_det = log_det + ld
        trace.append(t)
    return z, log_det, torch.stack(trace)


def inverse(z, layers):
    """(z', summed log_det [B]) of the leaky_relu layers inverted last to first."""
    log_det = torch.zeros(len(z), dtype=z.dtype, device=z.device)
    for p in reversed(layers):
        z, ld = planar_inverse(z, p)
        log_det = log_det + ld
    return z, log_det


def gaussian_log_prob(z, loc=None, log_scale=None):
    """log density of N(loc, diag(exp(log_scale))^2), the standard normal by default."""
    d = z[0].numel()
    if loc is None:
        return -0.5 * d * math.log(2 * math.pi) - _sum(0.5 * z * z)
    return -0.5 * d * math.log(2 * math.pi) - _sum(log_scale + 0.5 * ((z - loc) / torch.exp(log_scale)) ** 2)


def sample_from(eps, layers):
    """(z, log q(z)) of the flow over a standard-normal base at the base draw eps."""
    z, log_det, _ = forward(eps, layers)
    return z, gaussian_log_prob(eps) - log_det


def kink_rows(trace64, layers):
    """[B] bool: rows whose fp64 trace is within KINK of lin = 0 in a leaky_relu layer or of r = 0 in a radial layer."""
    out = torch.zeros(trace64.shape[1], dtype=torch.bool)
    for k, p in enumerate(layers):
        if p["kind"] != "tanh":
            out |= trace64[k].abs().cpu() < KINK
    return out


# ---------------------------------------------------------------- seeded inputs, one set per case
def seed_of(*case):
    return zlib.crc32(repr(case).encode())


def cast(t, dtype, device=None):
    if isinstance(t, (list, tuple)):
        return [cast(v, dtype, device) for v in t]
    if isinstance(t, dict):
        return {k: cast(v, dtype, device) for k, v in t.items()}
    if not torch.is_tensor(t):
        return t
    return t.to(dtype=dtype if t.is_floating_point() else None, device=device)


def kinds_of(stack, k):
    """The layer kinds of the named stacks: "tanh", "leaky_relu", "radial", or "mixed" cycling the three."""
    return [KINDS[i % 3] if stack == "mixed" else stack for i in range(k)]


def make_layer(kind, shape, g):
    d = int(torch.tensor(shape).prod())
    un = lambda lo, hi, *s: lo + (hi - lo) * torch.rand(*s, generator=g, dtype=torch.float64)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    if kind == "radial":
        return {"kind": kind, "alpha": 0.5 + un(-1.0 / d, 1.0 / d, 1), "beta": un(-1.0 / d - 1.0, 1.0 / d - 1.0, 1),
                "z_0": rn(1, *shape)}
    lw = math.sqrt(2.0 / d)
    return {"kind": kind, "u": un(-math.sqrt(2.0), math.sqrt(2.0), 1, *shape), "w": un(-lw, lw, 1, *shape), "b": 0.5 * rn(1)}


@functools.lru_cache(maxsize=64)
def inputs(stack, shape, k, b):
    """(layers, z [b, *shape], g_z like z, g_ld [b]) in fp64.  Shared between tests: do not modify."""
    shape = (shape,) if isinstance(shape, int) else tuple(shape)
    g = torch.Generator().manual_seed(seed_of("planar_radial", stack, shape, k, b))
    layers = [make_layer(kind, shape, g) for kind in kinds_of(stack, k)]
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    return layers, rn(b, *shape), rn(b, *shape), rn(b)


def leaves(layers):
    """The layers with their parameters as fresh leaf tensors that require grad."""
    return [{n: (v.detach().clone().requires_grad_(True) if torch.is_tensor(v) else v) for n, v in p.items()} for p in layers]


def gradients(layers, z, g_z, g_ld, dtype):
    """Autograd on the restatement in ``dtype``: (z', log_det, trace, d z, [per layer {name: gradient}]) of
    (z' g_z).sum() + (log_det g_ld).sum(); a cotangent may be None."""
    ls = leaves(cast(layers, dtype))
    x = z.to(dtype).clone().requires_grad_(True)
    out, ld, trace = forward(x, ls)
    loss = 0
    if g_z is not None:
        loss = loss + (out * g_z.to(dtype)).sum()
    if g_ld is not None:
        loss = loss + (ld * g_ld.to(dtype)).sum()
    loss.backward()
    grads = [{n: v.grad for n, v in p.items() if torch.is_tensor(v)} for p in ls]
    return out.detach(), ld.detach(), trace.detach(), x.grad, grads
