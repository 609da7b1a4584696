"""Plain-torch restatement of the flow VAE's end caps (csrc/vae_ends.hip) and of the NormalizingFlowVAE container, written
with repeat / unsqueeze and without log(exp(.)): what the kernels and the modules are compared against.  N = B S rows, row n
belongs to data item n // S; a parameter tensor is h = [mean | lv] along dim 1 (lv the log variance).  Nothing here
imports vcnf_amd."""
import math
import zlib

import torch
import torch.nn.functional as F

LOG_2PI = math.log(2 * math.pi)
KINDS = ("encode", "gauss_z", "gauss_x", "bernoulli")
NEGATIVE_SLOPE = 0.2


def seed_of(*key):
    return zlib.crc32(repr(key).encode())


def cast(t, dtype):
    if isinstance(t, dict):
        return {k: cast(v, dtype) for k, v in t.items()}
    return t.to(dtype) if torch.is_tensor(t) and t.is_floating_point() else t


def feature_shape(shape):
    return (shape,) if isinstance(shape, int) else tuple(shape)


def params(rows, shape, g):
    """h [rows, 2 C, ...] = [mean ~ 2 N(0, 1) | lv ~ N(0, 1)]."""
    shape = feature_shape(shape)
    mean = 2.0 * torch.randn((rows,) + shape, generator=g, dtype=torch.float64)
    lv = torch.randn((rows,) + shape, generator=g, dtype=torch.float64)
    return torch.cat([mean, lv], 1)


def inputs(kind, B, S, shape):
    """Seeded fp64 inputs of one end cap:
    encode     h [B, 2 C, ...], eps [B, S, C, ...]
    gauss_z    v [B S, C, ...] (the latents), h [B, 2 C, ...]          the encoder's log_prob: v_div = 1, h_div = S
    gauss_x    v [B, C, ...] (the data), h [B S, 2 C, ...]             the Gaussian decoder: v_div = S, h_div = 1
    bernoulli  x [B, C, ...] uniform on [0, 1] with item 0 all 0 and item 1 all 1, score [B S, C, ...] ~ 3 N(0, 1)"""
    assert kind in KINDS
    shape = feature_shape(shape)
    g = torch.Generator().manual_seed(seed_of(kind, B, S, shape))
    randn = lambda *lead: torch.randn(tuple(lead) + shape, generator=g, dtype=torch.float64)
    if kind == "encode":
        return {"h": params(B, shape, g), "eps": randn(B, S)}
    if kind == "gauss_z":
        return {"h": params(B, shape, g), "v": randn(B * S)}
    if kind == "gauss_x":
        return {"h": params(B * S, shape, g), "v": randn(B)}
    x = torch.rand((B,) + shape, generator=g, dtype=torch.float64)
    x[0] = 0.0
    if B > 1:
        x[1] = 1.0
    return {"x": x, "score": 3.0 * randn(B * S)}


def split(h):
    c = h.shape[1] // 2
    return h[:, :c], h[:, c:]


def _sum(t, first):
    return t.sum(list(range(first, t.dim()))) if t.dim() > first else t


def encode(h, eps):
    """(z [B, S, ...], log q [B, S])."""
    mean, lv = split(h)
    mean, lv = mean.unsqueeze(1), lv.unsqueeze(1)
    z = mean + torch.exp(0.5 * lv) * eps
    d = eps[0, 0].numel()
    return z, -0.5 * d * LOG_2PI - _sum(0.5 * lv + 0.5 * eps ** 2, 2)


def repeat_rows(t, times):
    """Row b of t in the rows b * times ... (b + 1) * times - 1."""
    return t.unsqueeze(1).repeat(1, times, *([1] * (t.dim() - 1))).reshape((-1,) + tuple(t.shape[1:]))


def gauss_log_prob(v, h, v_div=1, h_div=1):
    """[N]: row n reads v[n // v_div] and h[n // h_div]."""
    v, h = repeat_rows(v, v_div), repeat_rows(h, h_div)
    mean, lv = split(h)
    d = v[0].numel()
    return -0.5 * d * LOG_2PI - 0.5 * _sum(lv + (v - mean) ** 2 * torch.exp(-lv), 1)


def log_sigmoid(a):
    return -torch.relu(-a) - torch.log1p(torch.exp(-torch.abs(a)))


def bernoulli_log_prob(x, score, x_div=1):
    x = repeat_rows(x, x_div).reshape(score.shape)
    return _sum(x * log_sigmoid(score) + (1 - x) * log_sigmoid(-score), 1)


# ---------------------------------------------------------------- the container
def planar_leaky(z, u, w, b):
    """Planar layer with leaky_relu: (z', log|det|)."""
    lin = torch.sum(w * z, 1) + b
    inner = torch.sum(w * u)
    u_hat = u + (torch.log(1 + torch.exp(inner)) - 1 - inner) * w / torch.sum(w ** 2)
    h_ = torch.where(lin < 0, torch.full_like(lin, NEGATIVE_SLOPE), torch.ones_like(lin))
    return z + u_hat * (h_ * lin).unsqueeze(1), torch.log(torch.abs(1 + torch.sum(w * u_hat) * h_))


def diag_gaussian_log_prob(z, loc, log_scale):
    return -0.5 * z[0].numel() * LOG_2PI - torch.sum(log_scale + 0.5 * ((z - loc) / torch.exp(log_scale)) ** 2, 1)


def container(sd, x, eps, n_flows, prior_log_prob=None):
    """NormalizingFlowVAE.forward for the test model - a Linear encoder (q0.net), n_flows leaky_relu Planar layers, a
    Linear Bernoulli decoder (decoder.net) and a DiagGaussian prior (prior.loc, prior.log_scale; or ``prior_log_prob``) -
    from its state dict ``sd``, the data x [B, D_x] and the encoder's draw eps [B, S, d]: (z, log_q, log_p) as [B, S, ...]."""
    b, s = eps.shape[:2]
    z, log_q = encode(F.linear(x, sd["q0.net.weight"], sd["q0.net.bias"]), eps)
    z, log_q = z.reshape(b * s, -1), log_q.reshape(-1)
    for i in range(n_flows):
        z, log_det = planar_leaky(z, *(sd["flows.%d.%s" % (i, n)] for n in "uwb"))
        log_q = log_q - log_det
    if prior_log_prob is None:
        log_p = diag_gaussian_log_prob(z, sd["prior.loc"], sd["prior.log_scale"])
    else:
        log_p = prior_log_prob(z)
    log_p = log_p + bernoulli_log_prob(x, F.linear(z, sd["decoder.net.weight"], sd["decoder.net.bias"]), s)
    return z.reshape(b, s, -1), log_q.reshape(b, s), log_p.reshape(b, s)


def container_grads(sd, x, eps, n_flows, prior_log_prob=None):
    """((z, log_q, log_p), {name: d loss / d sd[name]}) for loss = mean(log_q) - mean(log_p)."""
    leaves = {k: v.detach().clone().requires_grad_() for k, v in sd.items()}
    out = container(leaves, x, eps, n_flows, prior_log_prob)
    (out[1].mean() - out[2].mean()).backward()
    return tuple(t.detach() for t in out), {k: v.grad for k, v in leaves.items()}
