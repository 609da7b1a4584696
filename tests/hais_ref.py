"""Plain-torch restatement of Hamiltonian annealed importance sampling as normflow 1.2 writes it (sampling/hais.py,
distributions/linear_interpolation.py) on top of target_ref and stochastic_ref: the annealed HamiltonianMonteCarlo
layer - the reference's layer against beta log p + (1 - beta) log N(loc, exp(log_scale)^2) - with autograd scores or the
closed-form scores of include/vcnf_hip.h, the chain of such layers, the HAIS loop with its draws from torch's generator,
and the closed-form backward.  It computes in the dtype of ``z``; the draws are arguments except in ``hais``.

Also here, because the CPU and the GPU tests share them: the cases, their inputs and draws, the near-tie band and the
references computed once per case."""
import functools
import math

import torch

import stochastic_ref as sref
import target_ref as ref

DTYPES = sref.DTYPES
LOC, LOG_SCALE = (0.3, -0.2), (0.2, 0.1)                 # the prior
CASES = sref.HMC_CASES + (("ring", 2, 4, 0.3),)          # (family, n, steps, step); the last one rejects often
MS = (4, 9)                                              # betas = linspace(1, 0, M + 1): M - 1 layers
BATCHES = sref.BATCHES
# Salts of the draws' seeds, 0 where not listed; both were chosen by properties of the restatement alone, never by what a
# kernel gives (test_hais_abi.test_near_ties asserts the two properties for every run).
#  - ring-2, 1 step, B = 63: a row is left out when any of its K decisions is in the band, which about 1 % of the
#    decisions are, and with salt 0 this small batch has more such rows than few_near allows.
#  - ring-2, 4 steps of 0.3, B = 1000, M = 9: the case that rejects often is stiff, and over eight layers a few rows per
#    thousand have a leapfrog that amplifies rounding by 1e3 - 1e4.  There the fp32 restatement's own probability is far
#    from the fp64 one - with salt 0 by 0.085 in row 500, eight band widths, where |prob - unif| is 0.156 - so fp32
#    cannot tell which way such a decision goes, and on an MI355X the fp32 kernel, 3e-3 from the fp64 row after the
#    amplifying layer where the fp32 restatement is 7e-4 from it, decided that row the other way.  The comparison of
#    decisions is well posed in fp32 where every decision outside the band keeps |prob64 - unif| > 8 |prob32 - prob64|
#    (the factor helpers.parity grants an fp32 result over the reference's own fp32 noise).  In every other run
#    |prob32 - prob64| is at most 0.009 of that margin; of this run's seeds few satisfy it (salts 0 - 159 do not, the
#    ratio is 0.1 to 28 there), 160 is the first, with 0.098.
SALTS = {("ring", 2, 1, 63, 4): 1, ("ring", 2, 4, 1000, 9): 160}


def prior_parameters(dtype=torch.float64):
    return torch.tensor(LOC, dtype=dtype), torch.tensor(LOG_SCALE, dtype=dtype)


def prior_log_prob(z, loc, log_scale):
    """normflow's DiagGaussian.log_prob over (2,) without a temperature."""
    return -0.5 * 2 * math.log(2 * math.pi) - torch.sum(log_scale + 0.5 * torch.pow((z - loc) / torch.exp(log_scale), 2), 1)


class PlainPrior:
    """A prior in plain torch with the reference's interface: forward(num_samples) -> (z, log p), log_prob(z)."""

    def __init__(self, dtype=torch.float64):
        self.loc, self.log_scale = prior_parameters(dtype)

    def forward(self, num_samples=1):
        eps = torch.randn(num_samples, 2, dtype=self.loc.dtype)
        z = self.loc + torch.exp(self.log_scale) * eps
        return z, self.log_prob(z)

    def log_prob(self, z):
        return prior_log_prob(z, self.loc, self.log_scale)


def betas_of(m, dtype=torch.float64):
    return torch.linspace(1, 0, m + 1, dtype=dtype)


def layer_betas(m, dtype=torch.float64):
    """The betas of the chain's layers in their order: betas[n - 1] ... betas[1] of sampling/hais.py."""
    betas = betas_of(m, dtype)
    return [betas[i] for i in range(m - 1, 0, -1)]


def bridge_log_prob(family, n, z, beta):
    """LinearInterpolation(target, prior, beta).log_prob."""
    loc, log_scale = prior_parameters(z.dtype)
    return beta * ref.log_prob(family, n, z) + (1 - beta) * prior_log_prob(z, loc, log_scale)


def autograd_score(family, n, z, beta):
    x = z.detach().clone().requires_grad_(True)
    logp = bridge_log_prob(family, n, x, beta)
    return torch.autograd.grad(logp, x, grad_outputs=torch.ones_like(logp))[0]


def closed_form_score(family, n, z, beta):
    """The score as include/vcnf_hip.h states it: beta st + (1 - beta) s0 with s0 = -u / sig."""
    loc, log_scale = prior_parameters(z.dtype)
    sig = torch.exp(log_scale)
    u = (z - loc) / sig
    return beta * sref.closed_form_score(family, n, z) + (1 - beta) * (-u / sig)


def annealed_layer(family, n, z, noise, unif, log_step_size, log_mass, steps, beta, score=autograd_score, accept=None):
    """stochastic_ref.hmc_layer with the bridge's density: (z_out, log_det, accept, probabilities)."""
    log_prob = lambda x: bridge_log_prob(family, n, x, beta)
    gradlogP = lambda x: score(family, n, x.detach(), beta)
    p = noise * torch.exp(0.5 * log_mass)
    z_new = z.clone()
    p_new = p.clone()
    step_size = torch.exp(log_step_size)
    for i in range(steps):
        p_half = p_new - (step_size / 2.0) * -gradlogP(z_new)
        z_new = z_new + step_size * (p_half / torch.exp(log_mass))
        p_new = p_half - (step_size / 2.0) * -gradlogP(z_new)
    probabilities = torch.exp(
        log_prob(z_new) - log_prob(z)
        - 0.5 * torch.sum(p_new ** 2 / torch.exp(log_mass), 1)
        + 0.5 * torch.sum(p ** 2 / torch.exp(log_mass), 1))
    mask = unif < probabilities if accept is None else accept
    z_out = torch.where(mask.unsqueeze(1), z_new, z)
    return z_out, log_prob(z) - log_prob(z_out), mask, probabilities.detach()


def chain(family, n, z, noise, unif, params, steps, betas, score=autograd_score, accept=None):
    """The layers in order: (z_out, sum of the log_dets in layer order, accept [K, B], probabilities [K, B])."""
    log_det = torch.zeros(len(z), dtype=z.dtype)
    masks, probs = [], []
    for k, (ls, lm) in enumerate(params):
        z, ld, mask, prob = annealed_layer(family, n, z, noise[k], unif[k], ls, lm, steps, betas[k].to(z.dtype), score,
                                           None if accept is None else accept[k])
        log_det = log_det + ld
        masks.append(mask)
        probs.append(prob)
    return z, log_det, torch.stack(masks), torch.stack(probs)


def hais_weights(family, n, z, prior_logp, noise, unif, params, steps, betas, score=autograd_score):
    """The loop of HAIS.sample from the prior draw z on: (samples, log_weights, accept, probabilities)."""
    log_weights = -prior_logp
    masks, probs = [], []
    for k, (ls, lm) in enumerate(params):
        z, add, mask, prob = annealed_layer(family, n, z, noise[k], unif[k], ls, lm, steps, betas[k].to(z.dtype), score)
        log_weights = log_weights + add
        masks.append(mask)
        probs.append(prob)
    log_weights = log_weights + ref.log_prob(family, n, z)
    return z, log_weights, torch.stack(masks), torch.stack(probs)


def hais(family, n, betas, num_samples, steps, step_size, log_mass, dtype=torch.float64):
    """sampling/hais.py's sample with its draws from torch's generator in the reference's order: the prior's randn, then
    per layer randn_like(z) and rand of [B].  (samples, log_weights)."""
    prior = PlainPrior(dtype)
    m = betas.shape[0] - 1
    samples, log_weights = prior.forward(num_samples)
    log_weights = -log_weights
    for i in range(m - 1, 0, -1):
        noise = torch.randn_like(samples)
        unif = torch.rand(num_samples, dtype=dtype)                    # rand_like(probabilities)
        samples, add, _, _ = annealed_layer(family, n, samples, noise, unif, torch.log(step_size), log_mass, steps, betas[i])
        log_weights += add
    log_weights += ref.log_prob(family, n, samples)
    return samples, log_weights


def closed_form_backward(family, n, z, noise, params, steps, betas, accept, gz, gl, score=autograd_score):
    """stochastic_ref.hmc_closed_form_backward with score_k in place of the score: (g_z, [(g_log_step_size, g_log_mass)])."""
    rows = [z]
    for k, (ls, lm) in enumerate(params):
        rows.append(annealed_layer(family, n, rows[-1], noise[k], None, ls, lm, steps, betas[k], score, accept[k])[0].detach())
    grads = [None] * len(params)
    for k in range(len(params) - 1, -1, -1):
        ls, lm = params[k]
        step, mass, sqm = torch.exp(ls), torch.exp(lm), torch.exp(0.5 * lm)
        x, a = rows[k], accept[k].to(z.dtype).unsqueeze(1)
        s = [score(family, n, x, betas[k])]
        p, halves = noise[k] * sqm, []
        for i in range(steps):
            p_half = p - (step / 2.0) * -s[-1]
            x = x + step * (p_half / mass)
            s.append(score(family, n, x, betas[k]))
            p = p_half - (step / 2.0) * -s[-1]
            halves.append(p_half)
        G = a * (gz - gl.unsqueeze(1) * s[-1])
        g_step = torch.zeros_like(G)
        g_mass = torch.zeros_like(G)
        for i in range(steps):
            g_p_half, g_p_next = (steps - i) * G * step / mass, (steps - 1 - i) * G * step / mass
            g_step = g_step + G * halves[i] / mass + g_p_half * s[i] / 2 + g_p_next * s[i + 1] / 2
            g_mass = g_mass - G * step * halves[i] / mass ** 2
        g_sqm = steps * G * step / mass * noise[k]
        gz = (1 - a) * gz + G + a * gl.unsqueeze(1) * s[0]
        g_step, g_mass, g_sqm = g_step.sum(0), g_mass.sum(0), g_sqm.sum(0)
        grads[k] = (g_step * step, g_mass * mass + g_sqm * 0.5 * sqm)
    return gz, grads


def inputs(family, n, b):
    """(eps, z) in fp64: the prior's draw and z = loc + exp(log_scale) eps, from a seeded generator."""
    g = torch.Generator().manual_seed(ref.seed_of("hais-prior", family, n, b))
    eps = torch.randn(b, 2, generator=g, dtype=torch.float64)
    loc, log_scale = prior_parameters()
    return eps, loc + torch.exp(log_scale) * eps


def draws(family, n, b, steps, m):
    """(noise [K, b, 2], unif [K, b]) in fp64 for the K = m - 1 layers."""
    g = torch.Generator().manual_seed(ref.seed_of("hais", family, n, b, steps, m, SALTS.get((family, n, steps, b, m), 0)))
    noise = torch.randn(m - 1, b, 2, generator=g, dtype=torch.float64)
    return noise, torch.rand(m - 1, b, generator=g, dtype=torch.float64)


@functools.lru_cache(maxsize=None)
def reference(family, n, steps, step, b, m):
    """The restatement of one case like stochastic_ref.hmc_reference: {"z", "noise", "unif", "params", "betas" (fp64),
    dtype: (z_out, log_det, accept, prob), "closed": the fp64 chain with the closed-form scores, "band": decisions in the
    band [K, B], "near": rows with one, "yardstick": (z_out, log_det) differences of the two fp64 chains}.  Shared between
    tests: do not modify."""
    z = inputs(family, n, b)[1]
    noise, unif = draws(family, n, b, steps, m)
    params = sref.hmc_parameters(step, m - 1)
    betas = layer_betas(m)
    out = {"z": z, "noise": noise, "unif": unif, "params": params, "betas": torch.stack(betas)}
    for dtype in DTYPES:
        out[dtype] = chain(family, n, z.to(dtype), noise.to(dtype), unif.to(dtype),
                           [(ls.to(dtype), lm.to(dtype)) for ls, lm in params], steps, betas)
    out["closed"] = chain(family, n, z, noise, unif, params, steps, betas, score=closed_form_score)
    prob = out[torch.float64][3]
    out["band"] = (torch.clamp(prob, max=2.0) - unif).abs() < sref.HMC_BAND
    out["near"] = out["band"].any(0)
    out["yardstick"] = tuple(float((out["closed"][j] - out[torch.float64][j]).abs().max()) for j in (0, 1))
    return out


def fp32_resolves(r):
    """Whether fp32 can tell every decision of the reference ``r`` outside the band: |prob64 - unif| > 8 |prob32 - prob64|
    with the probabilities clamped at 2 as the band's are.  Returns (holds, largest |prob32 - prob64| / |prob64 - unif|)."""
    p64, p32 = torch.clamp(r[torch.float64][3], max=2.0), torch.clamp(r[torch.float32][3].double(), max=2.0)
    ratio = ((p32 - p64).abs() / (p64 - r["unif"]).abs())[~r["band"]]
    worst = float(ratio.max()) if ratio.numel() else 0.0
    return 8.0 * worst < 1.0, worst


def runs_of(case):
    """(b, m) of the forward tests: every batch at M = 4 and B = 1000 at M = 9."""
    return [(b, MS[0]) for b in BATCHES] + [(1000, MS[1])]


def band_share(case):
    """Share of a case's decisions in the band, pooled over runs_of(case)."""
    near = total = 0
    for b, m in runs_of(case):
        band = reference(*case, b, m)["band"]
        near, total = near + int(band.sum()), total + band.numel()
    return near / total
