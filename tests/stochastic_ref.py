"""Plain-torch restatement of the stochastic layers of normflow 1.2 (normflows/flows/stochastic.py) as the reference
writes them, with the draws as arguments: HamiltonianMonteCarlo (leapfrog with the detached score, the accept / reject
decision, log_det = log p(z) - log p(z_out)) and MetropolisHastings with a diagonal Gaussian proposal (log_det 0).  The
density and the score are target_ref's (the score autograd's unless another is passed).  It computes in the dtype and on
the device of ``z``; the tests run it in fp32 and fp64 and compare the kernels of csrc/stochastic.hip against it.

Also here, because the CPU tests and the GPU tests share them: the cases, their inputs and draws, the near-tie bands,
and the references computed once per case."""
import functools
import math

import torch

import target_ref as ref

DTYPES = (torch.float32, torch.float64)
DEFAULTS = (("two_moons", 0), ("circular", 8), ("ring", 2))
STIFF = (("circular", 33), ("ring", 7))                  # at step 0.1 their leapfrog diverges: (5, 0.02) only
TARGETS = DEFAULTS + STIFF
# (family, n, steps, step)
HMC_CASES = tuple((f, n, s, h) for f, n in DEFAULTS for s, h in ((1, 0.05), (8, 0.1))) + tuple((f, n, 5, 0.02) for f, n in STIFF)
BATCHES = (1, 63, 64, 65, 1000)
RUN = 3                                                  # layers of the run at B = 1000
HMC_BAND, MH_BAND, BAND_CAP = 1e-2, 1e-3, 0.02
MH_STEPS = (1, 4)
MH_SCALES = ((0.3, 0.24), (1.0, 0.8))
MH_BATCHES = (1, 65, 1000)


def hmc_parameters(step, n_layers=1, numel=2):
    """[(log_step_size, log_mass)] in fp64: log(step) + [0, 0.2] and [0.1, -0.2] for the first layer, each later layer
    of a run with a smaller step and another mass."""
    out = []
    for k in range(n_layers):
        ls = torch.tensor([math.log(step), math.log(step) + 0.2], dtype=torch.float64) - 0.1 * k
        lm = torch.tensor([0.1, -0.2], dtype=torch.float64) + 0.15 * k * torch.tensor([1.0, -1.0], dtype=torch.float64)
        out.append((ls[:numel].clone(), lm[:numel].clone()))
    return out


def hmc_draws(family, n, b, steps, n_layers=1):
    """(noise [K, b, 2], unif [K, b]) in fp64: first the noise, then the uniforms."""
    g = torch.Generator().manual_seed(ref.seed_of("hmc", family, n, b, steps))
    noise = torch.randn(n_layers, b, 2, generator=g, dtype=torch.float64)
    return noise, torch.rand(n_layers, b, generator=g, dtype=torch.float64)


def mh_draws(family, n, b, steps):
    """(eps [steps, b, 2], w [steps, b]) in fp64."""
    g = torch.Generator().manual_seed(ref.seed_of("mh", family, n, b, steps))
    eps = torch.randn(steps, b, 2, generator=g, dtype=torch.float64)
    return eps, torch.rand(steps, b, generator=g, dtype=torch.float64)


def inputs(family, n, b):
    """z [b, 2] in fp64: target_ref's rows (r == 0, on the crest, far out, ...) out of its B = 1000 set."""
    return ref.inputs(family, n, 1000)[0][:b]


def hmc_layer(family, n, z, noise, unif, log_step_size, log_mass, steps, score=ref.score, accept=None):
    """(z_out, log_det, accept, probabilities) of one layer.  ``accept``: decisions to impose in place of its own.
    Differentiable in z, log_step_size and log_mass as the reference is: the score is detached."""
    log_prob = lambda x: ref.log_prob(family, n, x)
    gradlogP = lambda x: score(family, n, x.detach())
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


def hmc_run(family, n, z, noise, unif, params, steps, score=ref.score, accept=None):
    """A run of layers: (z_out, sum of the log_dets in layer order, accept [K, B], probabilities [K, B])."""
    log_det = torch.zeros(len(z), dtype=z.dtype, device=z.device)
    masks, probs = [], []
    for k, (ls, lm) in enumerate(params):
        z, ld, mask, prob = hmc_layer(family, n, z, noise[k], unif[k], ls, lm, steps, score, None if accept is None else accept[k])
        log_det = log_det + ld
        masks.append(mask)
        probs.append(prob)
    return z, log_det, torch.stack(masks), torch.stack(probs)


def mh_walk(family, n, z, eps, w, scale):
    """(z_out, log_det = 0, accept [steps, B], min(exp(.), 1) [steps, B]) of the walk with the proposal z_ = eps scale + z."""
    log_det = torch.zeros(len(z), dtype=z.dtype, device=z.device)
    log_p = ref.log_prob(family, n, z)
    masks, ratios = [], []
    for i in range(len(eps)):
        z_ = eps[i] * scale + z
        log_p_diff = torch.zeros(len(z), dtype=z.dtype, device=z.device)
        log_p_ = ref.log_prob(family, n, z_)
        log_w_accept = log_p_ - log_p + log_p_diff
        w_accept = torch.clamp(torch.exp(log_w_accept), max=1)
        accept = w[i] <= w_accept
        z = torch.where(accept.unsqueeze(1), z_, z)
        log_p = torch.where(accept, log_p_, log_p)
        masks.append(accept)
        ratios.append(w_accept)
    empty = torch.zeros((0, len(z)), device=z.device)
    return z, log_det, (torch.stack(masks) if masks else empty.bool()), (torch.stack(ratios) if ratios else empty.to(z.dtype))


def closed_form_score(family, n, z):
    """The scores as include/vcnf_hip.h states them, in plain torch: the same mathematics as autograd's, other roundings."""
    unit = lambda v, r: torch.where(r > 0, v / torch.where(r > 0, r, torch.ones_like(r)), torch.zeros_like(v))
    z0, z1 = z[:, 0], z[:, 1]
    r = torch.sqrt(z0 ** 2 + z1 ** 2)
    if family == "two_moons":
        a = z0.abs()
        e = torch.exp(-4 * a / 0.09)
        k = -(r - 2) / 0.04
        return torch.stack([k * unit(z0, r) + torch.sign(z0) * ((2 - a) / 0.09 - (4 / 0.09) * e / (1 + e)), k * unit(z1, r)], 1)
    scale = float(ref.scale_of(family, n))
    i = torch.arange(n, dtype=z.dtype, device=z.device)
    if family == "circular":
        c = torch.stack([2 * torch.sin(2 * math.pi * i / n), 2 * torch.cos(2 * math.pi * i / n)], 1)
        diff = c[None] - z[:, None]
        wgt = torch.softmax(-(diff ** 2).sum(2) / (2 * scale ** 2), 1)
        return (wgt[:, :, None] * diff).sum(1) / scale ** 2
    t = 2 * (i + 1) / n
    wgt = torch.softmax(-(r[:, None] - t[None]) ** 2 / (2 * scale ** 2), 1)
    k = (wgt * (t[None] - r[:, None])).sum(1) / scale ** 2
    return torch.stack([k * unit(z0, r), k * unit(z1, r)], 1)


@functools.lru_cache(maxsize=None)
def hmc_reference(family, n, steps, step, b, n_layers=1):
    """The restatement of one HMC case: {"z", "noise", "unif", "params" (fp64), dtype: (z_out, log_det, accept, prob),
    "closed": the fp64 run with the closed-form scores, "near": rows in the band of any layer, "yardstick": (z_out,
    log_det) differences of the two fp64 runs}.  Shared between tests: do not modify."""
    z = inputs(family, n, b)
    noise, unif = hmc_draws(family, n, b, steps, n_layers)
    params = hmc_parameters(step, n_layers)
    out = {"z": z, "noise": noise, "unif": unif, "params": params}
    for dtype in DTYPES:                                 # nothing here requires grad: only the score's own graph exists
        out[dtype] = hmc_run(family, n, z.to(dtype), noise.to(dtype), unif.to(dtype),
                             [(ls.to(dtype), lm.to(dtype)) for ls, lm in params], steps)
    out["closed"] = hmc_run(family, n, z, noise, unif, params, steps, score=closed_form_score)
    prob = out[torch.float64][3]
    out["near"] = ((torch.clamp(prob, max=2.0) - unif).abs() < HMC_BAND).any(0)
    out["yardstick"] = tuple(float((out["closed"][j] - out[torch.float64][j]).abs().max()) for j in (0, 1))
    return out


@functools.lru_cache(maxsize=None)
def mh_reference(family, n, steps, scale, b):
    """The restatement of one MH case, like hmc_reference: {"z", "eps", "w", dtype: (z_out, log_det, accept, ratio), "near"}."""
    z = inputs(family, n, b)
    eps, w = mh_draws(family, n, b, steps)
    out = {"z": z, "eps": eps, "w": w}
    with torch.no_grad():
        for dtype in DTYPES:
            out[dtype] = mh_walk(family, n, z.to(dtype), eps.to(dtype), w.to(dtype), torch.tensor(scale, dtype=dtype))
    out["near"] = ((out[torch.float64][3] - w).abs() < MH_BAND).any(0)
    return out


def few_near(near, decisions_per_row=1):
    """What every single batch must satisfy besides its case's pooled share: the rows left out of the comparisons are at
    most the cap's share of the batch's decisions - or 2 where that is less, which is so for B <= 65 - and never the
    whole batch, so every batch compares something (a batch of one row has no near row)."""
    b, left_out = len(near), int(near.sum())
    return left_out <= max(2, int(BAND_CAP * b * decisions_per_row)) and left_out < b


def hmc_band_share(family, n, steps, step):
    """Share of a case's decisions that lie in the band, pooled over its batches (K = 1) and the layers of its run at
    B = 1000.  A batch of 65 rows has 1.5 % of its rows in the band with one near row and 3.1 % with two, whatever the
    inputs: the cap of 2 % is a statement about a case's decisions, not about how they fall into its small batches."""
    near = total = 0
    for b, k in [(b, 1) for b in BATCHES] + [(1000, RUN)]:
        r = hmc_reference(family, n, steps, step, b, k)
        band = (torch.clamp(r[torch.float64][3], max=2.0) - r["unif"]).abs() < HMC_BAND
        near, total = near + int(band.sum()), total + band.numel()
    return near / total


def mh_band_share(family, n, steps, scale):
    """Share of a case's rows with any step in the band, pooled over its batches."""
    near = sum(int(mh_reference(family, n, steps, scale, b)["near"].sum()) for b in MH_BATCHES)
    return near / sum(MH_BATCHES)


def hmc_closed_form_backward(family, n, z, noise, params, steps, accept, gz, gl, score=ref.score):
    """The closed form of include/vcnf_hip.h in torch: (g_z, [(g_log_step_size, g_log_mass)]) of a run for the cotangents
    gz of z_out and gl of the summed log_det, from each layer's entrance row, its decision and its recomputed trajectory;
    the operand gradients go on to the log parameters by the chain rule of exp."""
    rows = [z]
    for k, (ls, lm) in enumerate(params):
        rows.append(hmc_layer(family, n, rows[-1], noise[k], None, ls, lm, steps, score, accept[k])[0].detach())
    grads = [None] * len(params)
    for k in range(len(params) - 1, -1, -1):
        ls, lm = params[k]
        step, mass, sqm = torch.exp(ls), torch.exp(lm), torch.exp(0.5 * lm)
        x, a = rows[k], accept[k].to(z.dtype).unsqueeze(1)
        s = [score(family, n, x)]
        p, halves = noise[k] * sqm, []
        for i in range(steps):
            p_half = p - (step / 2.0) * -s[-1]
            x = x + step * (p_half / mass)
            s.append(score(family, n, x))
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


def plain_target(family, n):
    """A Target subclass that is none of the kernel targets: its log_prob is target_ref's, on any device."""
    import vcnf_amd as nf

    class PlainTarget(nf.distributions.Target):
        def __init__(self):
            super().__init__()
            self.n_dims = 2

        def log_prob(self, z):
            return ref.log_prob(family, n, z)
    return PlainTarget()
