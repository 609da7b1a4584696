"""Plain-torch restatement of the five energy densities of normflow 1.2 (normflows/distributions/prior.py) as the
reference writes them - torch.norm, torch.abs, norm(p=4), the last axis first for the Sinusoidal trio - with
torch.logaddexp for the two-branch log (``naive_log_prob`` keeps the reference's log(exp a + exp b)).  The score is
autograd's; ``closed_form_score`` restates the scores of include/vcnf_hip.h in torch, the same mathematics in another
rounding order, which the tests use as their fp64 yardstick.  The stochastic layers are restated here with the density
as a callable (stochastic_ref's are tied to target_ref.log_prob): HamiltonianMonteCarlo plain and annealed, the
closed-form backward and the MetropolisHastings walk.  Everything computes in the dtype of ``z``.

Also here, because the CPU and the GPU tests share them: the cases, their inputs and draws, the near-tie bands and the
references computed once per case."""
import functools
import math

import numpy as np
import torch

import target_ref as ref

DTYPES = (torch.float32, torch.float64)
# (family, parameters): TwoModes(loc, scale), Sinusoidal*(scale, period), Smiley(scale)
CASES = (("two_modes", (2.0, 0.2)), ("two_modes", (-1.5, 0.3)), ("sinusoidal", (0.4, 4.0)), ("gap", (0.4, 4.0)),
         ("split", (0.4, 4.0)), ("smiley", (0.2,)), ("sinusoidal", (0.5, 3.0)))
FAMILIES = (("two_modes", (2.0, 0.2)), ("sinusoidal", (0.4, 4.0)), ("gap", (0.4, 4.0)), ("split", (0.4, 4.0)), ("smiley", (0.2,)))
GAP = (3.0, 1.0, 0.6)                    # amp, mu, width of Sinusoidal_gap
SPLIT = (3.0, 1.0, 0.3)                  # of Sinusoidal_split
# target_ref's rows, then: Smiley's kink (the score of its |.| term is exactly 0 there), the gap's second ridge
# (w1 = 1, w = 3), both branches of the gap equal
FIXED_ROWS = ref.FIXED_ROWS + ((1.0, -0.8), (1.0, -2.0), (1.0, -0.5))
BATCHES = (1, 63, 64, 65, 1000)
HMC_STEPS = ((1, 0.05), (4, 0.3))        # (steps, step)
RUN = 3
HMC_BAND, MH_BAND, BAND_CAP = 1e-2, 1e-3, 0.02
MH_STEPS = (1, 4)
MH_SCALES = ((0.3, 0.24), (1.0, 0.8))
MH_BATCHES = (1, 65, 1000)
LOC, LOG_SCALE = (0.3, -0.2), (0.2, 0.1)                 # the prior of the annealed runs
M = 4                                                    # betas = linspace(1, 0, M + 1): M - 1 annealed layers
case_id = lambda c: "%s-%s" % (c[0], "-".join(str(p) for p in c[1])) if isinstance(c, tuple) and isinstance(c[1], tuple) else str(c)


def prior_of(case):
    """The module of a case."""
    import vcnf_amd as nf
    D = nf.distributions
    family, p = case
    return {"two_modes": D.TwoModes, "sinusoidal": D.Sinusoidal, "gap": D.Sinusoidal_gap, "split": D.Sinusoidal_split,
            "smiley": D.Smiley}[family](*p)


def _branches(case, z):
    """(a, b or None, tail) of the Sinusoidal trio, the last axis first as the reference moves it."""
    family, (scale, period) = case
    z_ = z.permute((z.dim() - 1,) + tuple(range(0, z.dim() - 1))) if z.dim() > 1 else z
    w_1 = torch.sin(2 * np.pi / period * z_[0])
    tail = 0.5 * (torch.norm(z_, dim=0, p=4) / (20 * scale)) ** 4
    a = -0.5 * ((z_[1] - w_1) / scale) ** 2
    if family == "sinusoidal":
        return a, None, tail
    if family == "gap":
        amp, mu, width = GAP
        w = amp * torch.exp(-0.5 * ((z_[0] - mu) / width) ** 2)
    else:
        amp, mu, width = SPLIT
        w = amp * torch.sigmoid((z_[0] - mu) / width)
    return a, -0.5 * ((z_[1] - w_1 + w) / scale) ** 2, tail


def log_prob(case, z):
    family, p = case
    if family == "two_modes":
        loc, scale = p
        a = torch.abs(z[:, 0])
        eps = abs(loc)
        return (-0.5 * ((torch.norm(z, dim=1) - loc) / (2 * scale)) ** 2
                - 0.5 * ((a - eps) / (3 * scale)) ** 2
                + torch.log(1 + torch.exp(-2 * a * eps / (3 * scale) ** 2)))
    if family == "smiley":
        scale, = p
        return (-0.5 * ((torch.norm(z, dim=1) - 2) / (2 * scale)) ** 2
                - 0.5 * ((torch.abs(z[:, 1] + 0.8) - 1.2) / (2 * scale)) ** 2)
    a, b, tail = _branches(case, z)
    return a - tail if b is None else torch.logaddexp(a, b) - tail


def naive_log_prob(case, z):
    """The gap and the split with the two-branch log as the reference writes it."""
    a, b, tail = _branches(case, z)
    return torch.log(torch.exp(a) + torch.exp(b)) - tail


def score(case, z):
    """d log p / d z by autograd: torch's gradients of norm and abs are 0 at 0."""
    x = z.detach().clone().requires_grad_(True)
    return torch.autograd.grad(log_prob(case, x).sum(), x)[0]


def closed_form_score(case, z):
    """The scores as include/vcnf_hip.h states them, in plain torch."""
    unit = lambda v, r: torch.where(r > 0, v / torch.where(r > 0, r, torch.ones_like(r)), torch.zeros_like(v))
    family, p = case
    z0, z1 = z[:, 0], z[:, 1]
    r = torch.sqrt(z0 ** 2 + z1 ** 2)
    if family == "two_modes":
        loc, s = p
        a, eps, c1, c2 = z0.abs(), abs(loc), 2 * s, 3 * s
        e = torch.exp(-2 * a * eps / c2 ** 2)
        k = -(r - loc) / c1 ** 2
        return torch.stack([k * unit(z0, r) + torch.sign(z0) * ((eps - a) / c2 ** 2 - (2 * eps / c2 ** 2) * e / (1 + e)),
                            k * unit(z1, r)], 1)
    if family == "smiley":
        c = 2 * p[0]
        t = (z1 + 0.8).abs()
        k = -(r - 2) / c ** 2
        return torch.stack([k * unit(z0, r), k * unit(z1, r) - torch.sign(z1 + 0.8) * (t - 1.2) / c ** 2], 1)
    s, period = p
    q, om = (20 * s) ** 4, 2 * math.pi / period
    d, dw1 = z1 - torch.sin(om * z0), om * torch.cos(om * z0)
    if family == "sinusoidal":
        return torch.stack([d * dw1 / s ** 2 - 2 * z0 ** 3 / q, -d / s ** 2 - 2 * z1 ** 3 / q], 1)
    if family == "gap":
        amp, mu, width = GAP
        w = amp * torch.exp(-0.5 * ((z0 - mu) / width) ** 2)
        dw = -w * (z0 - mu) / width ** 2
    else:
        amp, mu, width = SPLIT
        w = amp * torch.sigmoid((z0 - mu) / width)
        dw = w * (1 - w / amp) / width
    a, b = -0.5 * (d / s) ** 2, -0.5 * ((d + w) / s) ** 2
    pb = torch.sigmoid(b - a)
    pa = 1 - pb
    return torch.stack([(pa * d * dw1 + pb * (d + w) * (dw1 - dw)) / s ** 2 - 2 * z0 ** 3 / q,
                        -(pa * d + pb * (d + w)) / s ** 2 - 2 * z1 ** 3 / q], 1)


def gradients(case, z, g, dtype):
    """(log p [B], score [B, 2], d (g . log p) / d z [B, 2]) of the restatement in ``dtype``."""
    x = z.to(dtype).clone().requires_grad_(True)
    lp = log_prob(case, x)
    grad = torch.autograd.grad((lp * g.to(dtype)).sum(), x)[0]
    return lp.detach(), score(case, z.to(dtype)), grad


@functools.lru_cache(maxsize=None)
def inputs(case, b):
    """(z [b, 2], g [b]) in fp64 by target_ref's recipe: the first min(b, 10) of FIXED_ROWS, then randn * 1.5 for one half
    of the other rows and randn * 3 for the other half, none of them with r < 1e-3.  Shared between tests: do not
    modify."""
    g = torch.Generator().manual_seed(ref.seed_of("energy", case, b))
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
    return torch.cat([fixed, z], 0), torch.randn(b, generator=g, dtype=torch.float64)


def rows(case, b):
    """z [b, 2] of the stochastic tests: the first b rows of the B = 1000 inputs."""
    return inputs(case, 1000)[0][:b]


# ---------------------------------------------------------------- densities of a layer
def prior_log_prob(z):
    """normflow's DiagGaussian.log_prob over (2,) without a temperature, with the parameters LOC, LOG_SCALE."""
    loc, log_scale = torch.tensor(LOC, dtype=z.dtype), torch.tensor(LOG_SCALE, dtype=z.dtype)
    return -0.5 * 2 * math.log(2 * math.pi) - torch.sum(log_scale + 0.5 * torch.pow((z - loc) / torch.exp(log_scale), 2), 1)


def density(case, beta=None, closed=False):
    """(log_prob, score) of a layer as callables of z: the case's own, or with ``beta`` the LinearInterpolation of the case
    and the prior; the score autograd's, or with ``closed`` the closed form of include/vcnf_hip.h."""
    if beta is None:
        lp = lambda z: log_prob(case, z)
    else:
        lp = lambda z: beta * log_prob(case, z) + (1 - beta) * prior_log_prob(z)
    if not closed:
        def sc(z):
            x = z.detach().clone().requires_grad_(True)
            out = lp(x)
            return torch.autograd.grad(out, x, grad_outputs=torch.ones_like(out))[0]
    elif beta is None:
        sc = lambda z: closed_form_score(case, z.detach())
    else:
        def sc(z):
            sig = torch.exp(torch.tensor(LOG_SCALE, dtype=z.dtype))
            u = (z.detach() - torch.tensor(LOC, dtype=z.dtype)) / sig
            return beta * closed_form_score(case, z.detach()) + (1 - beta) * (-u / sig)
    return lp, sc


def densities(case, n_layers, betas=None, closed=False):
    return [density(case, None if betas is None else float(betas[k]), closed) for k in range(n_layers)]


def layer_betas(m=M):
    """The betas of a HAIS chain's layers in their order: betas[m - 1] ... betas[1] of linspace(1, 0, m + 1)."""
    betas = torch.linspace(1, 0, m + 1, dtype=torch.float64)
    return tuple(float(betas[i]) for i in range(m - 1, 0, -1))


# ---------------------------------------------------------------- the stochastic layers
def hmc_parameters(step, n_layers=1):
    """[(log_step_size, log_mass)] in fp64, as stochastic_ref.hmc_parameters makes them."""
    out = []
    for k in range(n_layers):
        ls = torch.tensor([math.log(step), math.log(step) + 0.2], dtype=torch.float64) - 0.1 * k
        lm = torch.tensor([0.1, -0.2], dtype=torch.float64) + 0.15 * k * torch.tensor([1.0, -1.0], dtype=torch.float64)
        out.append((ls, lm))
    return out


def hmc_layer(dens, z, noise, unif, log_step_size, log_mass, steps, accept=None):
    """flows/stochastic.py HamiltonianMonteCarlo.forward with the draws as arguments: (z_out, log_det, accept,
    probabilities).  ``accept``: decisions to impose in place of its own.  The score is detached, as the reference's is."""
    log_p, gradlogP = dens
    p = noise * torch.exp(0.5 * log_mass)
    z_new = z.clone()
    p_new = p.clone()
    step_size = torch.exp(log_step_size)
    for i in range(steps):
        p_half = p_new - (step_size / 2.0) * -gradlogP(z_new)
        z_new = z_new + step_size * (p_half / torch.exp(log_mass))
        p_new = p_half - (step_size / 2.0) * -gradlogP(z_new)
    probabilities = torch.exp(
        log_p(z_new) - log_p(z)
        - 0.5 * torch.sum(p_new ** 2 / torch.exp(log_mass), 1)
        + 0.5 * torch.sum(p ** 2 / torch.exp(log_mass), 1))
    mask = unif < probabilities if accept is None else accept
    z_out = torch.where(mask.unsqueeze(1), z_new, z)
    return z_out, log_p(z) - log_p(z_out), mask, probabilities.detach()


def hmc_run(dens, z, noise, unif, params, steps, accept=None):
    """A run of layers, ``dens`` their densities: (z_out, summed log_det, accept [K, B], probabilities [K, B])."""
    log_det = torch.zeros(len(z), dtype=z.dtype)
    masks, probs = [], []
    for k, (ls, lm) in enumerate(params):
        z, ld, mask, prob = hmc_layer(dens[k], z, noise[k], None if unif is None else unif[k], ls, lm, steps,
                                      None if accept is None else accept[k])
        log_det = log_det + ld
        masks.append(mask)
        probs.append(prob)
    return z, log_det, torch.stack(masks), torch.stack(probs)


def hmc_backward(dens, z, noise, params, steps, accept, gz, gl):
    """The closed form of include/vcnf_hip.h in torch, as stochastic_ref.hmc_closed_form_backward states it:
    (g_z, [(g_log_step_size, g_log_mass)])."""
    entrance = [z]
    for k, (ls, lm) in enumerate(params):
        entrance.append(hmc_layer(dens[k], entrance[-1], noise[k], None, ls, lm, steps, accept[k])[0].detach())
    grads = [None] * len(params)
    for k in range(len(params) - 1, -1, -1):
        ls, lm = params[k]
        sc = dens[k][1]
        step, mass, sqm = torch.exp(ls), torch.exp(lm), torch.exp(0.5 * lm)
        x, a = entrance[k], accept[k].to(z.dtype).unsqueeze(1)
        s = [sc(x)]
        p, halves = noise[k] * sqm, []
        for i in range(steps):
            p_half = p - (step / 2.0) * -s[-1]
            x = x + step * (p_half / mass)
            s.append(sc(x))
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


def mh_walk(case, z, eps, w, scale):
    """flows/stochastic.py MetropolisHastings.forward with a diagonal Gaussian proposal and the draws as arguments:
    (z_out, accept [steps, B], min(exp(.), 1) [steps, B])."""
    log_p = log_prob(case, z)
    masks, ratios = [], []
    for i in range(len(eps)):
        z_ = eps[i] * scale + z
        log_p_ = log_prob(case, z_)
        w_accept = torch.clamp(torch.exp(log_p_ - log_p), max=1)
        accept = w[i] <= w_accept
        z = torch.where(accept.unsqueeze(1), z_, z)
        log_p = torch.where(accept, log_p_, log_p)
        masks.append(accept)
        ratios.append(w_accept)
    return z, torch.stack(masks), torch.stack(ratios)


# ---------------------------------------------------------------- references, computed once
# Salts of the draws' seeds, 0 where not listed, chosen by a property of the restatement alone (test_energy_ref.py
# asserts it for every run), never by what a kernel gives: a row is left out when any of its K decisions is in the band,
# about 1 % of the decisions are, and with salt 0 these small batches have more such rows than few_near allows.
SALTS = {(("smiley", (0.2,)), 65, 4, 3, True): 1}


def hmc_draws(case, b, steps, n_layers, annealed):
    salt = SALTS.get((case, b, steps, n_layers, annealed), 0)
    g = torch.Generator().manual_seed(ref.seed_of("energy-hmc", case, b, steps, n_layers, annealed, salt))
    noise = torch.randn(n_layers, b, 2, generator=g, dtype=torch.float64)
    return noise, torch.rand(n_layers, b, generator=g, dtype=torch.float64)


@functools.lru_cache(maxsize=None)
def hmc_reference(case, steps, step, b, n_layers=1, annealed=False):
    """The restatement of one HMC run like stochastic_ref.hmc_reference: {"z", "noise", "unif", "params", "betas" (None
    for a plain run), dtype: (z_out, log_det, accept, prob), "closed": the fp64 run with the closed-form scores, "band":
    decisions in the band [K, B], "near": rows with one, "yardstick": (z_out, log_det) differences of the two fp64 runs}.
    An annealed run has the M - 1 layers of a HAIS chain.  Shared between tests: do not modify."""
    betas = layer_betas() if annealed else None
    n_layers = len(betas) if annealed else n_layers
    z = rows(case, b)
    noise, unif = hmc_draws(case, b, steps, n_layers, annealed)
    params = hmc_parameters(step, n_layers)
    out = {"z": z, "noise": noise, "unif": unif, "params": params, "betas": betas}
    dens = densities(case, n_layers, betas)
    for dtype in DTYPES:
        out[dtype] = hmc_run(dens, z.to(dtype), noise.to(dtype), unif.to(dtype), [(ls.to(dtype), lm.to(dtype)) for ls, lm in params], steps)
    out["closed"] = hmc_run(densities(case, n_layers, betas, closed=True), z, noise, unif, params, steps)
    out["band"] = (torch.clamp(out[torch.float64][3], max=2.0) - unif).abs() < HMC_BAND
    out["near"] = out["band"].any(0)
    out["yardstick"] = tuple(float((out["closed"][j] - out[torch.float64][j]).abs().max()) for j in (0, 1))
    return out


def hmc_runs(annealed=False):
    """(b, n_layers) of the forward tests: every batch with one layer and B = 1000 with a run; the annealed chain at
    B = 65 and 1000."""
    return [(65, M - 1), (1000, M - 1)] if annealed else [(b, 1) for b in BATCHES] + [(1000, RUN)]


def hmc_band_share(case, steps, step, annealed=False):
    """(share of a case's decisions in the band, share of rejections, fp32 decisions outside the band that differ from
    fp64's), pooled over hmc_runs."""
    near = total = rejected = differ = 0
    for b, k in hmc_runs(annealed):
        r = hmc_reference(case, steps, step, b, k, annealed)
        near, total = near + int(r["band"].sum()), total + r["band"].numel()
        rejected += int((~r[torch.float64][2]).sum())
        differ += int(((r[torch.float32][2] != r[torch.float64][2]) & ~r["band"]).sum())
    return near / total, rejected / total, differ


def few_near(near, decisions_per_row=1):
    """stochastic_ref.few_near: what a single batch must satisfy besides its case's pooled share."""
    b, left_out = len(near), int(near.sum())
    return left_out <= max(2, int(BAND_CAP * b * decisions_per_row)) and left_out < b


@functools.lru_cache(maxsize=None)
def mh_reference(case, steps, scale, b):
    """{"z", "eps", "w", dtype: (z_out, accept, ratio), "near"} of one walk.  Shared between tests: do not modify."""
    z = rows(case, b)
    g = torch.Generator().manual_seed(ref.seed_of("energy-mh", case, b, steps))
    eps = torch.randn(steps, b, 2, generator=g, dtype=torch.float64)
    w = torch.rand(steps, b, generator=g, dtype=torch.float64)
    out = {"z": z, "eps": eps, "w": w}
    with torch.no_grad():
        for dtype in DTYPES:
            out[dtype] = mh_walk(case, z.to(dtype), eps.to(dtype), w.to(dtype), torch.tensor(scale, dtype=dtype))
    out["near"] = ((out[torch.float64][2] - w).abs() < MH_BAND).any(0)
    return out


def mh_band_share(case, steps, scale):
    """Share of a case's rows with any step in the band, pooled over its batches."""
    return sum(int(mh_reference(case, steps, scale, b)["near"].sum()) for b in MH_BATCHES) / sum(MH_BATCHES)


class PlainEnergy:
    """An object with the reference's interface whose log_prob is the restatement's on any device: none of the kernel
    densities.  With ``dtype`` the restatement computes in that dtype whatever z's is and returns z's."""

    def __init__(self, case, dtype=None):
        self.case, self.dtype = case, dtype

    def log_prob(self, z):
        return log_prob(self.case, z if self.dtype is None else z.to(self.dtype)).to(z.dtype)
