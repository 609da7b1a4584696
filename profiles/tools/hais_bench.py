"""``nf.sampling.HAIS.sample`` through the annealed kernels of csrc/stochastic.hip against the two things a user has
without them, on the same GPU in the same process: the same sampler with ``fuse=False`` (a launch of the same kernel per
layer, and one of csrc/target_density.hip for the last term) and the torch composition - the same chain over
``stochastic_ref.plain_target``, a Target subclass in plain torch that the kernel does not cover, so every score is an
``autograd.grad`` through two ``log_prob``s.  Shapes (N, M) = (1024, 10), (1024, 100), (16384, 20) with 5 leapfrog steps
(M - 1 layers each), fp32 and fp64, eager, Python and the draws included.  Also forward + backward of one
``reverse_kld`` step of a NormalizingFlow whose flows are the chain's layers (the run is one autograd node), against the
same model with ``fuse_stochastic_stacks = False`` and on the torch composition.

Timing: the protocol of bench_windows.py, the variants of one (shape, dtype, target) alternated.

    python profiles/tools/hais_bench.py [--shapes 1024x10,1024x100,16384x20] [--targets two_moons] [--window 0.15] [--reps 5] [--out FILE]
"""
import torch

import bench_windows as bw         # first: it puts the repository root and tests/ on sys.path
import stochastic_ref as sref
import vcnf_amd as nf
from vcnf_amd import fused_stochastic

TARGETS = {"two_moons": (lambda: nf.distributions.TwoMoons(), 0), "circular": (lambda: nf.distributions.CircularGaussianMixture(8), 8),
           "ring": (lambda: nf.distributions.RingMixture(2), 2)}
STEPS, STEP = 5, 0.05


def _prior(dtype):
    return nf.distributions.DiagGaussian(2, trainable=False).to(dtype).cuda()


def _sampler(target, dtype, m, fuse):
    betas = torch.linspace(1, 0, m + 1, dtype=dtype)
    step_size = torch.tensor([STEP, 1.2 * STEP], dtype=dtype, device="cuda")
    log_mass = torch.tensor([0.1, -0.2], dtype=dtype, device="cuda")
    return nf.sampling.HAIS(betas, _prior(dtype), target, STEPS, step_size, log_mass, fuse=fuse)


def _model(sampler, fuse):
    model = nf.NormalizingFlow(sampler.prior, sampler.layers, p=sampler.target)
    model.fuse_stochastic_stacks = fuse
    return model


def _variants(num, m, name, dtype):
    """variant -> call(i)"""
    make, n = TARGETS[name]
    kernel = make().to(dtype).cuda()
    plain = sref.plain_target(name, n).cuda()
    probe = torch.zeros(1, 2, dtype=dtype, device="cuda")
    samplers = {"one launch per chain": _sampler(kernel, dtype, m, True), "one launch per layer": _sampler(kernel, dtype, m, False),
                "torch composition": _sampler(plain, dtype, m, True)}
    with torch.no_grad():
        assert fused_stochastic.covers(samplers["one launch per chain"].layers[0], probe)
        assert not fused_stochastic.covers(samplers["torch composition"].layers[0], probe)
    models = {v: _model(s, v == "one launch per chain") for v, s in samplers.items()}

    def sample(sampler):
        def call(i):
            with torch.no_grad():
                sampler.sample(num)
        return call

    def train(model):
        def call(i):
            model.zero_grad(set_to_none=True)
            model.reverse_kld(num).backward()
        return call

    out = {"HAIS.sample, " + v: sample(s) for v, s in samplers.items()}
    out.update({"reverse_kld forward + backward, " + v: train(mod) for v, mod in models.items()})
    return out


def run(shapes, targets, window, reps, out):
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    lines = ["| N | M | dtype | target | variant | us per call | spread | x one launch per chain |", "|---|---|---|---|---|---|---|---|"]
    torch.manual_seed(17)
    for num, m in shapes:
        for dtype in (torch.float32, torch.float64):
            for name in targets:
                variants = _variants(num, m, name, dtype)
                results, failed = bw.measure(variants, window, reps)
                for v in variants:
                    lead = "| %d | %d | %s | %s | %s |" % (num, m, bw.dtype_name(dtype), name, v)
                    base = results.get(v.split(",")[0] + ", one launch per chain")
                    if v in failed:
                        lines.append("%s failed: %s | | |" % (lead, failed[v]))
                    else:
                        med, spread, _ = results[v]
                        lines.append("%s %.1f | %.3f | %s |" % (lead, med * 1e6, spread, "%.2f" % (med / base.median) if base else ""))
                    print(lines[-1], flush=True)
                del variants
                torch.cuda.empty_cache()
    return bw.finish(lines, window, reps, out)


if __name__ == "__main__":
    ap = bw.parser(0.15)
    ap.add_argument("--shapes", default="1024x10,1024x100,16384x20")
    ap.add_argument("--targets", default="two_moons")
    a = ap.parse_args()
    run([tuple(int(v) for v in s.split("x")) for s in a.shapes.split(",")], a.targets.split(","), a.window, a.reps, a.out)
