"""A run of HamiltonianMonteCarlo layers through csrc/stochastic.hip against the two things a user has without it, on
the same GPU in the same process: the same layers one by one (a launch of the same kernel per layer, what
``fuse_stochastic_stacks = False`` gives a model) and the same modules on their torch path - the reference's composition,
taken because the target is wrapped in a plain ``Target`` subclass whose ``log_prob`` is the kernel target's, so every
score is an ``autograd.grad`` through one launch of csrc/target_density.hip.  Shapes (B, K, steps) = (1024, 1, 5),
(1024, 8, 5), (2048, 32, 10); the three default targets in fp32, and fp64 at the middle shape.  Per variant the eager
forward pass without autograd, and forward + backward of ``log_det.sum() + z.sum()``.  The calls are what a training loop
pays, Python and the draws included.

Timing: the protocol of bench_windows.py, the variants of one (shape, dtype, target) alternated.

    python profiles/tools/stochastic_bench.py [--shapes 1024x1x5,1024x8x5,2048x32x10] [--window 0.15] [--reps 5] [--out FILE]
"""
import math

import torch

import bench_windows as bw         # first: it puts the repository root and tests/ on sys.path
import vcnf_amd as nf
from vcnf_amd import fused_stochastic

TARGETS = {"TwoMoons": lambda: nf.distributions.TwoMoons(), "CircularGaussianMixture": lambda: nf.distributions.CircularGaussianMixture(),
           "RingMixture": lambda: nf.distributions.RingMixture()}
STEP = 0.05


class Wrapped(nf.distributions.Target):
    """The kernel target behind a plain Target: the layers take their torch composition."""

    def __init__(self, inner):
        super().__init__()
        self.inner = inner
        self.n_dims = 2

    def log_prob(self, z):
        return self.inner.log_prob(z)


def _layers(target, k, steps, dtype):
    out = []
    for i in range(k):
        ls = torch.tensor([math.log(STEP), math.log(STEP) + 0.2]) - 0.01 * i
        lm = torch.tensor([0.1, -0.2])
        out.append(nf.flows.HamiltonianMonteCarlo(target, steps, ls, lm))
    return torch.nn.ModuleList(out).to(dtype).cuda()


def _variants(b, k, steps, name, dtype):
    """variant -> call(i)"""
    target = TARGETS[name]().to(dtype).cuda()
    kernel, torch_path = _layers(target, k, steps, dtype), _layers(Wrapped(target), k, steps, dtype)
    assert fused_stochastic.covers(kernel[0], torch.zeros(1, 2, dtype=dtype, device="cuda"))
    assert not fused_stochastic.covers(torch_path[0], torch.zeros(1, 2, dtype=dtype, device="cuda"))
    z0 = (1.5 * torch.randn(b, 2, dtype=dtype, device="cuda"))

    def one_launch(z):
        return fused_stochastic.run(list(kernel), z, None, 1.0)

    def one_by_one(layers):
        def walk(z):
            log_det = torch.zeros(len(z), dtype=z.dtype, device=z.device)
            for layer in layers:
                z, ld = layer(z)
                log_det = log_det + ld
            return z, log_det
        return walk

    def forward(walk):
        def call(i):
            with torch.no_grad():
                walk(z0)
        return call

    def both(walk, layers):
        def call(i):
            layers.zero_grad(set_to_none=True)
            z, log_det = walk(z0.clone().requires_grad_(True))
            (log_det.sum() + z.sum()).backward()
        return call

    return {"forward, one launch per run": forward(one_launch),
            "forward, one launch per layer": forward(one_by_one(kernel)),
            "forward, torch path": forward(one_by_one(torch_path)),
            "forward + backward, one launch per run": both(one_launch, kernel),
            "forward + backward, one launch per layer": both(one_by_one(kernel), kernel),
            "forward + backward, torch path": both(one_by_one(torch_path), torch_path)}


def run(shapes, window, reps, out):
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    lines = ["| B | K | steps | dtype | target | variant | us per call | spread | x the run |", "|---|---|---|---|---|---|---|---|---|"]
    torch.manual_seed(17)
    middle = shapes[len(shapes) // 2]
    for b, k, steps in shapes:
        for dtype in (torch.float32, torch.float64):
            if dtype == torch.float64 and (b, k, steps) != middle:
                continue
            for name in TARGETS:
                variants = _variants(b, k, steps, name, dtype)
                results, failed = bw.measure(variants, window, reps)
                for v in variants:
                    lead = "| %d | %d | %d | %s | %s | %s |" % (b, k, steps, bw.dtype_name(dtype), name, v)
                    base = results.get(v.split(",")[0] + ", one launch per run")
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
    ap.add_argument("--shapes", default="1024x1x5,1024x8x5,2048x32x10")
    a = ap.parse_args()
    run([tuple(int(v) for v in s.split("x")) for s in a.shapes.split(",")], a.window, a.reps, a.out)
