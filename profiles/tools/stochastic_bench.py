"""A run of HamiltonianMonteCarlo layers through csrc/stochastic.hip against the two things a user has without it, on
the same GPU in the same process: the same layers one by one (a launch of the same kernel per layer, what
``fuse_stochastic_stacks = False`` gives a model) and the same modules on their torch path - the reference's composition,
taken because the target is wrapped in a plain ``Target`` subclass whose ``log_prob`` is the kernel target's, so every
score is an ``autograd.grad`` through one launch of csrc/target_density.hip.  Shapes (B, K, steps) = (1024, 1, 5),
(1024, 8, 5), (2048, 32, 10); the three default targets in fp32, and fp64 at the middle shape.  Per variant the eager
forward pass without autograd, and forward + backward of ``log_det.sum() + z.sum()``.  The calls are what a training loop
pays, Python and the draws included.

Timing: a window is `calls` back-to-back calls between two device events, sized by a calibration pass so that it lasts
at least --window seconds; time per call = window / calls (launches included).  After warm-up the variants of one
(shape, dtype, target) are alternated for --reps windows each; the table gives the median and the spread (max - min) /
median.

    python profiles/tools/stochastic_bench.py [--shapes 1024x1x5,1024x8x5,2048x32x10] [--window 0.15] [--reps 5] [--out FILE]
"""
import argparse
import math
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT]
import vcnf_amd as nf  # noqa: E402
from vcnf_amd import fused_stochastic  # noqa: E402

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


def _window(call, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(calls):
        call(i)
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e-3 / calls          # seconds per call


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
                calls, times = {}, {}
                for v, call in variants.items():                # warm-up, then size the window
                    _window(call, 2)
                    t = _window(call, 3)
                    calls[v] = max(2, int(window / t) + 1)
                    times[v] = []
                for _ in range(reps):
                    for v, call in variants.items():
                        times[v].append(_window(call, calls[v]))
                med = {v: statistics.median(times[v]) for v in variants}
                for v in variants:
                    base = med[v.split(",")[0] + ", one launch per run"]
                    spread = (max(times[v]) - min(times[v])) / med[v]
                    lines.append("| %d | %d | %d | %s | %s | %s | %.1f | %.3f | %.2f |" % (
                        b, k, steps, "fp64" if dtype == torch.float64 else "fp32", name, v, med[v] * 1e6, spread, med[v] / base))
                    print(lines[-1], flush=True)
                del variants
                torch.cuda.empty_cache()
    text = "windows of >= %.2f s, %d alternated windows per variant\n\n%s\n" % (window, reps, "\n".join(lines))
    if out:
        with open(out, "w") as f:
            f.write(text)
    return text


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="1024x1x5,1024x8x5,2048x32x10")
    ap.add_argument("--window", type=float, default=0.15)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    run([tuple(int(v) for v in s.split("x")) for s in a.shapes.split(",")], a.window, a.reps, a.out)
