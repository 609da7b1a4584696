"""The flow VAE of the reference's example/vae.py, forward + backward, with and without the kernels of this package on
its way: encoder 784 -> 512 -> 256 -> 2 d (d = 40, ReLU), K = 10 Planar layers, Bernoulli decoder d -> 256 -> 512 -> 784,
DiagGaussian prior; loss = mean(log_q) - mean(log_p).  Variants, on the same GPU in the same process with the same
weights: "kernels" (fuse=True on both ends, fuse_planar_stacks = True) and "torch ends, layer by layer" (fuse=False on
both ends, fuse_planar_stacks = False).  The calls are what a training loop pays, Python and the dense layers included.

Timing: the protocol of bench_windows.py, the two variants of a (B, S, dtype) alternated.

    python profiles/tools/vae_bench.py [--shapes 256x1,64x16,4096x1] [--window 0.3] [--reps 5] [--out FILE]
    python profiles/tools/vae_bench.py --trace     # five steps per shape of the kernel variant, for a kernel trace
"""
import torch
from torch import nn

import bench_windows as bw         # first: it puts the repository root and tests/ on sys.path
import vcnf_amd as nf

LATENT, LAYERS = 40, 10


def model(dtype, fuse):
    torch.manual_seed(0)
    D = nf.distributions
    enc = nn.Sequential(nn.Linear(784, 512), nn.ReLU(True), nn.Linear(512, 256), nn.ReLU(True), nn.Linear(256, 2 * LATENT))
    dec = nn.Sequential(nn.Linear(LATENT, 256), nn.ReLU(True), nn.Linear(256, 512), nn.ReLU(True), nn.Linear(512, 784))
    flows = [nf.flows.Planar((LATENT,)) for _ in range(LAYERS)]
    m = nf.NormalizingFlowVAE(D.DiagGaussian(LATENT, trainable=False), D.NNDiagGaussian(enc, fuse=fuse), flows,
                              D.NNBernoulliDecoder(dec, fuse=fuse))
    m.fuse_planar_stacks = fuse
    return m.to(dtype).cuda()


def step(m, x, s):
    def call(i):
        m.zero_grad(set_to_none=True)
        _, log_q, log_p = m(x, num_samples=s)
        (torch.mean(log_q) - torch.mean(log_p)).backward()
    return call


def data(b, dtype):
    return torch.rand(b, 784, generator=torch.Generator().manual_seed(1)).round().to(dtype).cuda()


def run(shapes, window, reps, out):
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    lines = ["| B | S | dtype | variant | us per step | spread | x kernels |", "|---|---|---|---|---|---|---|"]
    for b, s in shapes:
        for dtype in (torch.float32, torch.float64):
            x = data(b, dtype)
            variants = {"kernels": step(model(dtype, True), x, s), "torch ends, layer by layer": step(model(dtype, False), x, s)}
            results, failed = bw.measure(variants, window, reps)
            for name in variants:
                lead = "| %d | %d | %s | %s |" % (b, s, bw.dtype_name(dtype), name)
                base = results.get("kernels")
                if name in failed:
                    lines.append("%s failed: %s | | |" % (lead, failed[name]))
                else:
                    med, spread, _ = results[name]
                    lines.append("%s %.1f | %.3f | %s |" % (lead, med * 1e6, spread, "%.2f" % (med / base.median) if base else ""))
                print(lines[-1], flush=True)
            del variants
            torch.cuda.empty_cache()
    return bw.finish(lines, window, reps, out)


def trace(shapes):
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    for b, s in shapes:
        call = step(model(torch.float32, True), data(b, torch.float32), s)
        for i in range(5):
            call(i)
    torch.cuda.synchronize()


if __name__ == "__main__":
    ap = bw.parser(0.3)
    ap.add_argument("--shapes", default="256x1,64x16,4096x1")
    ap.add_argument("--trace", action="store_true")
    a = ap.parse_args()
    shapes = [tuple(int(v) for v in s.split("x")) for s in a.shapes.split(",")]
    trace(shapes) if a.trace else run(shapes, a.window, a.reps, a.out)
