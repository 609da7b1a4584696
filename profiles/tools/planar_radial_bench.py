"""A run of Planar / Radial layers against the two things a user has without it, on the same GPU in the same process: the
model with ``fuse_planar_stacks = False`` (one launch of the same kernel per layer, the operands built per layer) and the
plain-torch restatement of the same arithmetic (tests/planar_radial_ref.py, run on the device tensors).  Shapes
(B, D, K) = (1024, 2, 32) and (2048, 16, 64), fp32 and fp64, all-tanh Planar and all-Radial stacks; per variant
``sample_from`` without autograd and the reverse KL divergence against a fixed DiagGaussian target, forward plus backward
(the model's ``reverse_kld``; the restatement's loss at a draw of its own).  The calls are what a training loop pays,
Python included.

Timing: the protocol of bench_windows.py, the variants of one (shape, dtype, stack) alternated.

    python profiles/tools/planar_radial_bench.py [--shapes 1024x2x32,2048x16x64] [--window 0.2] [--reps 5] [--out FILE]
"""
import torch

import bench_windows as bw         # first: it puts the repository root and tests/ on sys.path
import planar_radial_ref as ref
import vcnf_amd as nf


def _model(layers, d, dtype):
    flows = []
    for p in layers:
        if p["kind"] == "radial":
            f = nf.flows.Radial(d, z_0=p["z_0"].to(dtype))
            f.alpha.data, f.beta.data = p["alpha"].to(dtype), p["beta"].to(dtype)
        else:
            f = nf.flows.Planar(d, act=p["kind"], u=p["u"].to(dtype), w=p["w"].to(dtype), b=p["b"].to(dtype))
        flows.append(f)
    target = nf.distributions.DiagGaussian(d, trainable=False)
    target.log_scale.fill_(0.3)
    return nf.NormalizingFlow(nf.distributions.DiagGaussian(d), flows, p=target).to(dtype).cuda()


def _variants(b, d, k, stack, dtype):
    """name -> call(i)"""
    layers, eps, _, _ = ref.inputs(stack, d, k, b)
    model = _model(layers, d, dtype)
    eps = eps.to(dtype).cuda()
    dev = ref.cast(layers, dtype, "cuda")
    leaves = ref.leaves(dev)
    params = [v for p in leaves for v in p.values() if torch.is_tensor(v)]
    loc, ls = model.p.loc.detach(), model.p.log_scale.detach()

    def sample_from(fused):
        def call(i):
            model.fuse_planar_stacks = fused
            with torch.no_grad():
                model.sample_from(eps)
        return call

    def reverse_kld(fused):
        def call(i):
            model.fuse_planar_stacks = fused
            model.zero_grad(set_to_none=True)
            model.reverse_kld(b).backward()
        return call

    def eager_sample_from(i):
        with torch.no_grad():
            ref.sample_from(eps, dev)

    def eager_reverse_kld(i):
        z, lq = ref.sample_from(torch.randn(b, d, device="cuda", dtype=dtype), leaves)
        loss = lq.mean() - ref.gaussian_log_prob(z, loc, ls).mean()
        torch.autograd.grad(loss, params)

    return {"sample_from, one launch per run": sample_from(True),
            "sample_from, fuse_planar_stacks = False": sample_from(False),
            "sample_from, torch restatement": eager_sample_from,
            "reverse_kld forward + backward, one launch per run": reverse_kld(True),
            "reverse_kld forward + backward, fuse_planar_stacks = False": reverse_kld(False),
            "reverse_kld forward + backward, torch restatement": eager_reverse_kld}


def run(shapes, window, reps, out):
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    lines = ["| B | D | K | dtype | stack | variant | us per call | spread | x the run |", "|---|---|---|---|---|---|---|---|---|"]
    torch.manual_seed(17)
    for b, d, k in shapes:
        for dtype in (torch.float32, torch.float64):
            for stack in ("tanh", "radial"):
                variants = _variants(b, d, k, stack, dtype)
                results, failed = bw.measure(variants, window, reps)
                for name in variants:
                    lead = "| %d | %d | %d | %s | %s | %s |" % (b, d, k, bw.dtype_name(dtype), stack, name)
                    base = results.get([n for n in variants if n.split(",")[0].lower() == name.split(",")[0].lower()][0])
                    if name in failed:
                        lines.append("%s failed: %s | | |" % (lead, failed[name]))
                    else:
                        med, spread, _ = results[name]
                        lines.append("%s %.1f | %.3f | %s |" % (lead, med * 1e6, spread, "%.2f" % (med / base.median) if base else ""))
                    print(lines[-1], flush=True)
                del variants
                torch.cuda.empty_cache()
    return bw.finish(lines, window, reps, out)


if __name__ == "__main__":
    ap = bw.parser(0.2)
    ap.add_argument("--shapes", default="1024x2x32,2048x16x64")
    a = ap.parse_args()
    run([tuple(int(v) for v in s.split("x")) for s in a.shapes.split(",")], a.window, a.reps, a.out)
