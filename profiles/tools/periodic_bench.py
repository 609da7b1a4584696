"""The circular layers and their base against what a user has without them, on the same GPU in the same process: the
plain-torch restatement of normflow 1.2's periodic.py and UniformGaussian (tests/periodic_ref.py, run on the device
tensors).  Per dtype:

* ``PeriodicShift.forward`` and ``UniformGaussian.log_prob`` / ``forward`` at (B, D) = (1024, 3) with one circular column
  and (1048576, 64) with 32 (every other column);
* ``log_prob`` of the reference's circular spline model (four circular couplings with a PeriodicShift each, a
  PeriodicWrap, UniformGaussian base; D = 3) at 1024 samples, built with the package's classes and, over the same
  couplings, with the restatement's;
* the bare library calls ``_lib.periodic`` and ``_lib.uniform_gaussian_log_prob`` into preallocated outputs at the large
  shape: one launch and no allocation, so at that size the time per call is the kernel's to within a launch overhead.
  Its bytes (every element read once and written once; read once for the density) over that time are given as a share
  of the 8 TB/s peak.

Everything is eager, Python included, under no_grad.  Timing: the protocol of bench_windows.py, the variants of one
group alternated.

    python profiles/tools/periodic_bench.py [--window 0.2] [--reps 5] [--out FILE]
"""
import math

import torch

import bench_windows as bw         # first: it puts the repository root and tests/ on sys.path
import periodic_ref as ref
import vcnf_amd as nf
from vcnf_amd import _lib


def _layer_groups(b, d, dtype):
    """group name -> ({variant: call}, bytes the bare call moves or None)"""
    ind = [1] if d == 3 else list(range(0, d, 2))
    size = torch.empty((), dtype=dtype).element_size()
    z = (3 * math.pi * torch.randn(b, d, device="cuda", dtype=torch.float64)).to(dtype)
    scale = torch.ones(d)
    scale[ind] = 2 * math.pi
    mine_s, ref_s = nf.flows.PeriodicShift(ind, math.pi, 0.5), ref.PeriodicShift(ind, math.pi, 0.5)
    mine_q = nf.distributions.UniformGaussian(d, ind, scale).to(dtype).cuda()
    ref_q = ref.UniformGaussian(d, ind, scale).to(dtype).cuda()
    groups = {
        "PeriodicShift.forward": ({"kernel": lambda i: mine_s.forward(z), "torch restatement": lambda i: ref_s.forward(z)}, None),
        "UniformGaussian.log_prob": ({"kernel": lambda i: mine_q.log_prob(z), "torch restatement": lambda i: ref_q.log_prob(z)}, None),
        "UniformGaussian.forward": ({"kernel": lambda i: mine_q.forward(b), "torch restatement": lambda i: ref_q.forward(b)}, None),
    }
    if b * d >= 1 << 24:
        half, shift = mine_s._tables(z)
        out, logp = torch.empty_like(z), torch.zeros(b, device="cuda", dtype=dtype)
        inv, _, _, _, const_term = mine_q._tables()
        groups["bare vcnf_periodic"] = ({"kernel": lambda i: _lib.periodic(z, half, shift, 1.0, out=out)}, 2 * b * d * size)
        groups["bare vcnf_uniform_gaussian_log_prob"] = (
            {"kernel": lambda i: _lib.uniform_gaussian_log_prob(z, inv, const_term, logp=logp)}, (b * d + 2 * b) * size)
    return groups


def _model_group(b, dtype):
    torch.manual_seed(21)
    bound = torch.tensor([2.5, math.pi, 2.5])
    scale = torch.tensor([5.0, 2 * math.pi, 5.0])
    mine, twin = [], []
    for i in range(4):
        c = nf.flows.CircularCoupledRationalQuadraticSpline(3, 1, 16, [1], num_bins=4, tail_bound=bound, reverse_mask=i % 2,
                                                            init_identity=False)
        mine += [c, nf.flows.PeriodicShift([1], math.pi, 0.5 + i)]
        twin += [c, ref.PeriodicShift([1], math.pi, 0.5 + i)]
    model = nf.NormalizingFlow(nf.distributions.UniformGaussian(3, [1], scale), mine + [nf.flows.PeriodicWrap([1], math.pi)])
    other = nf.NormalizingFlow(ref.UniformGaussian(3, [1], scale), twin + [ref.PeriodicWrap([1], math.pi)])
    model, other = model.to(dtype).cuda().eval(), other.to(dtype).cuda().eval()
    x = torch.stack([1.5 * torch.randn(b), math.pi * (2 * torch.rand(b) - 1), 1.5 * torch.randn(b)], 1).to(dtype).cuda()
    return {"circular spline model log_prob": ({"kernel": lambda i: model.log_prob(x),
                                                "torch restatement": lambda i: other.log_prob(x)}, None)}


def run(window, reps, out):
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    lines = ["| B | D | dtype | call | variant | us per call | spread | x the kernel path | share of 8 TB/s |", "|---|---|---|---|---|---|---|---|---|"]
    torch.manual_seed(17)
    with torch.no_grad():
        for dtype in (torch.float32, torch.float64):
            for b, d in ((1024, 3), (1 << 20, 64), (1024, 0)):
                groups = _layer_groups(b, d, dtype) if d else _model_group(b, dtype)
                for group, (variants, nbytes) in groups.items():
                    results, failed = bw.measure(variants, window, reps)
                    for name in variants:
                        lead = "| %d | %d | %s | %s | %s |" % (b, d or 3, bw.dtype_name(dtype), group, name)
                        base = results.get("kernel")
                        if name in failed:
                            lines.append("%s failed: %s | | | |" % (lead, failed[name]))
                        else:
                            med, spread, _ = results[name]
                            lines.append("%s %.1f | %.3f | %s | %s |" % (
                                lead, med * 1e6, spread, "%.2f" % (med / base.median) if base else "",
                                "%.1f %%" % (100 * nbytes / med / bw.HBM_PEAK) if nbytes else ""))
                        print(lines[-1], flush=True)
                del groups
                torch.cuda.empty_cache()
    return bw.finish(lines, window, reps, out)


if __name__ == "__main__":
    a = bw.parser(0.2).parse_args()
    run(a.window, a.reps, a.out)
