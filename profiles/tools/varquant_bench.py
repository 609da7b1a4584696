"""Dequantisation of categorical columns against what a user has without the kernels, on the same GPU in the same process:
the plain-torch restatement of the formulas (tests/varquant_ref.py) run on the same device tensors.  There is no parent
implementation to compare with.  Rows (B, D, C) = (2048, 14, 8) with the Adult levels in fp64 and fp32, and
(1048576, 14, 8) in fp32:

* ``Dequantization.dequantize`` (uniform; the draw included in both variants);
* ``VariationalDequantization.dequantize`` without flows (the two end caps) and with a run of four
  [MaskedAffineFlow, ActNorm] pairs over the 8 noise columns; the restatement runs the same flows between its end caps;
* the merge VJP: the node's forward and backward against the restatement's forward and autograd backward, and the VJP
  launch alone;
* ``quantize``;
* a ``forward_kld`` + ``backward`` step of a masked-stack model (eight [MaskedAffineFlow, ActNorm] pairs, D = 14, H = 28)
  with categorical columns on the kernels, with the dequantiser's torch composition in their place, and without
  categorical columns (continuous rows).

Everything is eager, Python and the draw included.  Timing: the protocol of bench_windows.py, the variants of one group
alternated.

    python profiles/tools/varquant_bench.py [--window 0.2] [--reps 5] [--out FILE]
"""
import copy

import torch

import bench_windows as bw         # first: it puts the repository root and tests/ on sys.path
import varquant_ref as ref
import vcnf_amd as nf
from vcnf_amd import _lib, autograd

COLUMNS, LEVELS = ref.ADULT
ALPHA = 1e-5


def _pairs(d, h, pairs):
    mask = torch.tensor([1.0 if i % 2 == 0 else 0.0 for i in range(d)])
    flows = []
    for i in range(pairs):
        s, t = nf.nets.MLP([d, h, d], init_zeros=True), nf.nets.MLP([d, h, d], init_zeros=True)
        flows += [nf.flows.MaskedAffineFlow(mask if i % 2 == 0 else 1 - mask, t, s), nf.flows.ActNorm(d)]
    return flows


def _restated_variational(vdq, x, u):
    v, ctx, ld = ref.prepare(x, COLUMNS, LEVELS, u, ALPHA)
    for flow in vdq.flows:
        v, part = flow(v)
        ld = ld + part
    out, part = ref.merge(x, COLUMNS, LEVELS, v, True, ALPHA)
    return out, ld + part


def _call_groups(b, dtype):
    """group name -> {variant: call} of the dequantiser's calls, under no_grad unless the call says otherwise"""
    c = len(COLUMNS)
    x = ref.rows(b, 14, COLUMNS, LEVELS, 1, dtype, "cuda")
    w = 4 * torch.randn(b, c, dtype=dtype, device="cuda")
    g_out, g_ld = torch.randn_like(x), torch.randn(b, dtype=dtype, device="cuda")
    slot, lv = _lib.column_tables(COLUMNS, LEVELS, 14, x.device)
    uniform, caps = nf.nets.Dequantization(ALPHA), nf.nets.VariationalDequantization([], ALPHA)
    torch.manual_seed(23)
    learned = nf.nets.VariationalDequantization(_pairs(c, 16, 4), ALPHA).to("cuda", dtype)
    draw = lambda: torch.rand(b, c, dtype=dtype, device="cuda")
    with torch.no_grad():
        learned.dequantize(x, COLUMNS, LEVELS)           # the ActNorms take their statistics from this batch
        z = uniform.dequantize(x, COLUMNS, LEVELS)[0]

    def node(i):
        leaf = w.clone().requires_grad_()
        out, ld = autograd.DequantMergeFn.apply(x, leaf, slot, lv, True, ALPHA)
        torch.autograd.backward((out, ld), (g_out, g_ld))

    def restated_node(i):
        leaf = w.clone().requires_grad_()
        out, ld = ref.merge(x, COLUMNS, LEVELS, leaf, True, ALPHA)
        torch.autograd.backward((out, ld), (g_out, g_ld))

    def quiet(call):
        def run(i):
            with torch.no_grad():
                call()
        return run

    return {
        "dequantize, uniform": {"kernel": quiet(lambda: uniform.dequantize(x, COLUMNS, LEVELS)),
                                "torch restatement": quiet(lambda: ref.merge(x, COLUMNS, LEVELS, draw(), False, ALPHA))},
        "dequantize, variational, no flows": {"kernel": quiet(lambda: caps.dequantize(x, COLUMNS, LEVELS)),
                                              "torch restatement": quiet(lambda: _restated_variational(caps, x, draw()))},
        "dequantize, variational, 4 masked pairs": {"kernel": quiet(lambda: learned.dequantize(x, COLUMNS, LEVELS)),
                                                    "torch restatement": quiet(lambda: _restated_variational(learned, x, draw()))},
        "merge forward + VJP": {"kernel": node, "torch restatement": restated_node,
                                "kernel, the VJP launch alone": quiet(lambda: _lib.dequant_merge_bwd(x, slot, lv, w, True, ALPHA, g_out, g_ld))},
        "quantize": {"kernel": quiet(lambda: uniform.quantize(z, COLUMNS, LEVELS)),
                     "torch restatement": quiet(lambda: ref.quantize(z, COLUMNS, LEVELS, ALPHA))},
    }


def _step_group(b, dtype):
    torch.manual_seed(29)
    flows = _pairs(14, 28, 8)
    q0 = nf.distributions.DiagGaussian(14)
    vdq = nf.nets.VariationalDequantization(_pairs(len(COLUMNS), 16, 4), ALPHA)
    mine = nf.NormalizingFlow(q0, flows, categoricals=COLUMNS, catlevels=LEVELS, catvdeqs=vdq).to("cuda", dtype)
    x = ref.rows(b, 14, COLUMNS, LEVELS, 2, dtype, "cuda")
    with torch.no_grad():
        xt = mine.dequantize(x)[0]
        mine.log_prob(x)                                  # the ActNorms take their statistics from this batch
    twin = copy.deepcopy(mine)
    twin.catvdeqs.use_kernels = False
    plain = nf.NormalizingFlow(copy.deepcopy(q0), copy.deepcopy(flows)).to("cuda", dtype)

    def step(model, rows):
        def run(i):
            model.zero_grad(set_to_none=True)
            model.forward_kld(rows).backward()
        return run
    return {"forward_kld + backward, masked stack": {"kernel": step(mine, x), "torch composition": step(twin, x),
                                                     "no categorical columns": step(plain, xt)}}


def run(window, reps, out):
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    lines = ["| B | dtype | call | variant | us per call | spread | x the kernel path |", "|---|---|---|---|---|---|---|"]
    torch.manual_seed(17)
    for b, dtype in ((2048, torch.float64), (2048, torch.float32), (1048576, torch.float32)):
        groups = dict(_call_groups(b, dtype), **_step_group(b, dtype))
        for group, variants in groups.items():
            results, failed = bw.measure(variants, window, reps)
            base = results.get("kernel")
            for name in variants:
                lead = "| %d | %s | %s | %s |" % (b, bw.dtype_name(dtype), group, name)
                if name in failed:
                    lines.append("%s failed: %s | | |" % (lead, failed[name]))
                else:
                    med, spread, _ = results[name]
                    lines.append("%s %.1f | %.3f | %s |" % (lead, med * 1e6, spread, "%.2f" % (med / base.median) if base else ""))
                print(lines[-1], flush=True)
        del groups
        torch.cuda.empty_cache()
    return bw.finish(lines, window, reps, out)


if __name__ == "__main__":
    a = bw.parser(0.2).parse_args()
    run(a.window, a.reps, a.out)
