"""The sampling direction of the autoregressive flows: the one-launch kernel (csrc/made_sample.hip) against the same layer
with ``fuse_sampling = False``, which is the loop of D MADE passes - the code path of the commit before the kernel - on
the same GPU in the same process.  Per (B, D, H, blocks), fp32 and fp64: ``AutoregressiveRationalQuadraticSpline.forward``
(8 bins, linear tails) and ``MaskedAffineAutoregressive.inverse``, each as the layer call a user makes (packing lookup,
allocation and Python included) and as the bare ``_lib.made_sample`` call on the packed operands, whose time per call at
the large shapes is the kernel's own.  ``--model`` adds ``sample(2048)`` of a 16-layer model (spline layer + Permute, 16
times) with the first shape's D, H and blocks.  ``--launches`` counts the device kernels of one call of each variant with torch's profiler
instead of timing.

Timing: the protocol of bench_windows.py, the variants of one (shape, dtype, layer) alternated.

    python profiles/tools/ar_sampling_bench.py [--shapes 1024x2x128x2,...] [--model] [--launches] [--window 0.2] [--reps 5] [--out FILE]
"""
import torch

import bench_windows as bw         # first: it puts the repository root and tests/ on sys.path
import made_sample_ref as ref
import vcnf_amd as nf
from vcnf_amd import _lib, made_sample

SHAPES = "1024x2x128x2,2048x16x128x2,65536x16x128x2,2048x64x256x2"
MODEL_BATCH = 2048


def _layer(kind, d, h, nb, dtype):
    if kind == "spline":
        lay = nf.flows.AutoregressiveRationalQuadraticSpline(d, nb, h, num_bins=8, tail_bound=3.0, init_identity=False)
        inner = lay.mprqat
    else:
        lay = inner = nf.flows.MaskedAffineAutoregressive(d, h, num_blocks=nb)
    ref.redraw(inner.autoregressive_net)
    return lay.to(dtype).cuda().eval(), inner


def _variants(b, d, h, nb, kind, dtype):
    """name -> call(i)"""
    lay, inner = _layer(kind, d, h, nb, dtype)
    x = (1.5 * torch.randn(b, d)).to(dtype).cuda()
    entry = lay.forward if kind == "spline" else lay.inverse
    with torch.no_grad():
        packed = made_sample.plan(inner, x, None, inner._output_dim_multiplier())
    cfg = inner._spline_cfg() if kind == "spline" else None
    p = inner._output_dim_multiplier()

    def layer_call(fused):
        def call(i):
            inner.fuse_sampling = fused
            with torch.no_grad():
                entry(x)
        return call

    def bare(i):
        _lib.made_sample(x, packed[0], packed[1], None, None, h, nb, p, cfg)

    loop = {"fuse_sampling = False (the loop, the parent's path)": layer_call(False)}
    if packed is None:                 # a shape vcnf_amd.made_sample.plan sends to the loop: only the loop is timed
        return loop
    return {"one launch": layer_call(True), **loop, "bare _lib.made_sample": bare}


def _model_variants(b, d, h, nb, dtype, layers=16):
    flows = []
    for _ in range(layers):
        flows += [_layer("spline", d, h, nb, dtype)[0], nf.flows.Permute(d, mode="swap")]
    model = nf.NormalizingFlow(nf.distributions.DiagGaussian(d), flows).to(dtype).cuda().eval()

    def sample(fused):
        def call(i):
            for f in flows[::2]:
                f.mprqat.fuse_sampling = fused
            with torch.no_grad():
                model.sample(b)
        return call
    return {"one launch": sample(True), "fuse_sampling = False (the loop, the parent's path)": sample(False)}


def _launches(call):
    from torch.profiler import ProfilerActivity, profile
    call(0)
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        call(0)
        torch.cuda.synchronize()
    return sum(e.count for e in prof.key_averages() if e.device_type == torch.autograd.DeviceType.CUDA
               and not e.key.lower().startswith(("memcpy", "memset")))


def run(shapes, window, reps, out, model=False, launches=False):
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    last = "kernels per call" if launches else "us per call | spread | x one launch"
    lines = ["| B | D | H | blocks | dtype | call | variant | %s |" % last, "|---|---|---|---|---|---|---|%s" % ("---|" * (1 if launches else 3))]
    torch.manual_seed(17)
    groups = [(s, kind) for s in shapes for kind in ("spline", "affine")] + ([((MODEL_BATCH,) + shapes[0][1:], "model")] if model else [])
    for (b, d, h, nb), kind in groups:
        for dtype in (torch.float32, torch.float64):
            variants = _model_variants(b, d, h, nb, dtype) if kind == "model" else _variants(b, d, h, nb, kind, dtype)
            what = {"spline": "AutoregressiveRationalQuadraticSpline.forward", "affine": "MaskedAffineAutoregressive.inverse",
                    "model": "sample(B), 16 spline layers + Permutes"}[kind]
            results, failed = ({}, {}) if launches else bw.measure(variants, window, reps)
            for name in variants:
                lead = "| %d | %d | %d | %d | %s | %s | %s |" % (b, d, h, nb, bw.dtype_name(dtype), what, name)
                if launches:
                    lines.append("%s %d |" % (lead, _launches(variants[name])))
                elif name in failed:
                    lines.append("%s failed: %s | | |" % (lead, failed[name]))
                else:
                    med, spread, _ = results[name]
                    base = results.get("one launch")
                    lines.append("%s %.1f | %.3f | %s |" % (lead, med * 1e6, spread, "%.2f" % (med / base.median) if base else ""))
                print(lines[-1], flush=True)
            del variants
            torch.cuda.empty_cache()
    return bw.finish(lines, window, reps, out)


if __name__ == "__main__":
    ap = bw.parser(0.2)
    ap.add_argument("--shapes", default=SHAPES)
    ap.add_argument("--model", action="store_true", help="also sample(2048) of a 16-layer model of the first shape's D, H, blocks")
    ap.add_argument("--launches", action="store_true", help="count device kernels per call instead of timing")
    a = ap.parse_args()
    run([tuple(int(v) for v in s.split("x")) for s in a.shapes.split(",")], a.window, a.reps, a.out, a.model, a.launches)
