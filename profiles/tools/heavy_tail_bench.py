"""StudentT / GeneralizedGaussian base against the two things a user has without it, on the same GPU in the same
process: the plain-torch restatement of the same arithmetic (tests/heavy_tail_ref.py, run on the device) and the
existing DiagGaussian module at the same shape.  D = 64, B = 2048 and 1 048 576, fp32 and fp64; per variant log_prob,
from_noise with both draws given, and log_prob forward plus backward (loss = sum_b g_b log p_b, gradients to z and the
parameters).  The module-level calls are what a training loop pays, Python included; the vcnf_tail_* entry points are
also called directly, and those rows carry the algorithmic bytes (what must move once, from the shapes) and GB/s.

Timing: the protocol of bench_windows.py, the variants of one (batch, dtype, family) alternated.  Successive calls rotate
over enough input / output buffers to exceed 512 MiB (twice the Infinity Cache), so the rows come from HBM.

    python profiles/tools/heavy_tail_bench.py [--batches 2048,1048576] [--window 0.2] [--reps 5] [--out FILE]
"""
import torch

import bench_windows as bw         # first: it puts the repository root and tests/ on sys.path
import heavy_tail_ref as ref
import vcnf_amd as nf
from vcnf_amd import _lib

_ptr = _lib._ptr
D = 64
CLASSES = {"student_t": "StudentT", "gen_gaussian": "GeneralizedGaussian"}
_check = bw.checked               # module-level names, as the calls below always had: a launch-bound row is host time


def _variants(b, family, dtype, g):
    """name -> (call(i), algorithmic bytes or None); call(i) uses buffer set i % sets."""
    es = 8 if dtype == torch.float64 else 4
    sfx = "_f64" if es == 8 else "_f32"
    sets = bw.rotation_sets(b * D * es)
    rnd = lambda *s: torch.randn(*s, device="cuda", dtype=dtype, generator=g)
    q = getattr(nf.distributions, CLASSES[family])(D).to(dtype).cuda()
    with torch.no_grad():
        q.loc.copy_(2.0 * rnd(1, D))
        q.log_scale.copy_(0.3 * rnd(1, D))
        un = torch.rand(1, D, device="cuda", dtype=dtype, generator=g)
        getattr(q, ref.TAIL[family]).copy_(torch.log(1.5 + 28.5 * un) if family == "student_t" else torch.log(0.6 + 1.9 * un))
        loc, ls, tail, cst, conc = [t.detach().contiguous() for t in q._rows()]
        eps = rnd(sets, b, D)
        gamma = torch._standard_gamma(conc.expand(sets, b, D).contiguous())
        zs = torch.stack([q.from_noise(eps[i], gamma[i])[0] for i in range(sets)])
    p = {k: v.detach() for k, v in q.named_parameters()}
    dg = nf.distributions.DiagGaussian(D).to(dtype).cuda()
    with torch.no_grad():
        dg.loc.copy_(q.loc)
        dg.log_scale.copy_(q.log_scale)
    outs = torch.empty(sets, b, D, device="cuda", dtype=dtype)
    gvec = rnd(b)
    logp = torch.empty(b, device="cuda", dtype=dtype)
    L = _lib.lib()
    stream = _lib._stream()
    fn = lambda name: getattr(L, name + sfx)
    fam = q._family
    groups = int(L.vcnf_tail_bwd_groups(b, D))
    partials = torch.empty(groups, 3, D, device="cuda", dtype=dtype)
    sums = torch.empty(3, D, device="cuda", dtype=dtype)
    rows_bytes, block = 4 * D * es, 3 * D * es

    def k_log_prob(i):
        _check(fn("vcnf_tail_log_prob")(_ptr(zs[i % sets]), _ptr(loc), _ptr(ls), _ptr(tail), _ptr(cst), _ptr(logp), b, D, fam, 0,
                                        1.0, stream), "log_prob")

    def k_sample(i):
        k = i % sets
        _check(fn("vcnf_tail_sample")(_ptr(eps[k]), _ptr(gamma[k]), _ptr(loc), _ptr(ls), _ptr(tail), _ptr(cst), _ptr(outs[k]),
                                      _ptr(logp), b, D, fam, stream), "sample")

    def k_vjp(i):
        k = i % sets
        _check(fn("vcnf_tail_log_prob_bwd")(_ptr(zs[k]), _ptr(loc), _ptr(ls), _ptr(tail), _ptr(gvec), None, _ptr(outs[k]),
                                            _ptr(partials), b, D, fam, stream), "log_prob_bwd")
        _check(fn("vcnf_tail_reduce_partials")(_ptr(partials), groups, D, _ptr(sums[0]), _ptr(sums[1]), _ptr(sums[2]), stream),
               "reduce_partials")

    def module_fwd_bwd(mod):
        def call(i):
            mod.zero_grad(set_to_none=True)
            z = zs[i % sets].detach().requires_grad_()
            (mod.log_prob(z) * gvec).sum().backward()
        return call

    def module_log_prob(mod):
        def call(i):
            with torch.no_grad():
                mod.log_prob(zs[i % sets])
        return call

    def tail_from_noise(i):
        with torch.no_grad():
            q.from_noise(eps[i % sets], gamma[i % sets])

    def diag_from_noise(i):
        with torch.no_grad():
            dg.from_noise(eps[i % sets])

    leaves = {k: v.clone().requires_grad_() for k, v in p.items()}

    def eager_lp(i):
        with torch.no_grad():
            ref.log_prob(family, zs[i % sets], p)

    def eager_sample(i):
        with torch.no_grad():
            ref.sample(family, eps[i % sets], gamma[i % sets], p)

    def eager_fwd_bwd(i):
        z = zs[i % sets].detach().requires_grad_()
        lp = ref.log_prob(family, z, leaves)
        torch.autograd.grad(lp, [z] + list(leaves.values()), gvec)

    name = CLASSES[family]
    return {"vcnf_tail_log_prob": (k_log_prob, es * b * D + rows_bytes + es * b),
            "vcnf_tail_sample": (k_sample, 3 * es * b * D + rows_bytes + es * b),
            "vcnf_tail_log_prob_bwd + reduce_partials": (k_vjp, 2 * es * b * D + es * b + rows_bytes + 2 * groups * block + block),
            name + ".log_prob": (module_log_prob(q), None),
            name + ".from_noise(eps, gamma)": (tail_from_noise, None),
            name + " log_prob forward + backward": (module_fwd_bwd(q), None),
            "torch restatement log_prob": (eager_lp, None),
            "torch restatement sample": (eager_sample, None),
            "torch restatement log_prob forward + backward": (eager_fwd_bwd, None),
            "DiagGaussian.log_prob": (module_log_prob(dg), None),
            "DiagGaussian.from_noise(eps)": (diag_from_noise, None),
            "DiagGaussian log_prob forward + backward": (module_fwd_bwd(dg), None)}


def run(batches, window, reps, out):
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    lines = ["| B | dtype | family | variant | us per call | spread | bytes | GB/s | of 8 TB/s |", "|---|---|---|---|---|---|---|---|---|"]
    g = torch.Generator(device="cuda").manual_seed(17)
    torch.manual_seed(17)
    for b in batches:
        for dtype in (torch.float32, torch.float64):
            for family in ref.FAMILIES:
                variants = _variants(b, family, dtype, g)
                results, failed = bw.measure({name: v[0] for name, v in variants.items()}, window, reps)
                for name, (_, nbytes) in variants.items():
                    lead = "| %d | %s | %s | %s |" % (b, bw.dtype_name(dtype), family, name)
                    if name in failed:
                        lines.append("%s failed: %s | | | | |" % (lead, failed[name]))
                    else:
                        med, spread, _ = results[name]
                        lines.append("%s %.2f | %.3f | %s | %s | %s |" % (
                            lead, med * 1e6, spread, "" if nbytes is None else "%d" % nbytes,
                            "" if nbytes is None else "%.0f" % (nbytes / med / 1e9),
                            "" if nbytes is None else "%.2f" % (nbytes / med / bw.HBM_PEAK)))
                    print(lines[-1], flush=True)
                del variants
                torch.cuda.empty_cache()
    return bw.finish(lines, window, reps, out)


if __name__ == "__main__":
    ap = bw.parser(0.2)
    ap.add_argument("--batches", default="2048,1048576")
    a = ap.parse_args()
    run([int(v) for v in a.batches.split(",")], a.window, a.reps, a.out)
