"""MultivariateGaussian / MultivariateStudentT base against what a user has without it, on the same GPU in the same
process: the plain-torch composition of the same arithmetic (tests/mvn_ref.py run on the device: solve_triangular on
the [B, D] right-hand side, square, row sum and the elementwise tail, plus autograd for the backward).  Shapes
(B, D) = (2048, 16), (1 048 576, 64), (1 048 576, 128), fp32 and fp64; per variant log_prob, from_noise with the draws
given, and log_prob forward plus backward (loss = sum_b g_b log p_b, gradients to z and the parameters).  The
module-level calls are what a training loop pays, Python and the D x D solve included; the vcnf_mvn_* entry points are
also called directly, and those rows carry the algorithmic bytes (what must move once, from the shapes), GB/s, and the
multiply-adds of the triangular products (D (D + 1) / 2 per sample and product) as GFMA/s.

Timing: the protocol of bench_windows.py, the variants of one (shape, dtype, family) alternated; a variant the libraries
cannot run at a shape (the torch composition's solve at the largest) gets its `failed:` row.  Successive calls rotate
over enough input / output buffers to exceed 512 MiB (twice the Infinity Cache), so the rows come from HBM.

    python profiles/tools/mvn_bench.py [--shapes 2048x16,1048576x64,1048576x128] [--window 0.2] [--reps 5] [--out FILE]
"""
import torch

import bench_windows as bw         # first: it puts the repository root and tests/ on sys.path
import mvn_ref as ref
import vcnf_amd as nf
from vcnf_amd import _lib

_ptr = _lib._ptr
CLASSES = {"gaussian": "MultivariateGaussian", "student_t": "MultivariateStudentT"}
_check = bw.checked               # module-level names, as the calls below always had: a launch-bound row is host time


def _variants(b, d, family, dtype):
    """name -> (call(i), algorithmic bytes or None, triangular products per sample); call(i) uses buffer set i % sets."""
    es = 8 if dtype == torch.float64 else 4
    sfx = "_f64" if es == 8 else "_f32"
    sets = bw.rotation_sets(b * d * es)
    p = ref.cast(ref.inputs(family, d, 8)[0], dtype)
    q = getattr(nf.distributions, CLASSES[family])(d).to(dtype)
    q.load_state_dict(p)
    q = q.cuda()
    p = {k: v.cuda() for k, v in p.items()}
    student = family == "student_t"
    with torch.no_grad():
        loc, tri, consts = q.loc.reshape(-1).contiguous(), q.scale_tril.contiguous(), q._consts().contiguous()
        tri_inv = q._inverse(tri).contiguous()
        eps = torch.randn(sets, b, d, device="cuda", dtype=dtype)
        gamma = q._gamma(sets * b).reshape(sets, b).contiguous() if student else None
        zs = torch.stack([q.from_noise(*((eps[i], gamma[i]) if student else (eps[i],)))[0] for i in range(sets)])
    outs = torch.empty(sets, b, d, device="cuda", dtype=dtype)
    gvec = torch.randn(b, device="cuda", dtype=dtype)
    logp = torch.empty(b, device="cuda", dtype=dtype)
    L = _lib.lib()
    stream = _lib._stream()
    fn = lambda name: getattr(L, name + sfx)
    fam = q._family
    groups = int(L.vcnf_mvn_bwd_groups(b, d))
    block = d * d + d + 1
    partials = torch.empty(groups, block, device="cuda", dtype=dtype)
    d_loc, d_tri, d_nu = (torch.empty(n, device="cuda", dtype=dtype) for n in (d, d * d, 1))
    small = (d * d + d + 2) * es

    def k_log_prob(i):
        _check(fn("vcnf_mvn_log_prob")(_ptr(zs[i % sets]), _ptr(loc), _ptr(tri_inv), _ptr(consts), _ptr(logp), b, d, fam, 0, 1.0,
                                       stream), "log_prob")

    def k_sample(i):
        k = i % sets
        _check(fn("vcnf_mvn_sample")(_ptr(eps[k]), _ptr(gamma[k]) if student else None, _ptr(loc), _ptr(tri), _ptr(consts),
                                     _ptr(outs[k]), _ptr(logp), b, d, fam, stream), "sample")

    def k_vjp(i):
        k = i % sets
        _check(fn("vcnf_mvn_log_prob_bwd")(_ptr(zs[k]), _ptr(loc), _ptr(tri_inv), _ptr(consts), _ptr(gvec), None, _ptr(outs[k]),
                                           _ptr(partials), b, d, fam, stream), "log_prob_bwd")
        _check(fn("vcnf_mvn_reduce_partials")(_ptr(partials), groups, d, _ptr(d_loc), _ptr(d_tri), _ptr(d_nu), stream),
               "reduce_partials")

    def module_log_prob(i):
        with torch.no_grad():
            q.log_prob(zs[i % sets])

    def module_from_noise(i):
        with torch.no_grad():
            q.from_noise(*((eps[i % sets], gamma[i % sets]) if student else (eps[i % sets],)))

    def module_fwd_bwd(i):
        q.zero_grad(set_to_none=True)
        z = zs[i % sets].detach().requires_grad_()
        (q.log_prob(z) * gvec).sum().backward()

    leaves = {k: v.clone().requires_grad_() for k, v in p.items()}

    def eager_lp(i):
        with torch.no_grad():
            ref.log_prob(family, zs[i % sets], p)

    def eager_sample(i):
        with torch.no_grad():
            ref.sample(family, eps[i % sets], gamma[i % sets] if student else None, p)

    def eager_fwd_bwd(i):
        z = zs[i % sets].detach().requires_grad_()
        lp = ref.log_prob(family, z, leaves)
        torch.autograd.grad(lp, [z] + list(leaves.values()), gvec)

    name = CLASSES[family]
    return {"vcnf_mvn_log_prob": (k_log_prob, es * b * d + small + es * b, 1),
            "vcnf_mvn_sample": (k_sample, 2 * es * b * d + small + es * b * (2 if student else 1), 1),
            "vcnf_mvn_log_prob_bwd + reduce_partials": (k_vjp, 2 * es * b * d + es * b + small + (2 * groups + 1) * block * es, 3),
            name + ".log_prob": (module_log_prob, None, 0),
            name + ".from_noise": (module_from_noise, None, 0),
            name + " log_prob forward + backward": (module_fwd_bwd, None, 0),
            "torch composition log_prob": (eager_lp, None, 0),
            "torch composition sample": (eager_sample, None, 0),
            "torch composition log_prob forward + backward": (eager_fwd_bwd, None, 0)}


def run(shapes, window, reps, out, dtypes=(torch.float32, torch.float64)):
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    lines = ["| B | D | dtype | family | variant | us per call | spread | bytes | GB/s | of 8 TB/s | GFMA/s |",
             "|---|---|---|---|---|---|---|---|---|---|---|"]
    torch.manual_seed(17)
    for b, d in shapes:
        for dtype in dtypes:
            for family in ref.FAMILIES:
                variants = _variants(b, d, family, dtype)
                results, failed = bw.measure({name: v[0] for name, v in variants.items()}, window, reps)
                for name, (_, nbytes, products) in variants.items():
                    lead = "| %d | %d | %s | %s | %s |" % (b, d, bw.dtype_name(dtype), family, name)
                    if name in failed:
                        lines.append("%s failed: %s | | | | | |" % (lead, failed[name]))
                    else:
                        med, spread, _ = results[name]
                        lines.append("%s %.2f | %.3f | %s | %s | %s | %s |" % (
                            lead, med * 1e6, spread, "" if nbytes is None else "%d" % nbytes,
                            "" if nbytes is None else "%.0f" % (nbytes / med / 1e9),
                            "" if nbytes is None else "%.3f" % (nbytes / med / bw.HBM_PEAK),
                            "" if not products else "%.0f" % (products * b * d * (d + 1) / 2 / med / 1e9)))
                    print(lines[-1], flush=True)
                del variants
                torch.cuda.empty_cache()
    return bw.finish(lines, window, reps, out)


if __name__ == "__main__":
    ap = bw.parser(0.2)
    ap.add_argument("--shapes", default="2048x16,1048576x64,1048576x128")
    ap.add_argument("--dtypes", default="fp32,fp64")
    a = ap.parse_args()
    kinds = {"fp32": torch.float32, "fp64": torch.float64}
    run([tuple(int(v) for v in s.split("x")) for s in a.shapes.split(",")], a.window, a.reps, a.out,
        [kinds[k] for k in a.dtypes.split(",")])
