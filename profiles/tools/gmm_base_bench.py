"""GaussianMixture base kernels against the eager-torch restatement of the same arithmetic on the same GPU: per-call
times of vcnf_gmm_log_prob / _sample / _log_prob_bwd + _reduce_partials (fp32 and fp64) and, alternated with them in
the same process, of the plain-torch form (the only other way the library could compute this), at
(modes, features) = (1, 64), (8, 2), (16, 64), (64, 30) and B = 16 384 and 1 048 576.  For one mode the existing
vcnf_diag_gaussian_log_prob_f32 on the same rows is a second yardstick.

Timing: the protocol of bench_windows.py, the variants of one (batch, shape, dtype) alternated.  Beside the median and
the spread the table gives the algorithmic bytes of the kernels (what must move once, from the shapes) and GB/s.
Successive calls rotate over enough input / output buffers to exceed 512 MiB (twice the Infinity Cache), so the rows
come from HBM.

    python profiles/tools/gmm_base_bench.py [--batches 16384,1048576] [--window 0.2] [--reps 5] [--out FILE]
"""
import math

import torch

import bench_windows as bw         # first: it puts the repository root and tests/ on sys.path
from vcnf_amd import _lib

_ptr = _lib._ptr
SHAPES = [(1, 64), (8, 2), (16, 64), (64, 30)]
_check = bw.checked               # module-level names, as the calls below always had: a launch-bound row is host time


def eager_log_prob(z, loc, ls, ws):
    w = torch.softmax(ws, 1)
    u = (z[:, None, :] - loc) / torch.exp(ls)
    a = -0.5 * z.shape[1] * math.log(2 * math.pi) + torch.log(w) - 0.5 * torch.sum(u ** 2, 2) - torch.sum(ls, 2)
    return torch.logsumexp(a, 1)


def _variants(b, m, d, dtype, g):
    """name -> (call(i), algorithmic bytes or None); call(i) uses buffer set i % sets."""
    es = 8 if dtype == torch.float64 else 4
    sfx = "_f64" if es == 8 else "_f32"
    sets = bw.rotation_sets(b * d * es)
    rnd = lambda *s: torch.randn(*s, device="cuda", dtype=dtype, generator=g)
    loc, ls, ws = 2.0 * rnd(1, m, d), 0.3 * rnd(1, m, d), rnd(1, m)
    log_w = torch.log_softmax(ws, 1)[0].contiguous()
    loc2, ls2 = loc[0].contiguous(), ls[0].contiguous()
    mode = torch.multinomial(torch.softmax(ws, 1)[0], b, replacement=True, generator=g)
    mode32 = mode.to(torch.int32)
    eps = rnd(sets, b, d)
    zs = eps * torch.exp(ls2[mode]) + loc2[mode]                       # rows from the mixture itself
    outs = torch.empty(sets, b, d, device="cuda", dtype=dtype)
    gvec = rnd(b)
    logp = torch.empty(b, device="cuda", dtype=dtype)
    L = _lib.lib()
    stream = _lib._stream()
    fn = lambda name: getattr(L, name + sfx)
    groups = int(L.vcnf_gmm_bwd_groups(b, d, m))
    partials = torch.empty(groups, m, 2 * d + 1, device="cuda", dtype=dtype)
    d_loc, d_ls, d_w = torch.empty_like(loc2), torch.empty_like(ls2), torch.empty_like(log_w)
    lse = torch.empty(sets, b, device="cuda", dtype=dtype)
    for i in range(sets):
        _check(fn("vcnf_gmm_log_prob")(_ptr(zs[i]), _ptr(loc2), _ptr(ls2), _ptr(log_w), _ptr(lse[i]), b, d, m, 0, 1.0, stream), "lse")
    table = (2 * m * d + m) * es
    block = m * (2 * d + 1) * es

    def gmm_log_prob(i):
        _check(fn("vcnf_gmm_log_prob")(_ptr(zs[i % sets]), _ptr(loc2), _ptr(ls2), _ptr(log_w), _ptr(logp), b, d, m, 0, 1.0,
                                       stream), "gmm log_prob")

    def gmm_sample(i):
        _check(fn("vcnf_gmm_sample")(_ptr(eps[i % sets]), _ptr(mode32), _ptr(loc2), _ptr(ls2), _ptr(log_w), _ptr(outs[i % sets]),
                                     _ptr(logp), b, d, m, stream), "gmm sample")

    def gmm_vjp(i):
        k = i % sets
        _check(fn("vcnf_gmm_log_prob_bwd")(_ptr(zs[k]), _ptr(loc2), _ptr(ls2), _ptr(log_w), _ptr(lse[k]), _ptr(gvec), None,
                                           _ptr(outs[k]), _ptr(partials), b, d, m, stream), "gmm log_prob_bwd")
        _check(fn("vcnf_gmm_reduce_partials")(_ptr(partials), groups, m, d, _ptr(d_loc), _ptr(d_ls), _ptr(d_w), stream),
               "gmm reduce_partials")

    def gmm_fwd_vjp(i):
        k = i % sets
        _check(fn("vcnf_gmm_log_prob")(_ptr(zs[k]), _ptr(loc2), _ptr(ls2), _ptr(log_w), _ptr(lse[k]), b, d, m, 0, 1.0, stream),
               "gmm log_prob")
        gmm_vjp(i)

    leaves = [t.clone().requires_grad_() for t in (loc, ls, ws)]

    def eager_lp(i):
        with torch.no_grad():
            eager_log_prob(zs[i % sets], loc, ls, ws)

    def eager_sample(i):
        with torch.no_grad():
            z = eps[i % sets] * torch.exp(ls[0, mode]) + loc[0, mode]
            eager_log_prob(z, loc, ls, ws)

    def eager_fwd_vjp(i):
        z = zs[i % sets].detach().requires_grad_()
        lp = eager_log_prob(z, *leaves)
        torch.autograd.grad(lp, [z] + leaves, gvec)

    out = {"gmm log_prob": (gmm_log_prob, es * b * d + table + es * b),
           "gmm sample": (gmm_sample, 2 * es * b * d + 4 * b + table + es * b),
           "gmm log_prob VJP + reduce": (gmm_vjp, 2 * es * b * d + 2 * es * b + table + 2 * groups * block + block),
           "gmm log_prob + VJP + reduce": (gmm_fwd_vjp, None),
           "eager log_prob": (eager_lp, None),
           "eager sample": (eager_sample, None),
           "eager log_prob + autograd": (eager_fwd_vjp, None)}
    if es == 4 and m == 1:
        def dg_log_prob(i):
            _check(L.vcnf_diag_gaussian_log_prob_f32(_ptr(zs[i % sets]), _ptr(loc2), _ptr(ls2), 0.0, _ptr(logp), b, d, 0, 1.0,
                                                     stream), "diag log_prob")
        out["diag log_prob (M = 1 yardstick)"] = (dg_log_prob, es * b * d + 2 * d * es + es * b)
    return out


def run(batches, window, reps, out):
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    lines = ["| B | (M, D) | dtype | variant | us per call | spread | bytes | GB/s |", "|---|---|---|---|---|---|---|---|"]
    g = torch.Generator(device="cuda").manual_seed(17)
    for b in batches:
        for m, d in SHAPES:
            for dtype in (torch.float32, torch.float64):
                variants = _variants(b, m, d, dtype, g)
                results, failed = bw.measure({name: v[0] for name, v in variants.items()}, window, reps)
                for name, (_, nbytes) in variants.items():
                    lead = "| %d | (%d, %d) | %s | %s |" % (b, m, d, bw.dtype_name(dtype), name)
                    if name in failed:
                        lines.append("%s failed: %s | | | |" % (lead, failed[name]))
                    else:
                        med, spread, _ = results[name]
                        lines.append("%s %.2f | %.3f | %s | %s |" % (
                            lead, med * 1e6, spread, "" if nbytes is None else "%d" % nbytes,
                            "" if nbytes is None else "%.0f" % (nbytes / med / 1e9)))
                    print(lines[-1], flush=True)
                del variants
                torch.cuda.empty_cache()
    return bw.finish(lines, window, reps, out)


if __name__ == "__main__":
    ap = bw.parser(0.2)
    ap.add_argument("--batches", default="16384,1048576")
    a = ap.parse_args()
    run([int(v) for v in a.batches.split(",")], a.window, a.reps, a.out)
