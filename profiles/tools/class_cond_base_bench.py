"""Class-conditional Gaussian end caps against the DiagGaussian kernel on the same bytes: per-call times of
vcnf_cc_gaussian_log_prob / _sample / _log_prob_bwd (fp32 and fp64, hard labels, 10 classes) at config C4's three base
shapes, and, alternated with them in the same process, of vcnf_diag_gaussian_log_prob_f32 / _sample_f32 on the
flattened [B, d] problem of the same size (the yardstick: it reads the same z bytes; the class-conditional kernel reads
4 B of label per sample more and 2 * 10 * C parameters instead of 2 * d).

Timing: the protocol of bench_windows.py, the variants of one (shape, dtype) alternated.  Beside the median and the spread
the table gives the algorithmic bytes (what the kernel must move once, from the shapes), GB/s and that as a share of the
HBM peak (8.0 TB/s specified; a float4 copy measures 6.29 TB/s on this part).  Successive calls rotate over enough
input / output buffers to exceed twice the 256 MiB Infinity Cache, so the bytes come from HBM.

    python profiles/tools/class_cond_base_bench.py [--batch 16384] [--window 0.3] [--reps 5] [--out FILE]
"""
import torch

import bench_windows as bw         # first: it puts the repository root and tests/ on sys.path
from vcnf_amd import _lib

_ptr = _lib._ptr
SHAPES = [(48, 4, 4), (12, 8, 8), (6, 16, 16)]
NUM_CLASSES = 10
_check = bw.checked               # module-level names, as the calls below always had: a launch-bound row is host time


def _variants(b, shape, dtype, g):
    """name -> (launch(i), algorithmic bytes); launch(i) uses buffer set i % sets."""
    c, p = shape[0], shape[1] * shape[2]
    d = c * p
    es = 8 if dtype == torch.float64 else 4
    sfx = "_f64" if es == 8 else "_f32"
    sets = bw.rotation_sets(b * d * es)
    rnd = lambda *s: torch.randn(*s, device="cuda", dtype=dtype, generator=g)
    zs = [rnd(b, d) for _ in range(sets)]
    outs = [torch.empty(b, d, device="cuda", dtype=dtype) for _ in range(sets)]
    loc, ls = 0.3 * rnd(NUM_CLASSES, c), 0.3 * rnd(NUM_CLASSES, c)
    floc, fls = 0.3 * rnd(d), 0.3 * rnd(d)
    y = torch.randint(NUM_CLASSES, (b,), device="cuda", generator=g).to(torch.int32)
    gvec = rnd(b)
    logp = torch.empty(b, device="cuda", dtype=dtype)
    d_loc, d_ls = torch.empty(b, c, device="cuda", dtype=dtype), torch.empty(b, c, device="cuda", dtype=dtype)
    L = _lib.lib()
    stream = _lib._stream()
    fn = lambda name: getattr(L, name + sfx)
    table = 2 * NUM_CLASSES * c * es

    def cc_log_prob(i):
        _check(fn("vcnf_cc_gaussian_log_prob")(_ptr(zs[i % sets]), _ptr(loc), _ptr(ls), _ptr(y), 0.0, _ptr(logp), b, c, p,
                                               NUM_CLASSES, 0, 1.0, stream), "cc log_prob")

    def cc_sample(i):
        _check(fn("vcnf_cc_gaussian_sample")(_ptr(zs[i % sets]), _ptr(loc), _ptr(ls), _ptr(y), 0.0, _ptr(outs[i % sets]),
                                             _ptr(logp), b, c, p, NUM_CLASSES, stream), "cc sample")

    def cc_log_prob_bwd(i):
        _check(fn("vcnf_cc_gaussian_log_prob_bwd")(_ptr(zs[i % sets]), _ptr(loc), _ptr(ls), _ptr(y), 0.0, _ptr(gvec),
                                                   _ptr(outs[i % sets]), _ptr(d_loc), _ptr(d_ls), b, c, p, NUM_CLASSES,
                                                   stream), "cc log_prob_bwd")

    out = {"cc log_prob": (cc_log_prob, es * b * d + 4 * b + table + es * b),
           "cc sample": (cc_sample, 2 * es * b * d + 4 * b + table + es * b),
           "cc log_prob VJP": (cc_log_prob_bwd, 2 * es * b * d + 4 * b + table + es * b + 2 * es * b * c)}
    if es == 4:
        def dg_log_prob(i):
            _check(L.vcnf_diag_gaussian_log_prob_f32(_ptr(zs[i % sets]), _ptr(floc), _ptr(fls), 0.0, _ptr(logp), b, d, 0, 1.0,
                                                     stream), "diag log_prob")

        def dg_sample(i):
            _check(L.vcnf_diag_gaussian_sample_f32(_ptr(zs[i % sets]), _ptr(floc), _ptr(fls), 0.0, _ptr(outs[i % sets]),
                                                   _ptr(logp), b, d, stream), "diag sample")
        out["diag log_prob (yardstick)"] = (dg_log_prob, es * b * d + 2 * d * es + es * b)
        out["diag sample (yardstick)"] = (dg_sample, 2 * es * b * d + 2 * d * es + es * b)
    return out


def run(batch, window, reps, out):
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    lines = ["| shape | dtype | kernel | us per call | spread | bytes | GB/s | share of 8.0 TB/s |",
             "|---|---|---|---|---|---|---|---|"]
    g = torch.Generator(device="cuda").manual_seed(17)
    for shape in SHAPES:
        for dtype in (torch.float32, torch.float64):
            variants = _variants(batch, shape, dtype, g)
            results, failed = bw.measure({name: v[0] for name, v in variants.items()}, window, reps)
            for name, (_, nbytes) in variants.items():
                lead = "| %s | %s | %s |" % ("x".join(map(str, shape)), bw.dtype_name(dtype), name)
                if name in failed:
                    lines.append("%s failed: %s | | | | |" % (lead, failed[name]))
                else:
                    med, spread, _ = results[name]
                    lines.append("%s %.2f | %.3f | %d | %.0f | %.1f %% |" % (
                        lead, med * 1e6, spread, nbytes, nbytes / med / 1e9, 100.0 * nbytes / med / bw.HBM_PEAK))
                print(lines[-1], flush=True)
            del variants
            torch.cuda.empty_cache()
    return bw.finish(lines, window, reps, out, "B = %d, hard labels, %d classes, windows of >= %.2f s, %d alternated windows "
                     "per kernel" % (batch, NUM_CLASSES, window, reps))


if __name__ == "__main__":
    ap = bw.parser(0.3)
    ap.add_argument("--batch", type=int, default=16384)
    a = ap.parse_args()
    run(a.batch, a.window, a.reps, a.out)
