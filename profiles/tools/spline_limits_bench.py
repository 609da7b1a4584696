"""Per-element interval limits against the scalar-limit spline: kernel times of vcnf_rqs_elementwise_{f32,f64} (limits
in the config, the path of Python-float limits) and vcnf_rqs_elementwise_limits_{f32,f64} with full-shape limits
(period n) and with [64] limits broadcast against [n / 64, 64] (L2-resident), and the same for the VJPs
(vcnf_rqs_elementwise_bwd_* against vcnf_rqs_elementwise_limits_bwd_* writing all four per-element limit gradients).

Device events around single launches after warm-up; the variants of one (dtype, K, pass) are alternated for --reps
rounds; median and spread (max - min) / median per variant.  The byte model counts what each kernel must move once:
forward x + 3 logit rows + y + log-det (+ 16 B per element for full-shape fp32 limits); VJP additionally the two
upstream gradients, g_x and the 3 logit-gradient rows (+ the per-element limit gradients).

    python profiles/tools/spline_limits_bench.py [--n 33554432] [--reps 25] [--out FILE]
"""
import argparse
import ctypes
import os
import statistics
import sys

import torch

sys.path[:0] = [os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))]
from vcnf_amd import _lib  # noqa: E402

_ptr = _lib._ptr


def _case(n, k, dtype, g):
    x = torch.rand(n, device="cuda", dtype=dtype, generator=g) * 1.6 - 0.8
    uw, uh, ud = (torch.randn(n, m, device="cuda", dtype=dtype, generator=g) for m in (k, k, k + 1))
    gy, gl = (torch.randn(n, device="cuda", dtype=dtype, generator=g) for _ in range(2))
    return x, uw, uh, ud, gy, gl


def _launchers(n, k, dtype, bwd):
    g = torch.Generator(device="cuda").manual_seed(k)
    x, uw, uh, ud, gy, gl = _case(n, k, dtype, g)
    sfx = "_f64" if dtype == torch.float64 else "_f32"
    cfg = _lib.make_cfg(k, None, left=-1.0, right=1.0, bottom=-1.0, top=1.0)
    cfgp = ctypes.byref(cfg.f64 if dtype == torch.float64 else cfg)
    L = _lib.lib()
    stream = _lib._stream()
    y, lad, gx = (torch.empty_like(x) for _ in range(3))
    gw, gh, gd = torch.empty_like(uw), torch.empty_like(uh), torch.empty_like(ud)
    glim = [torch.empty_like(x) for _ in range(4)]
    full = [torch.full((n,), v, device="cuda", dtype=dtype) for v in (-1.0, 1.0, -1.0, 1.0)]
    row = [torch.full((64,), v, device="cuda", dtype=dtype) for v in (-1.0, 1.0, -1.0, 1.0)]
    bc_full = _lib.RqsLimitBcast((ctypes.c_int64 * 4)(*[n] * 4), (ctypes.c_int64 * 4)(*[1] * 4))
    bc_row = _lib.RqsLimitBcast((ctypes.c_int64 * 4)(*[64] * 4), (ctypes.c_int64 * 4)(*[1] * 4))
    common = (_ptr(x), _ptr(uw), _ptr(uh), _ptr(ud), k, k, k + 1)

    def check(st, what):
        if st != 0:
            raise RuntimeError("%s returned status %d" % (what, st))

    if not bwd:
        def scalar():
            check(getattr(L, "vcnf_rqs_elementwise" + sfx)(*common, _ptr(y), _ptr(lad), n, cfgp, 0, None, stream), "fwd")

        def limits(lims, bc):
            return lambda: check(getattr(L, "vcnf_rqs_elementwise_limits" + sfx)(
                *common, *[_ptr(t) for t in lims], ctypes.byref(bc), _ptr(y), _ptr(lad), n, cfgp, 0, None, stream),
                "fwd limits")
    else:
        def scalar():
            check(getattr(L, "vcnf_rqs_elementwise_bwd" + sfx)(*common, _ptr(gy), _ptr(gl), _ptr(gx), _ptr(gw), _ptr(gh),
                                                              _ptr(gd), n, cfgp, 0, stream), "bwd")

        def limits(lims, bc):
            return lambda: check(getattr(L, "vcnf_rqs_elementwise_limits_bwd" + sfx)(
                *common, *[_ptr(t) for t in lims], ctypes.byref(bc), _ptr(gy), _ptr(gl), _ptr(gx), _ptr(gw), _ptr(gh),
                _ptr(gd), *[_ptr(t) for t in glim], n, cfgp, 0, stream), "bwd limits")
    return {"scalar": scalar, "full": limits(full, bc_full), "[64]": limits(row, bc_row)}


def _bytes(n, k, es, bwd, variant):
    per = es * (1 + 2 * k + (k + 1)) + 2 * es                 # x, logits; y + lad (fwd) or gy + glad (bwd)
    if bwd:
        per += es * (1 + 2 * k + (k + 1))                    # g_x, logit gradients
    if variant == "full":
        per += 4 * es                                        # the four limits, read per element
    if bwd and variant != "scalar":
        per += 4 * es                                        # per-element limit gradients
    return per * n


def run(n, reps, out):
    lines = ["| dtype | K | pass | variant | median ms | spread | ratio to scalar | byte ratio | GB/s |",
             "|---|---|---|---|---|---|---|---|---|"]
    for dtype in (torch.float32, torch.float64):
        for k in (8, 10):
            for bwd in (False, True):
                fns = _launchers(n, k, dtype, bwd)
                for fn in fns.values():                      # warm-up
                    for _ in range(3):
                        fn()
                torch.cuda.synchronize()
                times = {name: [] for name in fns}
                for _ in range(reps):
                    for name, fn in fns.items():
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record()
                        fn()
                        e1.record()
                        times[name].append((e0, e1))
                torch.cuda.synchronize()
                es = 8 if dtype == torch.float64 else 4
                med = {}
                for name, evs in times.items():
                    ms = [a.elapsed_time(b) for a, b in evs]
                    med[name] = statistics.median(ms)
                    spread = (max(ms) - min(ms)) / med[name]
                    b = _bytes(n, k, es, bwd, name)
                    ratio = med[name] / med["scalar"]
                    lines.append("| %s | %d | %s | %s | %.4f | %.3f | %.3f | %.3f | %.0f |" % (
                        "fp64" if es == 8 else "fp32", k, "VJP" if bwd else "forward", name, med[name], spread, ratio,
                        b / _bytes(n, k, es, bwd, "scalar"), b / med[name] / 1e6))
                    print(lines[-1], flush=True)
                del fns
                torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n"
    if out:
        with open(out, "w") as f:
            f.write("n = %d, %d alternated repetitions\n\n" % (n, reps) + text)
    return text


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 25)
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    run(a.n, a.reps, a.out)
