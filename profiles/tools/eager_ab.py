"""Eager log_prob latency of two checkouts' host code in ONE process, alternating, so that what moves a whole process
(the machine's other work, clocks) moves both alike: this checkout's vcnf_amd against the package of another checkout,
loaded under another name.  Device code is the same library in both when only host code differs.

    python profiles/tools/eager_ab.py OTHER_CHECKOUT [BATCH]

Rows: C3 on the three-step path (host-bound, one planner call per layer), C3 fp16x3 (12 layers in one launch), C2 (the
affine family's run), Glow (one GlowBlock(24, 32) on [B, 24, 8, 8]: the composed mixer and the packed 1x1 convolution).  Ten alternating rounds each; minimum, median and maximum per side."""
import importlib.util
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import torch            # noqa: E402
import vcnf_amd as new  # noqa: E402


def load_as(name, root):
    pkg = os.path.join(os.path.abspath(root), "vcnf_amd")
    spec = importlib.util.spec_from_file_location(name, os.path.join(pkg, "__init__.py"), submodule_search_locations=[pkg])
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def c3(nf, **attrs):
    torch.manual_seed(0)
    flows = [nf.flows.CoupledRationalQuadraticSpline(64, 2, 128, 8, reverse_mask=bool(i % 2), num_context_channels=16)
             for i in range(12)]
    m = nf.NormalizingFlow(nf.distributions.DiagGaussian(64), flows).cuda()
    for f in flows:
        for k, v in attrs.items():
            setattr(f.prqct, k, v)
    return m


def c2(nf):
    torch.manual_seed(0)
    flows = []
    for _ in range(8):
        flows += [nf.flows.AffineCouplingBlock(nf.nets.MLP([16, 64, 64, 32])), nf.flows.Permute(32, mode="swap")]
    return nf.NormalizingFlow(nf.distributions.DiagGaussian(32), flows).cuda()


def glow(nf):
    torch.manual_seed(0)
    m = nf.NormalizingFlow(nf.distributions.DiagGaussian((24, 8, 8)), [nf.flows.GlowBlock(24, 32, init_zeros=False)]).cuda()
    return m.eval()         # (the first of the warm-up calls initialises the ActNorm)


def timeit(fn, n):
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / n * 1e3


def main():
    old = load_as("vcnf_other", sys.argv[1])
    b = int(sys.argv[2]) if len(sys.argv) > 2 else 2048
    rows = (("C3 split (three-step)", lambda nf: c3(nf, fused=False), 64, 16, 100), ("C3 fp16x3", c3, 64, 16, 500),
            ("C2", c2, 32, None, 500), ("Glow", glow, (24, 8, 8), None, 500))
    for name, mk, d, c, n in rows:
        x = torch.randn(b, d, device="cuda") if isinstance(d, int) else torch.randn(b, *d, device="cuda")
        kw = {"context": torch.randn(b, c, device="cuda")} if c else {}
        models = {"other": mk(old), "this": mk(new)}
        res = {k: [] for k in models}
        with torch.no_grad():
            for m in models.values():
                for _ in range(20):
                    m.log_prob(x, **kw)
            for _ in range(10):
                for k, m in models.items():
                    res[k].append(timeit(lambda: m.log_prob(x, **kw), n))
        for k, v in res.items():
            print("%s B=%d eager log_prob, %s: min %.4f median %.4f max %.4f ms" % (name, b, k, min(v), sorted(v)[5], max(v)),
                  flush=True)


if __name__ == "__main__":
    main()
