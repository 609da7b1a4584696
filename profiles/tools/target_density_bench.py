"""The target densities (csrc/target_density.hip, vcnf_amd.distributions.target) against what a user has without them:
the plain-torch restatement of the reference's log_prob (tests/target_ref.py) moved to the GPU, on the same GPU in the
same process.  TwoMoons, CircularGaussianMixture(8) and RingMixture(2) in fp32:

  (a) the kernel alone, with and without the score, at B = 1024 and 1 048 576: back-to-back launches of
      _lib.target_log_prob between two device events (at the small batch this is the launch rate, not the kernel), and
      with --launches / --parse-trace the kernel's own time from a rocprofv3 kernel trace taken in a run of its own:
          rocprofv3 --kernel-trace --output-format csv -d DIR -- python profiles/tools/target_density_bench.py --launches
          python profiles/tools/target_density_bench.py --parse-trace DIR
      The share of 8 TB/s counts 12 B per sample without the score and 20 B with it.
  (b) eager p.log_prob(z) forward + backward at B = 1024, Python included: log_prob of a z that requires grad and
      torch.autograd.grad of its sum, for the module and for the restatement.
  (c) reverse_kld(1024) forward + backward of the 32-layer tanh Planar model of profiles/planar_radial.md with the module
      as p, against the same model with the restatement as p.

Timing: the protocol of bench_windows.py, the variants of one row group alternated.

    python profiles/tools/target_density_bench.py [--window 0.2] [--reps 5] [--out FILE]
"""
import csv
import glob
import os
import statistics

import torch

import bench_windows as bw         # first: it puts the repository root and tests/ on sys.path
import planar_radial_ref as pr_ref
import target_ref as ref
import vcnf_amd as nf
from vcnf_amd import _lib

TARGETS = [("two_moons", 0), ("circular", 8), ("ring", 2)]
BATCHES = (1024, 1 << 20)


def module_of(family, n):
    D = nf.distributions
    t = D.TwoMoons() if family == "two_moons" else D.CircularGaussianMixture(n) if family == "circular" else D.RingMixture(n)
    return t.cuda()


class Restatement(torch.nn.Module):
    """The reference's module as a user would port it: log_prob in torch ops, its scale a buffer on the device."""

    def __init__(self, family, n):
        super().__init__()
        self.family, self.n = family, n
        scale = ref.scale_of(family, n)
        if torch.is_tensor(scale):
            self.register_buffer("scale", scale)
        else:
            self.scale = scale

    def log_prob(self, z):
        return ref.log_prob(self.family, self.n, z, self.scale)


def kernel_rows(label, b, calls, window, reps, lines):
    """Part (a) for one density and batch: the kernel wrapper without and with the score, 12 B and 20 B per sample."""
    variants = {("with" if w else "without"): c for w, c in calls.items()}
    results, failed = bw.measure(variants, window, reps)
    for name in variants:
        if name in failed:
            lines.append("| %s | %d | %s | failed: %s | | | |" % (label, b, name, failed[name]))
        else:
            t, spread, _ = results[name]
            rate = b * (20 if name == "with" else 12) / t
            lines.append("| %s | %d | %s | %.1f | %.3f | %.1f | %.3f |" % (label, b, name, t * 1e6, spread, rate * 1e-9, rate / bw.HBM_PEAK))
        print(lines[-1], flush=True)


def ratio_rows(label, variants, base, window, reps, lines):
    """Parts (b) and on: the variants of one density, each with its time as a multiple of ``base``'s."""
    results, failed = bw.measure(variants, window, reps)
    for name in variants:
        if name in failed:
            lines.append("| %s | %s | failed: %s | | |" % (label, name, failed[name]))
        else:
            t, spread, _ = results[name]
            lines.append("| %s | %s | %.1f | %.3f | %s |" % (
                label, name, t * 1e6, spread, "%.2f" % (t / results[base].median) if base in results else ""))
        print(lines[-1], flush=True)


def _z(b):
    g = torch.Generator().manual_seed(ref.seed_of("bench", b))
    return (2.0 * torch.randn(b, 2, generator=g)).cuda()


def kernel_calls(family, n, b):
    """{with score / without: call(i)} on the kernel wrapper, the operands prepared."""
    target = module_of(family, n)
    z = _z(b)
    table, scale = target._operands(z)
    return {want: (lambda i, want=want: _lib.target_log_prob(z, target._family, table, scale, want_score=want))
            for want in (False, True)}


def part_a(window, reps, lines):
    lines += ["", "(a) back-to-back launches of the kernel wrapper", "",
              "| target | B | score | us per call | spread | GB/s | of 8 TB/s |", "|---|---|---|---|---|---|---|"]
    for family, n in TARGETS:
        for b in BATCHES:
            kernel_rows("%s %d" % (family, n), b, kernel_calls(family, n, b), window, reps, lines)


def part_b(window, reps, lines):
    lines += ["", "(b) log_prob forward + backward at B = 1024, eager", "",
              "| target | variant | us per call | spread | x the module |", "|---|---|---|---|---|"]
    z = _z(1024)
    for family, n in TARGETS:
        def fwd_bwd(p):
            def call(i):
                x = z.detach().requires_grad_(True)
                torch.autograd.grad(p.log_prob(x).sum(), x)
            return call
        ratio_rows("%s %d" % (family, n), {"module (one launch + one multiply)": fwd_bwd(module_of(family, n)),
                                           "torch restatement": fwd_bwd(Restatement(family, n).cuda())},
                   "module (one launch + one multiply)", window, reps, lines)


def part_c(window, reps, lines):
    lines += ["", "(c) reverse_kld(1024) forward + backward, 32 tanh Planar layers, D = 2", "",
              "| target | p | us per call | spread | x the module |", "|---|---|---|---|---|"]
    layers, _, _, _ = pr_ref.inputs("tanh", 2, 32, 1024)
    for family, n in TARGETS:
        def model_with(p):
            flows = [nf.flows.Planar(2, act="tanh", u=q["u"].float(), w=q["w"].float(), b=q["b"].float()) for q in layers]
            model = nf.NormalizingFlow(nf.distributions.DiagGaussian(2), flows, p=p).cuda()

            def call(i):
                model.zero_grad(set_to_none=True)
                model.reverse_kld(1024).backward()
            return call
        ratio_rows("%s %d" % (family, n), {"module": model_with(module_of(family, n)),
                                           "torch restatement": model_with(Restatement(family, n))}, "module", window, reps, lines)


def launches(count=200):
    """What the kernel trace is taken of: every (target, batch, score) launched ``count`` times after a warm-up."""
    for family, n in TARGETS:
        for b in BATCHES:
            for call in kernel_calls(family, n, b).values():
                for i in range(count + 10):
                    call(i)
                torch.cuda.synchronize()


def parse_trace(directory):
    """Median kernel time per (kernel, grid size) from the kernel-trace CSVs under ``directory``."""
    rows = {}
    for path in glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True):
        with open(path, newline="") as f:
            for r in csv.DictReader(f):
                if "target_log_prob_kernel" not in r["Kernel_Name"]:
                    continue
                key = (r["Kernel_Name"], int(r["Grid_Size_X"]) if "Grid_Size_X" in r else int(r["Grid_Size"]))
                rows.setdefault(key, []).append(int(r["End_Timestamp"]) - int(r["Start_Timestamp"]))
    lines = ["| kernel | grid (lanes) | launches | median us | min us |", "|---|---|---|---|---|"]
    for (name, grid), ts in sorted(rows.items()):
        ts = sorted(ts)[:-10] if len(ts) > 20 else ts          # the warm-up launches are the slowest
        lines.append("| `%s` | %d | %d | %.2f | %.2f |" % (name, grid, len(ts), statistics.median(ts) * 1e-3, min(ts) * 1e-3))
    return "\n".join(lines)


def run(window, reps, out):
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    torch.manual_seed(17)
    lines = []
    part_a(window, reps, lines)
    part_b(window, reps, lines)
    part_c(window, reps, lines)
    return bw.finish(lines[1:], window, reps, out)         # every part leads with a blank line; the header brings its own


if __name__ == "__main__":
    ap = bw.parser(0.2)
    ap.add_argument("--launches", action="store_true", help="only launch the kernels (to be traced)")
    ap.add_argument("--parse-trace", default=None, metavar="DIR")
    a = ap.parse_args()
    if a.parse_trace:
        text = parse_trace(a.parse_trace)
        print(text)
        if a.out:
            with open(a.out, "w") as f:
                f.write(text + "\n")
    elif a.launches:
        assert torch.cuda.is_available(), "this measurement needs the GPU"
        launches()
    else:
        run(a.window, a.reps, a.out)
