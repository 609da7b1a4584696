"""The energy densities (vcnf_amd.distributions.prior on csrc/target_density.hip and csrc/stochastic.hip) against what a
user has without them: the plain-torch restatement of the reference's prior.py (tests/energy_ref.py) on the same GPU in
the same process.  TwoModes(2, 0.2), Sinusoidal(0.4, 4), Sinusoidal_gap(0.4, 4), Sinusoidal_split(0.4, 4) and
Smiley(0.2) in fp32:

  (a) the kernel alone, with and without the score, at B = 1024 and 1 048 576: back-to-back launches of
      _lib.target_log_prob between two device events (at the small batch this is the launch rate, not the kernel), and
      with --launches / --parse-trace the kernel's own time from a rocprofv3 kernel trace taken in a run of its own:
          rocprofv3 --kernel-trace --output-format csv -d DIR -- python profiles/tools/energy_targets_bench.py --launches
          python profiles/tools/energy_targets_bench.py --parse-trace DIR
      The share of 8 TB/s counts 12 B per sample without the score and 20 B with it.
  (b) eager p.log_prob(z) forward + backward at B = 1024, Python included, for the module and for the restatement.
  (c) a run of 8 HamiltonianMonteCarlo layers of 5 leapfrog steps at B = 1024, forward and forward + backward: one
      launch, the same layers one by one (one launch each), and the layers' torch composition against the restatement.
  (d) HAIS.sample(1024) at 10 betas: the sampler on the module, and on the restatement with a plain-torch walk.

Timing: the protocol of bench_windows.py, the variants of one row group alternated; the row forms are
target_density_bench.py's.

    python profiles/tools/energy_targets_bench.py [--window 0.2] [--reps 5] [--out FILE]
"""
import torch

import bench_windows as bw         # first: it puts the repository root and tests/ on sys.path
import energy_ref as eref
import target_density_bench as tdb
import vcnf_amd as nf
from vcnf_amd import _lib, fused_stochastic

CASES = eref.FAMILIES
BATCHES = (1024, 1 << 20)
LAYERS, STEPS, STEP = 8, 5, 0.05
BETAS = 10


def kernel_calls(case, b):
    prior = eref.prior_of(case)
    z = tdb._z(b)
    table, scale = prior._operands(z)
    return {want: (lambda i, want=want: _lib.target_log_prob(z, prior._family, table, scale, want_score=want))
            for want in (False, True)}


def part_a(window, reps, lines):
    lines += ["", "(a) back-to-back launches of the kernel wrapper", "",
              "| density | B | score | us per call | spread | GB/s | of 8 TB/s |", "|---|---|---|---|---|---|---|"]
    for case in CASES:
        for b in BATCHES:
            tdb.kernel_rows(eref.case_id(case), b, kernel_calls(case, b), window, reps, lines)


def part_b(window, reps, lines):
    lines += ["", "(b) log_prob forward + backward at B = 1024, eager", "",
              "| density | variant | us per call | spread | x the module |", "|---|---|---|---|---|"]
    z = tdb._z(1024)
    for case in CASES:
        def fwd_bwd(p):
            def call(i):
                x = z.detach().requires_grad_(True)
                torch.autograd.grad(p.log_prob(x).sum(), x)
            return call
        tdb.ratio_rows(eref.case_id(case), {"module (one launch + one multiply)": fwd_bwd(eref.prior_of(case)),
                                            "torch restatement": fwd_bwd(eref.PlainEnergy(case))},
                       "module (one launch + one multiply)", window, reps, lines)


def hmc_flows(target):
    params = eref.hmc_parameters(STEP, LAYERS)
    return [nf.flows.HamiltonianMonteCarlo(target, STEPS, ls.float(), lm.float()).cuda() for ls, lm in params]


def part_c(window, reps, lines):
    z = tdb._z(1024)
    for backward in (False, True):
        lines += ["", "(c) %d HMC layers of %d steps at B = 1024, %s" % (LAYERS, STEPS, "forward + backward" if backward else "forward"), "",
                  "| density | variant | us per call | spread | x one launch |", "|---|---|---|---|---|"]
        for case in CASES:
            def walk(flows, fused):
                def call(i):
                    with torch.set_grad_enabled(backward):
                        x = z.detach().requires_grad_(backward)
                        if fused:
                            out, ld = fused_stochastic.run(flows, x, None, 1.0)
                        else:
                            out, ld = x, 0.0
                            for flow in flows:
                                out, one = flow(out)
                                ld = ld + one
                        if backward:
                            for flow in flows:
                                flow.zero_grad(set_to_none=True)
                            (out.sum() + ld.sum()).backward()
                return call
            kernel, plain = hmc_flows(eref.prior_of(case)), hmc_flows(eref.PlainEnergy(case))
            tdb.ratio_rows(eref.case_id(case), {"one launch": walk(kernel, True), "layer by layer": walk(kernel, False),
                                                "torch composition": walk(plain, False)}, "one launch", window, reps, lines)


def part_d(window, reps, lines):
    lines += ["", "(d) HAIS.sample(1024) at %d betas, %d leapfrog steps" % (BETAS, STEPS), "",
              "| density | variant | us per call | spread | x one launch |", "|---|---|---|---|---|"]
    prior = nf.distributions.DiagGaussian(2, trainable=False).cuda()
    step_size = torch.tensor([STEP, 1.2 * STEP], device="cuda")
    log_mass = torch.tensor([0.1, -0.2], device="cuda")
    for case in CASES:
        def sampler(target, fuse=True):
            s = nf.sampling.HAIS(torch.linspace(1, 0, BETAS + 1), prior, target, STEPS, step_size, log_mass, fuse=fuse)

            def call(i):
                with torch.no_grad():
                    s.sample(1024)
            return call
        tdb.ratio_rows(eref.case_id(case), {"one launch": sampler(eref.prior_of(case)), "layer by layer": sampler(eref.prior_of(case), False),
                                            "torch composition": sampler(eref.PlainEnergy(case))}, "one launch", window, reps, lines)


def launches(count=200):
    """What the kernel trace is taken of: every (density, batch, score) launched ``count`` times after a warm-up."""
    for case in CASES:
        for b in BATCHES:
            for call in kernel_calls(case, b).values():
                for i in range(count + 10):
                    call(i)
                torch.cuda.synchronize()


def run(window, reps, out):
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    torch.manual_seed(17)
    lines = []
    for part in (part_a, part_b, part_c, part_d):
        part(window, reps, lines)
    return bw.finish(lines[1:], window, reps, out)         # every part leads with a blank line; the header brings its own


if __name__ == "__main__":
    ap = bw.parser(0.2)
    ap.add_argument("--launches", action="store_true", help="only launch the kernels (to be traced)")
    ap.add_argument("--parse-trace", default=None, metavar="DIR")
    a = ap.parse_args()
    if a.parse_trace:
        text = tdb.parse_trace(a.parse_trace)
        print(text)
        if a.out:
            with open(a.out, "w") as f:
                f.write(text + "\n")
    elif a.launches:
        assert torch.cuda.is_available(), "this measurement needs the GPU"
        launches()
    else:
        run(a.window, a.reps, a.out)
