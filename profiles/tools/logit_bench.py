"""The Logit transform and the byte ingest against what a user has without them, on the same GPU in the same process:
the plain-torch restatement of normflow 1.2's transforms.Logit and of the bytes -> jitter -> scale chain
(tests/logit_ref.py, run on the device tensors).  In fp32:

* ``Logit.inverse``, ``Logit.forward`` and ``Logit.inverse_u8`` (noise supplied, and drawn by the call) at
  (1024, 3, 32, 32) and (16384, 3, 32, 32);
* the bare library calls ``_lib.logit`` and ``_lib.logit_inverse_u8`` at those shapes: their bytes (every element read
  once and written once; for the bytes 1 + 4 read and 4 written per element) over the time per call as a share of the
  8 TB/s peak.  The wrappers allocate their outputs, so the time holds torch's allocator as well;
* ``log_prob`` of a small multiscale Glow (3 x 8 x 8, two levels, one GlowBlock each, hidden 16) at 1024 images without
  a transform, with the Logit and with the restatement in its place, and from bytes.

Everything is eager, Python included, under no_grad.  Timing: the protocol of bench_windows.py, the variants of one
group alternated.

    python profiles/tools/logit_bench.py [--window 0.2] [--reps 5] [--out FILE]
"""
import torch

import bench_windows as bw         # first: it puts the repository root and tests/ on sys.path
import logit_ref as ref
import vcnf_amd as nf
from vcnf_amd import _lib


def _transform_groups(b):
    """group name -> ({variant: call}, bytes the bare call moves or None)"""
    shape = (b, 3, 32, 32)
    n = b * 3 * 32 * 32
    x = torch.rand(shape, device="cuda")
    z = 4 * torch.randn(shape, device="cuda")
    x_u8 = torch.randint(256, shape, device="cuda").to(torch.uint8)
    noise = torch.rand(shape, device="cuda")
    mine, twin = nf.transforms.Logit(0.05), ref.LogitRef(0.05)
    return {
        "Logit.inverse": ({"kernel": lambda i: mine.inverse(x), "torch restatement": lambda i: twin.inverse(x)}, None),
        "Logit.forward": ({"kernel": lambda i: mine.forward(z), "torch restatement": lambda i: twin.forward(z)}, None),
        "Logit.inverse_u8, noise given": ({"kernel": lambda i: mine.inverse_u8(x_u8, noise),
                                           "torch restatement": lambda i: ref.inverse_u8(x_u8, noise, 0.05)}, None),
        "Logit.inverse_u8, noise drawn": ({"kernel": lambda i: mine.inverse_u8(x_u8),
                                           "torch restatement": lambda i: ref.inverse_u8(x_u8, torch.rand(shape, device="cuda"), 0.05)}, None),
        "bare vcnf_logit_inverse": ({"kernel": lambda i: _lib.logit(x, 0.05, True)}, (2 * n + b) * 4),
        "bare vcnf_logit_forward": ({"kernel": lambda i: _lib.logit(z, 0.05, False)}, (2 * n + b) * 4),
        "bare vcnf_logit_inverse_u8": ({"kernel": lambda i: _lib.logit_inverse_u8(x_u8, noise, 1 / 256., 255 / 256., 0.05)}, 9 * n + 4 * b),
    }


def _model_group(b):
    torch.manual_seed(21)
    levels, hidden, inp = 2, 16, (3, 8, 8)
    merges, flows, shapes = [], [], []
    for i in range(levels):
        flows += [[nf.flows.GlowBlock(inp[0] * 2 ** (levels + 1 - i), hidden, split_mode="channel", scale=True), nf.flows.Squeeze()]]
        if i > 0:
            merges += [nf.flows.Merge()]
            shapes += [(inp[0] * 2 ** (levels - i), inp[1] // 2 ** (levels - i), inp[2] // 2 ** (levels - i))]
        else:
            shapes += [(inp[0] * 2 ** (levels + 1), inp[1] // 2 ** levels, inp[2] // 2 ** levels)]
    q0 = [nf.distributions.GlowBase(s, 4) for s in shapes]
    plain, mine, twin = [nf.MultiscaleFlow(q0, flows, merges, transform=t, class_cond=True).cuda().eval()
                         for t in (None, nf.transforms.Logit(0.05), ref.LogitRef(0.05))]
    x_u8 = torch.randint(256, (b,) + inp, device="cuda").to(torch.uint8)
    x = ref.bytes_to_unit(x_u8, torch.rand(x_u8.shape, device="cuda"))
    z = ref.LogitRef(0.05).inverse(x)[0]
    y = torch.randint(4, (b,), device="cuda")
    plain.log_prob(z, y)              # the ActNorms take their statistics from this batch
    for m in (plain, mine, twin):
        m.refresh_packed()
    return {"small Glow log_prob": ({"kernel": lambda i: mine.log_prob(x, y), "torch restatement": lambda i: twin.log_prob(x, y),
                                     "no transform": lambda i: plain.log_prob(z, y), "kernel, from bytes": lambda i: mine.log_prob(x_u8, y)}, None)}


def run(window, reps, out):
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    lines = ["| B | item | call | variant | us per call | spread | x the kernel path | share of 8 TB/s |", "|---|---|---|---|---|---|---|---|"]
    torch.manual_seed(17)
    with torch.no_grad():
        for b, item in ((1024, "3x32x32"), (16384, "3x32x32"), (1024, "3x8x8")):
            groups = _transform_groups(b) if item == "3x32x32" else _model_group(b)
            for group, (variants, nbytes) in groups.items():
                results, failed = bw.measure(variants, window, reps)
                for name in variants:
                    lead = "| %d | %s | %s | %s |" % (b, item, group, name)
                    base = results.get("kernel")
                    if name in failed:
                        lines.append("%s failed: %s | | | |" % (lead, failed[name]))
                    else:
                        med, spread, _ = results[name]
                        lines.append("%s %.1f | %.3f | %s | %s |" % (
                            lead, med * 1e6, spread, "%.2f" % (med / base.median) if base else "",
                            "%.1f %%" % (100 * nbytes / med / bw.HBM_PEAK) if nbytes else ""))
                    print(lines[-1], flush=True)
            del groups
            torch.cuda.empty_cache()
    return bw.finish(lines, window, reps, out)


if __name__ == "__main__":
    a = bw.parser(0.2).parse_args()
    run(a.window, a.reps, a.out)
