"""Device code of two source trees, kernel by kernel, without a GPU (profiles/stream_helpers.md section 1,
profiles/rqs_host.md section 1, profiles/split_half_units.md section 1, profiles/rqs64_unit.md section 2):

    isa_kernel_diff.py PARENT_CSRC NEW_CSRC [--work DIR] [--jobs N] [--reuse] [--renamed OLD=NEW ...] [--mix]

Each unit below is compiled in both trees with the build's own flags plus --cuda-device-only -S.  The two outputs are
cut into kernels, from the kernel's label to its .end_amdhsa_kernel (descriptor block included); the per-function
numbers of local labels (.LBB<n>_, BB<n>_) and runs of blanks are normalised.  Prints one table row per unit and exits
non-zero if a kernel symbol came or went or a kernel differs.

--renamed OLD=NEW (repeatable; OLD a regular expression over mangled symbols, NEW its re.sub replacement) pairs a
parent kernel with the new kernel whose symbol is the parent's with OLD replaced by NEW, and compares them after that
replacement.
--mix adds one row per differing kernel: registers, scratch, LDS and the counts of matrix, LDS, memory and barrier
instructions, parent -> new.
"""
import argparse
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

sys.path[:0] = [os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))]
from vcnf_amd.build import FLAGS as BUILD_FLAGS, UNITS as BUILD_UNITS   # the build's own flags and (source, extra flags, name)s

# the units that include rqs_host.hpp, host_common.hpp, fused_common.hpp or split_half.hpp, directly or through
# rqs_math.hpp / stream_common.hpp, and the units that take a limit or a code from include/vcnf_hip.h
# (profiles/abi_single_source.md section 3)
CHECKED = ("rqs_kernels.hip", "rqs_backward.hip", "rqs_f64.hip", "fused_layer.hip", "fused_final.hip",
           "fused_layer_v6.hip", "fused_layer_v6_pair.hip", "fused_layer_v6s.hip", "affine_kernels.hip",
           "class_cond_gaussian.hip", "gaussian_mixture.hip", "heavy_tail.hip", "conv1x1.hip", "conv3x3_1x1.hip", "linear_f16x3.hip",
           "linear_wgrad.hip", "resnet_trunk.hip", "fused_affine.hip", "gemm_probe.hip", "channel_mix.hip",
           "mvn_base.hip", "planar_radial.hip", "stochastic.hip", "target_density.hip", "vae_ends.hip", "periodic.hip", "logit.hip", "made_sample.hip")
UNITS = sorted(((s, e) for s, e, _ in BUILD_UNITS if s in CHECKED), key=lambda u: CHECKED.index(u[0]))
FLAGS = BUILD_FLAGS + ["--cuda-device-only", "-S"]


def kernels(path):
    """{symbol: normalised text from the symbol's label to its .end_amdhsa_kernel}"""
    lines = open(path).read().split("\n")
    label = {m.group(1): i for i, m in enumerate(re.match(r"([A-Za-z_$][\w$.]*):", l) for l in lines) if m}
    out = {}
    for i, l in enumerate(lines):
        m = re.match(r"\s*\.amdhsa_kernel\s+(\S+)", l)
        if not m:
            continue
        end = next(j for j in range(i, len(lines)) if lines[j].strip() == ".end_amdhsa_kernel")
        text = "\n".join(lines[label[m.group(1)]:end + 1])
        text = re.sub(r"\.LBB\d+_", ".LBBn_", text)
        text = re.sub(r"\bBB\d+_", "BBn_", text)
        out[m.group(1)] = re.sub(r"[ \t]+", " ", text)
    return out


MIX_FIELDS = (".amdhsa_next_free_vgpr", ".amdhsa_next_free_sgpr", ".amdhsa_private_segment_fixed_size",
              ".amdhsa_group_segment_fixed_size")
MIX_PREFIXES = ("v_mfma", "ds_", "global_load", "global_store", "buffer_load", "buffer_store", "s_barrier")


def mix(text):
    """descriptor fields and instruction counts by mnemonic prefix of one kernel's text"""
    words = [l.split() for l in text.split("\n")]
    field = {w[0]: w[1] for w in words if len(w) == 2 and w[0] in MIX_FIELDS}
    return [field.get(f, "?") for f in MIX_FIELDS] + [sum(1 for w in words if w and w[0].startswith(p)) for p in MIX_PREFIXES]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("parent")
    ap.add_argument("new")
    ap.add_argument("--work", default=None)
    ap.add_argument("--jobs", type=int, default=8)
    ap.add_argument("--reuse", action="store_true", help="compare the assembly files already in --work")
    ap.add_argument("--renamed", action="append", default=[], metavar="OLD=NEW")
    ap.add_argument("--mix", action="store_true")
    args = ap.parse_args()
    renamed = [r.split("=", 1) for r in args.renamed]
    work = args.work or tempfile.mkdtemp(prefix="isa_diff_")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

    def compile_one(job):
        tree, side, (src, extra) = job
        out = os.path.join(work, side, os.path.splitext(src)[0] + "".join(extra).replace("=", "") + ".s")
        os.makedirs(os.path.dirname(out), exist_ok=True)
        if not (args.reuse and os.path.exists(out)):
            subprocess.run([hipcc] + FLAGS + extra + [src, "-o", out], cwd=tree, check=True)
        return out

    jobs = [(os.path.abspath(t), side, u) for u in UNITS for t, side in ((args.parent, "parent"), (args.new, "new"))]
    with ThreadPoolExecutor(max_workers=args.jobs) as pool:
        outs = list(pool.map(compile_one, jobs))
    bad = 0
    total = [0, 0, 0]
    mix_rows = []
    print("| unit | kernels at the parent | kept their symbol | identical |\n|---|---|---|---|")
    for k, (src, extra) in enumerate(UNITS):
        a, b = kernels(outs[2 * k]), kernels(outs[2 * k + 1])
        for old, new in renamed:             # a parent kernel takes the new symbol where that pairs it
            for sym in [x for x in a if x not in b and re.sub(old, new, x) in b]:
                a[re.sub(old, new, sym)] = a.pop(sym).replace(sym, re.sub(old, new, sym))
        kept = sorted(set(a) & set(b))
        same = [s for s in kept if a[s] == b[s]]
        for s in sorted(set(a) ^ set(b)):
            print("  symbol only in %s: %s" % ("parent" if s in a else "new", s), file=sys.stderr)
        for s in kept:
            if a[s] != b[s]:
                print("  differs: %s %s" % (src, s), file=sys.stderr)
                if args.mix:
                    mix_rows.append("| `%s` | %s |" % (s, " | ".join(
                        x if x == y else "%s -> %s" % (x, y) for x, y in zip(map(str, mix(a[s])), map(str, mix(b[s]))))))
        bad += len(set(a) ^ set(b)) + len(kept) - len(same)
        total = [total[0] + len(a), total[1] + len(kept), total[2] + len(same)]
        print("| `%s`%s | %d | %d | %d |" % (src, " " + " ".join("`%s`" % e for e in extra) if extra else "",
                                             len(a), len(kept), len(same)))
    print("| total | %d | %d | %d |" % tuple(total))
    if mix_rows:
        heads = [f.replace(".amdhsa_", "") for f in MIX_FIELDS] + [p + "*" for p in MIX_PREFIXES]
        print("\n| kernel | %s |\n|%s" % (" | ".join(heads), "---|" * (len(heads) + 1)))
        print("\n".join(mix_rows))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
