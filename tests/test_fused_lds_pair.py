"""LdsV6Pair of csrc/fused_lds.hpp on its own (no GPU, no HIP): tests/c_host/fused_lds_pair_check.cpp is compiled with
g++ (plain C++17) and run as a child process.  For every shape of the fused RQS layer family it checks that the regions
of the two-layer kernel's LDS layout are ordered and do not overlap, that the byte count is the one-layer layout's plus
one table set, the figure of config C3, and that the layout fits a workgroup's 163 840 bytes exactly for the shapes
``vcnf_rqs_pair_fused_supported`` accepts."""
import os
import subprocess

import vcnf_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_fused_lds_pair_layout_and_query(tmp_path):
    exe = str(tmp_path / "fused_lds_pair_check")
    cmd = ["g++", "-std=c++17", "-O2", "-I", os.path.join(ROOT, "vcnf_amd", "csrc"),
           os.path.join(ROOT, "tests", "c_host", "fused_lds_pair_check.cpp"), "-o", exe]
    done = subprocess.run(cmd, capture_output=True, text=True)
    assert done.returncode == 0, done.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0, (run.returncode, run.stdout, run.stderr)
    assert "fused_lds_pair_check ok (12 instances, 11 with the pair form)" in run.stdout
    rows = [tuple(int(v) for v in l.split()[1:]) for l in run.stdout.splitlines() if l.startswith("pair ")]
    assert len(rows) == 12
    lib = vcnf_amd.lib()
    for di, c, nblk, nbytes, fits in rows:
        assert fits == int(nbytes <= 163840)
        assert lib.vcnf_rqs_pair_fused_supported(di, di, c, 128, nblk) == fits, (di, c, nblk)
    assert (32, 16, 2, 163696, 1) in rows and (32, 16, 3) in [r[:3] for r in rows if not r[4]]
    # outside the family, or another hidden width: no pair form
    assert lib.vcnf_rqs_pair_fused_supported(32, 32, 16, 64, 2) == 0
    assert lib.vcnf_rqs_pair_fused_supported(24, 24, 0, 128, 2) == 0
    assert lib.vcnf_rqs_pair_fused_supported(32, 16, 0, 128, 2) == 0
    assert lib.vcnf_rqs_pair_fused_supported(32, 32, 16, 128, 4) == 0
