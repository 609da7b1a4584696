"""csrc/fused_lds.hpp on its own (no GPU, no HIP): tests/c_host/fused_lds_check.cpp is compiled with g++ (plain C++17)
and run as a child process.  For every instance of the three fused RQS layer kernels it checks that the layout's byte
count equals the formula the launchers carried before the header existed, and that the regions are ordered and do not
overlap."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_fused_lds_layouts(tmp_path):
    exe = str(tmp_path / "fused_lds_check")
    cmd = ["g++", "-std=c++17", "-O2", "-I", os.path.join(ROOT, "vcnf_amd", "csrc"),
           os.path.join(ROOT, "tests", "c_host", "fused_lds_check.cpp"), "-o", exe]
    done = subprocess.run(cmd, capture_output=True, text=True)
    assert done.returncode == 0, done.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0, (run.returncode, run.stdout, run.stderr)
    assert "fused_lds_check ok (12 instances x 3 layouts)" in run.stdout
