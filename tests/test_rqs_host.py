"""csrc/rqs_host.hpp on its own (no GPU, no HIP): tests/c_host/rqs_host_check.cpp is compiled with g++ (plain C++17)
and run as a child process.  It checks the bin-count dispatcher over its three lists, the spline constants of one
configuration and the number of derivative logits."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_host_header_dispatch_and_constants(tmp_path):
    exe = str(tmp_path / "rqs_host_check")
    cmd = ["g++", "-std=c++17", "-O2", "-I", os.path.join(ROOT, "vcnf_amd", "csrc"),
           os.path.join(ROOT, "tests", "c_host", "rqs_host_check.cpp"), "-lm", "-o", exe]
    done = subprocess.run(cmd, capture_output=True, text=True)
    assert done.returncode == 0, done.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0, (run.returncode, run.stdout, run.stderr)
    assert "rqs_host_check ok" in run.stdout
