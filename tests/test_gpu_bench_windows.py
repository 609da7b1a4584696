"""profiles/tools/bench_windows.measure with its own timer, the device events: two variants of one small kernel."""
import os
import sys

import pytest
import torch

from vcnf_amd import _lib

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "tools"))
import bench_windows as bw  # noqa: E402

pytestmark = pytest.mark.gpu


def test_measure_with_device_events(hip):
    torch.manual_seed(3)
    b = 1024
    logp = torch.empty(b, device=hip)

    def variant(d):
        z, loc, log_scale = torch.randn(b, d, device=hip), torch.randn(d, device=hip), 0.3 * torch.randn(d, device=hip)
        return lambda i: _lib.diag_gaussian_log_prob(z, loc, log_scale, logp=logp)

    results, failed = bw.measure({"D = 8": variant(8), "D = 64": variant(64)}, window=0.02, reps=3)
    assert failed == {}
    assert sorted(results) == ["D = 64", "D = 8"]
    for name, r in results.items():
        assert len(r.times) == 3 and all(t > 0.0 for t in r.times), (name, r.times)
        assert min(r.times) <= r.median <= max(r.times), (name, r)
