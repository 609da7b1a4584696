"""The binding's launch helpers on the GPU: a failed call names the entry point that was actually called, and the
bench.py event hook sees the fused RQS wrappers as it always did (one bracket per wrapper call, around the first launch
of the range-safe pair, tagged with the batch size)."""
import pytest
import torch

import vcnf_amd as nf
from vcnf_amd import _lib

pytestmark = pytest.mark.gpu


def test_errors_name_the_entry_point_called(hip):
    z = torch.zeros(4, 0, dtype=torch.float64, device=hip)
    row = torch.zeros(0, dtype=torch.float64, device=hip)
    with pytest.raises(nf.VcnfError, match="vcnf_diag_gaussian_log_prob_f64"):       # no features: VCNF_ERR_SHAPE
        _lib.diag_gaussian_log_prob(z, row, row)
    # status 4 (min_bin_width * K > 1) stays the reference's ValueError (splines.py:104-107)
    bad = _lib.make_cfg(8, "linear", min_bin_width=0.2)
    x = torch.zeros(4, device=hip)
    with pytest.raises(ValueError):
        _lib.rqs_elementwise(x, torch.zeros(4, 8, device=hip), torch.zeros(4, 8, device=hip),
                             torch.zeros(4, 7, device=hip), bad, False)


def test_event_sink_sees_one_bracket_per_fused_rqs_call(hip):
    from vcnf_amd import fused as fz
    torch.manual_seed(5)
    flows = [nf.flows.CoupledRationalQuadraticSpline(32, 2, 128) for _ in range(2)]
    one = nf.NormalizingFlow(nf.distributions.DiagGaussian(32), flows[:1]).to(hip).eval()
    two = nf.NormalizingFlow(nf.distributions.DiagGaussian(32), flows).to(hip).eval()
    x = torch.randn(64, 32, device=hip)
    assert fz.eligible(flows[0].prqct, None)
    one.fuse_rqs_stacks, two.fuse_rqs_stacks = False, True
    seen = {}
    for name, model in (("layer", one), ("stack", two)):
        events = []
        _lib.EVENT_SINK = events
        try:
            with torch.no_grad():
                model.log_prob(x)
        finally:
            _lib.EVENT_SINK = None
        seen[name] = events
    torch.cuda.synchronize()
    for name, events in seen.items():
        assert len(events) == 1, (name, [e[2] for e in events])
        start, end, tag = events[0]
        assert tag == 64 and start.elapsed_time(end) >= 0.0, name
