"""The restatement of the Logit transform (logit_ref.py) pinned in fp64 on the CPU: the two directions undo each other,
both log-dets are those of the Jacobian, the closed-form VJPs that csrc/logit.hip implements are the gradients autograd
finds, alpha = 0 gives the infinities of the formulas without a NaN, and bits per dim matches a number worked by hand."""
import math

import pytest
import torch

import logit_ref as ref
import vcnf_amd as nf


def test_round_trip_fp64():
    torch.manual_seed(0)
    x = torch.rand(4, 3, 5, dtype=torch.float64)
    for alpha in (0.05, 1e-6, 0.3):
        t = ref.LogitRef(alpha)
        z, ld_inv = t.inverse(x)
        back, ld_fwd = t.forward(z)
        assert (back - x).abs().max().item() <= 1e-12
        assert (ld_inv + ld_fwd).abs().max().item() <= 1e-9 * (1 + ld_inv.abs().max().item())


@pytest.mark.parametrize("alpha", [0.05, 1e-6])
def test_log_dets_are_the_jacobians(alpha):
    torch.manual_seed(1)
    t = ref.LogitRef(alpha)
    x = torch.rand(5, 3, dtype=torch.float64) * 0.98 + 0.01
    z = 3 * torch.randn(5, 3, dtype=torch.float64)
    for point, direction in ((x, t.inverse), (z, t.forward)):
        _, ld = direction(point)
        for b in range(len(point)):
            jac = torch.autograd.functional.jacobian(lambda v: direction(v[None])[0][0], point[b])
            sign, logabs = torch.linalg.slogdet(jac)
            assert sign.item() == 1.0
            assert abs(logabs.item() - ld[b].item()) <= 1e-10 * (1 + abs(logabs.item()))


@pytest.mark.parametrize("alpha", [0.05, 1e-6])
def test_closed_form_vjps_match_autograd(alpha):
    torch.manual_seed(2)
    t = ref.LogitRef(alpha)
    x = (torch.rand(4, 3, 5, dtype=torch.float64) * 0.98 + 0.01).requires_grad_()
    z = (3 * torch.randn(4, 3, 5, dtype=torch.float64)).requires_grad_()
    g_out = torch.randn(4, 3, 5, dtype=torch.float64)
    g_ld = torch.randn(4, dtype=torch.float64)
    for point, direction, closed in ((x, t.inverse, ref.inverse_vjp), (z, t.forward, ref.forward_vjp)):
        out, ld = direction(point)
        want, = torch.autograd.grad((out * g_out).sum() + (ld * g_ld).sum(), point)
        got = closed(point.detach(), alpha, g_out, g_ld)
        assert ((got - want).abs() / (1 + want.abs())).max().item() <= 1e-10


def test_alpha_zero_infinities():
    t = ref.LogitRef(0.0)
    for dtype in (torch.float32, torch.float64):
        x = torch.full((3, 4), 0.5, dtype=dtype)
        x[0, 0], x[1, 1], x[2, 0], x[2, 1] = 0.0, 1.0, 0.0, 1.0
        z, ld = t.inverse(x)
        assert not torch.isnan(z).any() and not torch.isnan(ld).any()
        assert z[0, 0] == -math.inf and z[1, 1] == math.inf and z[2, 0] == -math.inf and z[2, 1] == math.inf
        assert torch.isfinite(z).sum().item() == 8
        assert (ld == math.inf).all()
        y, ld = t.forward(torch.tensor([[math.inf, 0.0], [-math.inf, 1.0], [88.0, -104.0]], dtype=dtype))
        assert not torch.isnan(y).any() and not torch.isnan(ld).any()
        assert y[0, 0] == 1.0 and y[1, 0] == 0.0
        assert ld[0] == -math.inf and ld[1] == -math.inf and math.isfinite(ld[2].item())


def test_forward_log_det_is_the_stable_form():
    """logsigmoid(z) + logsigmoid(-z) = -|z| - 2 log1p(exp(-|z|)): what the kernel evaluates."""
    z = torch.tensor([-104.0, -88.0, -3.0, -0.0, 0.0, 1e-3, 7.5, 88.0, 104.0, 700.0], dtype=torch.float64)
    want = torch.nn.functional.logsigmoid(z) + torch.nn.functional.logsigmoid(-z)
    got = -z.abs() - 2 * torch.log1p(torch.exp(-z.abs()))
    assert ((got - want).abs() / (1 + want.abs())).max().item() <= 1e-15


def test_bits_per_dim_by_hand():
    # 3072 dims at log p = -3072 ln 2 nats is 1 bit per dim of the density and 8 bits of the 256 levels
    assert nf.utils.bits_per_dim(-3072 * math.log(2), 3072) == pytest.approx(9.0, abs=1e-12)
    assert ref.bits_per_dim(-3072 * math.log(2), 3072) == pytest.approx(9.0, abs=1e-12)
    lp = torch.tensor([-7000.0, -6500.0], dtype=torch.float64)
    got = nf.utils.bits_per_dim(lp, 3072)
    want = torch.tensor([7000.0 / (3072 * 0.6931471805599453) + 8, 6500.0 / (3072 * 0.6931471805599453) + 8], dtype=torch.float64)
    assert torch.allclose(got, want, rtol=0, atol=1e-12)
    assert nf.utils.bits_per_dim(0.0, 10, levels=32) == pytest.approx(5.0, abs=1e-12)
    # 7000 / (3072 ln 2) = 3.2874...: the number worked by hand
    assert got[0].item() == pytest.approx(11.2874, abs=1e-4)
