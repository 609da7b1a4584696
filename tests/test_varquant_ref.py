"""The plain-torch restatement of categorical dequantisation (varquant_ref.py) pinned against autograd, in fp64 on the
CPU: the log-det of merge is the sum of the elementwise log-derivatives, quantize undoes merge on the codes, the two
log-dets cancel up to the noise term, and continuous columns come through bit for bit."""
import math

import pytest
import torch

import varquant_ref as ref

CASES = {k: v for k, v in ref.cases().items() if v[0] > 0}


def _inputs(name, seed=0):
    b, d, columns, levels = CASES[name]
    x = ref.rows(b, d, columns, levels, seed)
    gen = torch.Generator().manual_seed(seed + 100)
    n = 0.05 + 0.9 * torch.rand(b, len(columns), generator=gen, dtype=torch.float64)
    w = 4 * torch.randn(b, len(columns), generator=gen, dtype=torch.float64)
    return x, columns, levels, n, w


@pytest.mark.parametrize("alpha", [1e-5, 0.05])
@pytest.mark.parametrize("name", list(CASES))
def test_merge_log_det_is_the_sum_of_the_elementwise_log_derivatives(name, alpha):
    x, columns, levels, n, w = _inputs(name)
    # uniform: d out / d n per element
    n = n.clone().requires_grad_()
    out, ld = ref.merge(x, columns, levels, n, False, alpha)
    grad, = torch.autograd.grad(out[:, columns].sum(), n)
    want = torch.log(grad.abs()).sum(1)
    assert (ld - want).abs().max().item() <= 1e-10 * (1 + want.abs().max().item())
    # variational: the same through n = sigmoid(w), plus log sigmoid'(w)
    w = w.clone().requires_grad_()
    out, ld = ref.merge(x, columns, levels, w, True, alpha)
    grad, = torch.autograd.grad(out[:, columns].sum(), w)          # = d out / d n * sigmoid'(w)
    want = torch.log(grad.abs()).sum(1)
    assert (ld - want).abs().max().item() <= 1e-10 * (1 + want.abs().max().item())
    sig, = torch.autograd.grad(torch.sigmoid(w).sum(), w)
    noise_term = torch.log(sig).sum(1)
    pure, _ = ref.merge(x, columns, levels, torch.sigmoid(w.detach()), False, alpha)
    assert torch.equal(pure, out.detach())
    ld_uniform = ref.merge(x, columns, levels, torch.sigmoid(w.detach()), False, alpha)[1]
    assert (ld.detach() - (ld_uniform + noise_term)).abs().max().item() <= 1e-10 * (1 + ld.abs().max().item())


@pytest.mark.parametrize("alpha", [1e-5, 0.05, 0.0])
@pytest.mark.parametrize("name", list(CASES))
def test_quantize_returns_the_codes_and_the_log_dets_cancel(name, alpha):
    x, columns, levels, n, _ = _inputs(name, 1)
    out, ld = ref.merge(x, columns, levels, n, False, alpha)
    back, ld_q = ref.quantize(out, columns, levels, alpha)
    assert torch.equal(back, x), "codes and continuous columns"
    # merge's log-det is that of n -> out, quantize's that of out -> y K = k + n: they cancel
    assert (ld + ld_q).abs().max().item() <= 1e-10 * (1 + ld.abs().max().item())
    # in fp32 too, the 1000-level column included: no tie band is needed
    out32, _ = ref.merge(x.float(), columns, levels, n.float(), False, alpha)
    assert torch.equal(ref.quantize(out32, columns, levels, alpha)[0], x.float())


@pytest.mark.parametrize("name", list(CASES))
def test_continuous_columns_come_back_bit_for_bit(name):
    x, columns, levels, n, w = _inputs(name, 2)
    rest = [c for c in range(x.shape[1]) if c not in columns]
    for out in (ref.merge(x, columns, levels, n, False)[0], ref.merge(x, columns, levels, w, True)[0],
                ref.quantize(x, columns, levels)[0]):
        assert torch.equal(out[:, rest], x[:, rest])
    assert ref.merge(x, columns, levels, n, False)[0] is not x


def test_prepare_is_the_logit_of_the_draws_and_the_scaled_codes():
    x, columns, levels, n, _ = _inputs("wide", 3)
    u = n.clone().requires_grad_()
    v, ctx, ld = ref.prepare(x, columns, levels, u, 0.05)
    grad, = torch.autograd.grad(v.sum(), u)
    assert (ld - torch.log(grad).sum(1)).abs().max().item() <= 1e-10
    k = x[:, columns]
    for j, big_k in enumerate(levels):
        if big_k == 1:
            assert torch.equal(ctx[:, j], torch.zeros(len(x), dtype=torch.float64))
        else:
            assert ctx[:, j].min().item() == -1.0 and ctx[:, j].max().item() == 1.0      # rows 0 - 3 hold 0 and K - 1
            assert torch.equal(ctx[:, j], 2 * k[:, j] / (big_k - 1) - 1)
    s = 0.05 / 2 + 0.95 * n
    assert torch.equal(v.detach(), torch.log(s) - torch.log(1 - s))


def test_edges_alpha_zero_and_far_logits():
    columns, levels = [0], [3]
    x = torch.tensor([[2.0], [0.0], [2.0], [0.0]], dtype=torch.float64)
    w = torch.tensor([[104.0], [-104.0], [-104.0], [104.0]]).double()
    for dtype in (torch.float64, torch.float32):
        out, ld = ref.merge(x.to(dtype), columns, levels, w.to(dtype), True, 1e-5)
        assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(ld).all())
        codes, _ = ref.quantize(w.to(dtype), columns, levels, 1e-5)
        assert codes[:, 0].tolist() == [2.0, 0.0, 0.0, 2.0]
    out, ld = ref.merge(x.float(), columns, levels, w.float(), True, 0.0)
    assert not bool(torch.isnan(out).any()) and not bool(torch.isnan(ld).any())
    assert out[0, 0].item() == math.inf and out[1, 0].item() == -math.inf and ld[0].item() == math.inf
    v, _, ld = ref.prepare(x.float(), columns, levels, torch.zeros(4, 1), 0.0)
    assert bool((v == -math.inf).all()) and bool((ld == math.inf).all())
