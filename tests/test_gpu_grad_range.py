"""The training path's split-half backward GEMMs at the cotangent scales a mean loss produces.

forward_kld is a mean over the batch: at the benchmark's training batch (131 072) the cotangents that reach
csrc/linear_f16x3.hip (input-gradient form) and csrc/linear_wgrad.hip (linear_wgrad_f16x3_kernel) are of order 2^-17,
below fp16's smallest normal, where a bare hi / lo split keeps few bits (tests/test_split_half_ref.py pins that
arithmetic on the CPU).  The kernels therefore carry the cotangent times a power of two (split_half.hpp::pre_scale),
one per row of the cotangent in an input gradient and one per column in a weight gradient.  Asserted here for
cotangents randn * 2^-k, k in {0, 10, 17, 24, 30}, against fp64 products computed on the device:

  (a) every entry within 4 * 2^-24 * scale of the fp64 result, no absolute term (scale = sum |a b| of the entry's dot
      product, + |addend| where there is one; |dy|^T |x| for dW, sum |dy| for db);
  (b) where B > 1000: mean and p99.9 error of the GEMM not above 1.05x / 1.1x the library fp32 GEMM's on the same
      operands (measured at k = 0 and carried to k by the power of two: fp32 does not move with the scaling).  db is
      a column sum, not a GEMM: its error is printed beside torch's column sum and held to (a);
  (c) the result at k is 2^-k times the result at k = 0, bit for bit;
  (d) nothing clamped: nf.check_saturation() == 0.

``prescale=False`` on the wrappers runs the kernels as they were before the pre-scale; profiles/grad_range.md has both
sets of figures (before: (a) breaks from k = 17 on for the input gradient and from k = 24 on for the weight gradient).

One entry of 1e6 among entries at 2^-17 (a spread of 2^37, more than the 2^29 of full-precision range an exponent
leaves below the largest entry it is taken from) is why the exponent is per row / per column and not per launch: with
one exponent per launch the rows the large entry does not reach were 394 (input gradient) / 166 (weight gradient) ulp
of the scale off (profiles/grad_range.md).
"""
import pytest
import torch

import vcnf_amd as nf
from vcnf_amd import _lib, autograd

import split_half_ref as sh

pytestmark = pytest.mark.gpu

KS = (0, 10, 17, 24, 30)
BOUND = 4 * 2.0 ** -24
_OPS = {}


def _q999(e):
    return float(e.flatten().quantile(0.999))


def dgrad_operands(n_out, n_in, b):
    """g [b, n_out] at 2^0, w [n_out, n_in], mask, addend [b, n_in] (x and w as in test_gpu_gemm_error.py)."""
    key = ("dgrad", n_out, n_in, b)
    if key not in _OPS:
        gen = torch.Generator().manual_seed(7 + n_out + n_in + b)
        _OPS[key] = (torch.randn(b, n_out, generator=gen).cuda(), (torch.randn(n_out, n_in, generator=gen) / n_in ** 0.5).cuda(),
                     torch.randn(b, n_in, generator=gen).cuda(), torch.randn(b, n_in, generator=gen).cuda())
    return _OPS[key]


def dgrad_figures(g, w, mask, addend, k, prescale=None, unit=None):
    """One input-gradient launch on g * 2^-k (addend * 2^-k): result, per-entry error and scale, library's error at k = 0
    carried to k.  ``unit``: this function's return value at k = 0 (its library figures and result are reused)."""
    s = 2.0 ** -k
    gk, ak = g * s, (addend * s if addend is not None else None)
    got = _lib.linear_f16x3(gk, w, None, input_grad=True, mask=mask, addend=ak, prescale=prescale)
    ref = gk.double() @ w.double()
    scale = gk.abs().double() @ w.abs().double()
    if mask is not None:
        keep = (mask > 0).double()
        ref, scale = ref * keep + ak.double(), scale * keep + ak.abs().double()
    err = (got.double() - ref).abs()
    if unit is None:
        lib = g @ w
        if mask is not None:
            lib = lib * (mask > 0) + addend
        e_lib = (lib.double() - ref).abs()
        lib_mean, lib_q = float(e_lib.mean()), (_q999(e_lib) if e_lib.numel() > 1000 else 0.0)
        lib_max = float((e_lib / scale).max())
    else:
        lib_mean, lib_q, lib_max = unit["lib_mean"] * s, unit["lib_q"] * s, unit["lib_max"]
    return {"got": got, "err": err, "scale": scale, "lib_mean": lib_mean, "lib_q": lib_q, "lib_max": lib_max}


def wgrad_operands(n_in, n_out, b):
    key = ("wgrad", n_in, n_out, b)
    if key not in _OPS:
        gen = torch.Generator().manual_seed(n_in + n_out)
        _OPS[key] = (torch.randn(b, n_in, generator=gen).cuda(), torch.randn(b, n_out, generator=gen).cuda())
    return _OPS[key]


def wgrad_figures(x, dy, relu_x, k, prescale=True, unit=None):
    s = 2.0 ** -k
    dyk = dy * s
    dw, db = _lib.linear_wgrad(x, dyk, f16x3=True, relu_x=relu_x, prescale=prescale)
    xe = torch.relu(x) if relu_x else x
    ref_w, ref_b = dyk.double().t() @ xe.double(), dyk.double().sum(0)
    scale_w, scale_b = dyk.abs().double().t() @ xe.abs().double(), dyk.abs().double().sum(0)
    err_w, err_b = (dw.double() - ref_w).abs(), (db.double() - ref_b).abs()
    if unit is None:
        e_lib = ((dy.t() @ xe).double() - ref_w).abs()
        lib_mean, lib_q, lib_max = float(e_lib.mean()), _q999(e_lib), float((e_lib / scale_w).max())
        lib_b = float((dy.sum(0).double() - ref_b).abs().mean())
    else:
        lib_mean, lib_q, lib_max, lib_b = unit["lib_mean"] * s, unit["lib_q"] * s, unit["lib_max"], unit["lib_b"] * s
    return {"got": dw, "got_b": db, "err": err_w, "scale": scale_w, "err_b": err_b, "scale_b": scale_b,
            "lib_mean": lib_mean, "lib_q": lib_q, "lib_max": lib_max, "lib_b": lib_b}


def _line(what, k, f):
    u = f["err"] / f["scale"] / 2.0 ** -24
    return "%s 2^-%d: max %.3g mean %.3g ulp of the scale | mean %.3g p99.9 %.3g x library (library max %.3g)" % (
        what, k, float(u.max()), float(u.mean()), float(f["err"].mean()) / f["lib_mean"] if f["lib_mean"] else 0.0,
        (_q999(f["err"]) / f["lib_q"]) if f["lib_q"] else 0.0, f["lib_max"] / 2.0 ** -24)


def _check(what, k, f, unit, batch):
    print("\n" + _line(what, k, f))
    assert bool((f["err"] <= BOUND * f["scale"]).all()), (what, k, float((f["err"] / f["scale"]).max() / 2.0 ** -24))   # (a)
    if batch > 1000:                                                                                                   # (b)
        assert float(f["err"].mean()) <= 1.05 * f["lib_mean"], (what, k, float(f["err"].mean()), f["lib_mean"])
        assert _q999(f["err"]) <= 1.1 * f["lib_q"], (what, k, _q999(f["err"]), f["lib_q"])
    assert torch.equal(f["got"], unit["got"] * 2.0 ** -k), (what, k)                                                  # (c)


@pytest.mark.parametrize("b", [1, 63, 2577])
@pytest.mark.parametrize("n_out,n_in", [(128, 128), (736, 128)])
def test_input_gradient_at_small_cotangent_scales(hip, n_out, n_in, b):
    g, w, mask, addend = dgrad_operands(n_out, n_in, b)
    nf.check_saturation()
    for what, mk, ad in (("dgrad %dx%d B=%d" % (n_out, n_in, b), None, None), ("dgrad+mask+addend %dx%d B=%d" % (n_out, n_in, b), mask, addend)):
        unit = dgrad_figures(g, w, mk, ad, 0)
        for k in KS:
            _check(what, k, unit if k == 0 else dgrad_figures(g, w, mk, ad, k, unit=unit), unit, b)
    assert nf.check_saturation() == 0                                                                                 # (d)


@pytest.mark.parametrize("relu_x", [False, True])
@pytest.mark.parametrize("n_in,n_out,b", [(128, 128, 16421), (128, 736, 10000), (64, 5, 300)])
def test_weight_gradient_at_small_cotangent_scales(hip, n_in, n_out, b, relu_x):
    x, dy = wgrad_operands(n_in, n_out, b)
    nf.check_saturation()
    what = "wgrad %d->%d B=%d%s" % (n_in, n_out, b, " relu(x)" if relu_x else "")
    unit = wgrad_figures(x, dy, relu_x, 0)
    for k in KS:
        f = unit if k == 0 else wgrad_figures(x, dy, relu_x, k, unit=unit)
        _check(what, k, f, unit, b)
        ub = f["err_b"] / f["scale_b"] / 2.0 ** -24
        print("   db: max %.3g ulp of the scale, mean error %.3g x torch's column sum" % (float(ub.max()), float(f["err_b"].mean()) / max(f["lib_b"], 1e-300)))
        assert bool((f["err_b"] <= BOUND * f["scale_b"]).all()), (what, k, float(ub.max()))
        assert torch.equal(f["got_b"], unit["got_b"] * 2.0 ** -k), (what, k)
    assert nf.check_saturation() == 0


@pytest.mark.parametrize("b,n", [(3, 128), (63, 736), (300, 5), (2577, 128), (70001, 128), (1100, 8192), (1030, 6)])
def test_abs_max_rows_and_columns(hip, b, n):
    """csrc/linear_wgrad.hip::abs_max_rows_cols_kernel, the source of the pre-scale: the largest |value| of every row and
    of every column, equal to torch's - one workgroup and many (70 001 rows of 128: 547 passes of 128 rows over 256
    workgroups, two full trips and a ragged third; 2577 rows of 128: 21 workgroups, one pass each, the last ragged), 16-byte and (n = 5, 6, and a view that starts 4 bytes in) 4-byte loads, the widest row the kernel's LDS
    holds; an all-zero row / column gives 0, a NaN gives NaN in its row and column only (the kernels then do not scale
    them), an infinity likewise; the ticket word is left at zero, so a second launch gives the same."""
    gen = torch.Generator().manual_seed(b + n)
    for first in (0, 1):
        t = torch.randn(b * n + 1, generator=gen).cuda()[first:first + b * n].view(b, n)
        assert t.data_ptr() % 16 == 4 * first
        t[b // 2] = 0.0
        t[:, n // 2] = 0.0
        t[b - 1, n - 1] = -9.25
        for again in range(2):
            rows, cols = _lib.abs_max(t)
            assert torch.equal(rows, t.abs().amax(1)) and torch.equal(cols, t.abs().amax(0)), (first, again)
        assert float(rows[b // 2]) == 0.0 and float(cols[n // 2]) == 0.0 and float(rows[b - 1]) == 9.25 == float(cols[n - 1])
        t[0, 0] = float("nan")
        t[b - 1, n - 2] = float("inf")
        rows, cols = _lib.abs_max(t)
        want_r, want_c = t.abs().amax(1), t.abs().amax(0)
        assert torch.isnan(rows[0]) and torch.isnan(cols[0]) and torch.isinf(rows[b - 1]) and torch.isinf(cols[n - 2])
        assert torch.equal(rows[1:b - 1], want_r[1:b - 1]) and torch.equal(cols[1:n - 2], want_c[1:n - 2])
    scratch = _lib._AMAX_SCRATCH[_lib._stream_key(t.device)]
    assert float(scratch[0]) == 0.0


def _mixed(rows, cols, gen):
    u = torch.randint(-12, 13, (rows, 1), generator=gen).float()
    return (torch.randn(rows, cols, generator=gen) * 2.0 ** -17 * torch.exp2(u)).cuda()


def test_rows_of_mixed_scale(hip):
    """Cotangent rows at 2^-17 * 2^u, u uniform in [-12, 12] per row: a spread of 2^24, inside the 2^29 of
    full-precision range even a single exponent for the whole launch would leave below the largest entry - (a) per entry."""
    gen = torch.Generator().manual_seed(11)
    _, w, _, _ = dgrad_operands(128, 128, 2577)
    g = _mixed(2577, 128, gen)
    f = dgrad_figures(g, w, None, None, 0)
    print("\n" + _line("dgrad mixed rows", 17, f))
    assert bool((f["err"] <= BOUND * f["scale"]).all()), float((f["err"] / f["scale"]).max() / 2.0 ** -24)
    x, _ = wgrad_operands(128, 128, 16421)
    f = wgrad_figures(x, _mixed(16421, 128, gen), False, 0)
    print(_line("wgrad mixed rows", 17, f))
    assert bool((f["err"] <= BOUND * f["scale"]).all()) and bool((f["err_b"] <= BOUND * f["scale_b"]).all())
    assert nf.check_saturation() == 0


def test_zero_cotangent_and_2_to_minus_60(hip):
    g, w, mask, addend = dgrad_operands(128, 128, 63)
    x, dy = wgrad_operands(64, 5, 300)
    nf.check_saturation()
    assert not _lib.linear_f16x3(torch.zeros_like(g), w, None, input_grad=True).any()
    assert not _lib.linear_f16x3(torch.zeros_like(g), w, None, input_grad=True, mask=mask, addend=torch.zeros_like(addend)).any()
    dw, db = _lib.linear_wgrad(x, torch.zeros_like(dy), f16x3=True)
    assert not dw.any() and not db.any()
    s = 2.0 ** -60                                                                                                    # (c) at k = 60
    assert torch.equal(_lib.linear_f16x3(g * s, w, None, input_grad=True), _lib.linear_f16x3(g, w, None, input_grad=True) * s)
    assert torch.equal(_lib.linear_f16x3(g * s, w, None, input_grad=True, mask=mask, addend=addend * s),
                       _lib.linear_f16x3(g, w, None, input_grad=True, mask=mask, addend=addend) * s)
    (dw0, db0), (dwk, dbk) = _lib.linear_wgrad(x, dy, f16x3=True), _lib.linear_wgrad(x, dy * s, f16x3=True)
    assert torch.equal(dwk, dw0 * s) and torch.equal(dbk, db0 * s)
    assert nf.check_saturation() == 0


def test_one_huge_entry_is_not_clamped(hip):
    """One entry of 1e6 among entries at 2^-17: neither clamped nor counted (the pre-scale brings 1e6 to 2^14.9), and
    (a) on every entry - the row (input gradient) / column (weight gradient) that holds the 1e6 has an exponent of its
    own, the others keep theirs."""
    g, w, _, _ = dgrad_operands(128, 128, 63)
    x, dy = wgrad_operands(64, 5, 300)
    g, dy = g * 2.0 ** -17, dy * 2.0 ** -17
    g[5, 3] = 1.0e6
    dy[150, 2] = 1.0e6
    nf.check_saturation()
    fd = dgrad_figures(g, w, None, None, 0)
    fw = wgrad_figures(x, dy, False, 0)
    assert nf.check_saturation() == 0
    assert torch.isfinite(fd["got"]).all() and torch.isfinite(fw["got"]).all()
    # the entries the 1e6 reaches are right to fp32 rounding (clamped at 65504 they would be off by a factor of 15)
    assert bool((fd["err"][5] <= BOUND * fd["scale"][5]).all()) and bool((fw["err"][2] <= BOUND * fw["scale"][2]).all())
    worst = [float((f["err"] / f["scale"]).max() / 2.0 ** -24) for f in (fd, fw)]
    print("\none entry of 1e6 among 2^-17: worst entry %.3g (dgrad) / %.3g (wgrad) ulp of the scale" % tuple(worst))
    assert bool((fd["err"] <= BOUND * fd["scale"]).all()) and bool((fw["err"] <= BOUND * fw["scale"]).all()), worst
    assert bool((fw["err_b"] <= BOUND * fw["scale_b"]).all())


def test_fp16_subnormal_operands_reach_the_matrix_unit(hip):
    """Forward form with x = randn * 2^-14: the lo halves (and most hi halves) are fp16 subnormals.  The emulation
    (subnormals kept) gives at most 2.2 ulp of the scale; a matrix unit that flushed fp16 subnormal inputs would give
    hundreds.  No pre-scale on this form, so this is the bare arithmetic."""
    gen = torch.Generator().manual_seed(5)
    x = (torch.randn(2577, 128, generator=gen) * 2.0 ** -14).cuda()
    w = (torch.randn(128, 128, generator=gen) / 128 ** 0.5).cuda()
    got = _lib.linear_f16x3(x, w, None)
    ref, scale = x.double() @ w.double().t(), x.abs().double() @ w.abs().double().t()
    emu = sh.product(x.cpu(), w.cpu().t().contiguous())
    u = (got.double() - ref).abs() / scale / 2.0 ** -24
    ue = (emu.cuda() - ref).abs() / scale / 2.0 ** -24
    print("\nsubnormal probe, x at 2^-14: device max %.3g mean %.3g ulp of the scale; emulation max %.3g mean %.3g" % (
        float(u.max()), float(u.mean()), float(ue.max()), float(ue.mean())))
    assert float(u.max()) <= 4.0, float(u.max())


def _net_grads(net, x, ctx, up, k):
    old = autograd.WGRAD_MIN_BATCH
    autograd.WGRAD_MIN_BATCH = 8192
    try:
        net.zero_grad(set_to_none=True)
        xi = x.clone().requires_grad_(True)
        events = []
        _lib.EVENT_SINK = events
        try:
            (net(xi, ctx) * up * 2.0 ** -k).sum().backward()
        finally:
            _lib.EVENT_SINK = None
        return [xi.grad] + [p.grad.clone() for p in net.parameters()], [e[2] for e in events]
    finally:
        autograd.WGRAD_MIN_BATCH = old


def test_network_gradients_do_not_depend_on_the_loss_scale(hip):
    """ResidualNet at a training batch, loss = sum(net(x, ctx) * up * 2^-k): the forward pass does not see k (same ReLU
    masks), every backward op is linear in the cotangent and each split-half launch takes its powers of two out exactly,
    so 2^k times every gradient (input and parameters) is the k = 0 gradient bit for bit, k in {17, 30}."""
    torch.manual_seed(3)
    net = nf.nets.ResidualNet(48, 96, 128, context_features=16, num_blocks=2).cuda()
    x, ctx, up = (torch.randn(8192 + 5, n, device="cuda") for n in (48, 16, 96))
    unit, tags = _net_grads(net, x, ctx, up, 0)
    assert tags.count("linear_wgrad") == 1 + 2 * 2 + 2 + 1 and "abs_max" in tags and "linear_f16x3" in tags
    names = ["input"] + [n for n, _ in net.named_parameters()]
    for k in (17, 30):
        got, _ = _net_grads(net, x, ctx, up, k)
        for name, a, b in zip(names, got, unit):
            assert torch.equal(a * 2.0 ** k, b), (k, name, float((a * 2.0 ** k - b).abs().max()), float(b.abs().max()))
    assert nf.check_saturation() == 0
