"""Categorical dequantisation on the HIP kernels (csrc/dequant.hip): prepare, merge with both kinds of noise, the merge
VJP and quantize against the plain-torch restatement (varquant_ref.py), then the model container and a training step.

The error rule.  With ref64 the fp64 restatement on the inputs the kernel sees (fp32 inputs are the rounded fp64 ones) and
s its own s, per categorical element and per row

    cond = 1/s + 1/(1 - s)
    |out - ref64| <= C eps (1 + |ref64| + cond)
    |ld  - ref64| <= C eps (1 + sum_c (|log s| + |log(1 - s)| + |logsigmoid(w) + logsigmoid(-w)| + log K_c) + sum_c cond)

with C = 4 in fp32 and C = 8 in fp64.  A flat tolerance would be vacuous or false at the top category of the 1000-level
column, where 1 - s is about 1e-5.  Every figure is printed before it is asserted (``VARQUANT`` lines): the kernel's
ratio to the rule with C = 1, and the fp32 restatement's own ratio on this device."""
import copy
import functools
import re

import pytest
import torch

import grid_caps as gc
import varquant_ref as ref
import vcnf_amd as nf
from vcnf_amd import _lib, autograd

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.float64]
EPS = {torch.float32: torch.finfo(torch.float32).eps, torch.float64: torch.finfo(torch.float64).eps}
FACTOR = {torch.float32: 4.0, torch.float64: 8.0}
CASES = ref.cases()
PLANTED = [104.0, -104.0, -104.0, 104.0, 88.0, -88.0, 17.0, -17.0]      # rows 0 - 3 hold the codes K - 1, 0, K - 1, 0
# (case, alpha): every shape at 1e-5, the Adult and the wide levels at 0.05 too, alpha = 0 in one case
CASE_ALPHAS = [(name, 1e-5) for name in CASES] + [("adult", 0.05), ("wide", 0.05), ("lane_per_row", 0.05), ("adult", 0.0)]


def _ids(v):
    return str(v).replace("torch.", "")


@functools.lru_cache(maxsize=None)
def inputs(name):
    """(x, u, n, w) in fp64 on the CPU: rows, uniform draws with a row of zeros, noise in [0.05, 0.95], logit noise 4 randn
    with the planted values in its first rows."""
    b, d, columns, levels = CASES[name]
    x = ref.rows(b, d, columns, levels, 1)
    g = torch.Generator().manual_seed(2)
    u = torch.rand(b, len(columns), dtype=torch.float64, generator=g)
    if b > 1:
        u[1] = 0.0
    n = 0.05 + 0.9 * torch.rand(b, len(columns), dtype=torch.float64, generator=g)
    w = 4 * torch.randn(b, len(columns), dtype=torch.float64, generator=g)
    for r, v in enumerate(PLANTED[:b]):
        w[r] = v
    return x, u, n, w


def on_device(name, dtype):
    b, d, columns, levels = CASES[name]
    return (columns, levels) + tuple(t.to(dtype).cuda() for t in inputs(name))


def tables(x, columns, levels):
    return _lib.column_tables(columns, levels, x.shape[1], x.device)


def check(got, r32, r64, scale, dtype, what, exact_nonfinite=False):
    """|got - r64| <= C eps scale over the entries where r64 and scale are finite; elsewhere (alpha = 0) the entries are
    the fp32 restatement's, with its values.  Prints the kernel's and the fp32 restatement's ratio to eps scale."""
    got, r32, r64, scale = (t.detach().double().cpu() for t in (got, r32, r64, scale))
    assert got.shape == r64.shape, "%s: shape %s vs %s" % (what, tuple(got.shape), tuple(r64.shape))
    assert not bool(torch.isnan(got).any()), what + ": NaN"
    if not got.numel():
        return
    ok = torch.isfinite(r64) & torch.isfinite(scale) & torch.isfinite(r32)
    if exact_nonfinite:
        same = r32 if dtype == torch.float32 else r64          # the restatement in the kernel's own type
        assert torch.equal(torch.isfinite(got), torch.isfinite(same)), what + ": the entries that are not finite differ"
        assert torch.equal(got[~torch.isfinite(same)], same[~torch.isfinite(same)]), what + ": infinities differ"
    else:
        assert bool(ok.all()) and bool(torch.isfinite(got).all()), what + ": not finite"
    unit = EPS[dtype] * scale[ok]
    mine, its = ((got[ok] - r64[ok]).abs() / unit).max().item(), ((r32[ok] - r64[ok]).abs() / EPS[torch.float32] / scale[ok]).max().item()
    print("VARQUANT %-58s %s  kernel %.3f of eps x scale (allowed %g)  fp32 restatement %.3f" % (
        what, _ids(dtype), mine, FACTOR[dtype], its))
    assert mine <= FACTOR[dtype], "%s: %.3f x eps x scale, allowed %g" % (what, mine, FACTOR[dtype])


def spread(per_column, columns, like):
    """[B, C] values in their columns of a [B, D] tensor of zeros."""
    out = torch.zeros_like(like)
    out[:, columns] = per_column
    return out


# ---------------------------------------------------------------- prepare and merge
@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
@pytest.mark.parametrize("name, alpha", CASE_ALPHAS)
def test_prepare_against_the_restatement(hip, name, alpha, dtype):
    columns, levels, x, u, n, w = on_device(name, dtype)
    slot, lv = tables(x, columns, levels)
    v, ctx, ld = _lib.dequant_prepare(x, slot, lv, u, alpha)
    v2, ctx2, ld2 = _lib.dequant_prepare(x, slot, lv, u, alpha)
    assert torch.equal(v, v2) and torch.equal(ctx, ctx2) and torch.equal(ld, ld2), "two calls give the same bits"
    assert v.shape == u.shape and ctx.shape == u.shape and ld.shape == (len(x),) and ld.dtype == dtype
    v64, ctx64, ld64 = ref.prepare(x.double(), columns, levels, u.double(), alpha)
    v32, ctx32, ld32 = ref.prepare(x.float(), columns, levels, u.float(), alpha)
    assert torch.equal(ctx, ref.prepare(x, columns, levels, u, alpha)[1]), "ctx has the restatement's bits"
    s = alpha / 2 + (1 - alpha) * u.double()
    cond = 1 / s + 1 / (1 - s)
    mags = torch.log(s).abs() + torch.log(1 - s).abs() + abs(torch.log1p(torch.tensor(-alpha)).item())
    check(v, v32, v64, 1 + v64.abs() + cond, dtype, "prepare v %s alpha %g" % (name, alpha), alpha == 0)
    check(ld, ld32, ld64, 1 + mags.sum(1) + cond.sum(1), dtype, "prepare ld %s alpha %g" % (name, alpha), alpha == 0)
    if len(x):
        # the accumulating form is the out-of-place result and one add
        for sign in (1.0, -1.0):
            log_q0 = torch.linspace(-3, 3, len(x), dtype=dtype, device="cuda")
            log_q = log_q0.clone()
            got = _lib.dequant_prepare(x, slot, lv, u, alpha, logdet=log_q, sign=sign)[2]
            assert got is log_q and torch.equal(log_q, log_q0 + sign * ld)


@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
@pytest.mark.parametrize("logit", [True, False], ids=["variational", "uniform"])
@pytest.mark.parametrize("name, alpha", CASE_ALPHAS)
def test_merge_against_the_restatement(hip, name, alpha, logit, dtype):
    columns, levels, x, u, n, w = on_device(name, dtype)
    if not logit:
        w = u                                    # the noise itself, its row of zeros included
    slot, lv = tables(x, columns, levels)
    out, ld = _lib.dequant_merge(x, slot, lv, w, logit, alpha)
    out2, ld2 = _lib.dequant_merge(x, slot, lv, w, logit, alpha)
    assert torch.equal(out, out2) and torch.equal(ld, ld2), "two calls give the same bits"
    assert out.shape == x.shape and out.dtype == dtype and ld.shape == (len(x),) and ld.dtype == dtype
    out64, ld64 = ref.merge(x.double(), columns, levels, w.double(), logit, alpha)
    out32, ld32 = ref.merge(x.float(), columns, levels, w.float(), logit, alpha)
    rest = [c for c in range(x.shape[1]) if c not in columns]
    assert torch.equal(out[:, rest], x[:, rest]), "continuous columns are the input's, bit for bit"
    s = ref.merge_s(x.double(), columns, levels, w.double(), logit, alpha)
    cond = 1 / s + 1 / (1 - s)
    mags, cond_sum = ref.merge_terms(x.double(), columns, levels, w.double(), logit, alpha)
    what = "merge %s %s alpha %g" % ("variational" if logit else "uniform", name, alpha)
    check(out[:, columns], out32[:, columns], out64[:, columns], 1 + out64[:, columns].abs() + cond, dtype, what + " out",
          alpha == 0)
    check(ld, ld32, ld64, 1 + mags + cond_sum, dtype, what + " ld", alpha == 0)
    if len(x):
        for sign in (1.0, -1.0):
            log_q0 = torch.linspace(-3, 3, len(x), dtype=dtype, device="cuda")
            log_q = log_q0.clone()
            got, got_ld = _lib.dequant_merge(x, slot, lv, w, logit, alpha, logdet=log_q, sign=sign)
            assert got_ld is log_q and torch.equal(got, out)
            if alpha:
                assert torch.equal(log_q, log_q0 + sign * ld)


def _shifted(t):
    """The same values behind a pointer that only allows scalar accesses."""
    s = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)[1:].view(t.shape)
    s.copy_(t)
    assert s.is_contiguous() and (s.data_ptr() % 16 != 0 or not t.numel())
    return s


@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
@pytest.mark.parametrize("name", ["sixteen", "long_rows", "adult"])
def test_the_access_width_does_not_show_in_the_bits(hip, name, dtype):
    """The same rows behind a pointer that only allows scalar accesses give the bits of the packs (D = 16: 16-byte packs
    in both types; D = 14 and D = 130: 8-byte packs in fp32, 16-byte packs in fp64)."""
    if name == "sixteen":
        columns, levels = [0, 5, 6, 15], [3, 4, 1, 50]
        x = ref.rows(37, 16, columns, levels, 11).to(dtype).cuda()
        g = torch.Generator().manual_seed(12)
        u = torch.rand(37, 4, dtype=torch.float64, generator=g).to(dtype).cuda()
        w = (4 * torch.randn(37, 4, dtype=torch.float64, generator=g)).to(dtype).cuda()
    else:
        columns, levels, x, u, n, w = on_device(name, dtype)
    slot, lv = tables(x, columns, levels)
    xs = _shifted(x)
    for a, b in zip(_lib.dequant_prepare(x, slot, lv, u, 0.05), _lib.dequant_prepare(xs, slot, lv, u, 0.05)):
        assert torch.equal(a, b)
    for logit, noise in ((True, w), (False, u)):
        for a, b in zip(_lib.dequant_merge(x, slot, lv, noise, logit, 0.05), _lib.dequant_merge(xs, slot, lv, noise, logit, 0.05)):
            assert torch.equal(a, b) and bool(torch.isfinite(a).all())
        g_out, g_ld = torch.randn_like(x), torch.randn(len(x), dtype=dtype, device="cuda")
        for a, b in zip(_lib.dequant_merge_bwd(x, slot, lv, noise, logit, 0.05, g_out, g_ld, want_x=True),
                        _lib.dequant_merge_bwd(xs, slot, lv, noise, logit, 0.05, _shifted(g_out), g_ld, want_x=True)):
            assert torch.equal(a, b) and bool(torch.isfinite(a).all())
    z = _lib.dequant_merge(x, slot, lv, w, True, 0.05)[0]
    for a, b in zip(_lib.quantize(z, slot, lv, 0.05), _lib.quantize(_shifted(z), slot, lv, 0.05)):
        assert torch.equal(a, b)


# ---------------------------------------------------------------- past the grid cap
def grid_cap():
    """The unit's cap on its workgroups and its block size, read from the source as tests/grid_caps.py reads the others."""
    src = gc.source("dequant.hip")
    found = {k: re.findall(gc._constexpr(k), src) for k in ("kMaxBlocks", "kBlock")}
    assert all(len(v) == 1 for v in found.values()), found
    return gc._value(found["kMaxBlocks"][0]), gc._value(found["kBlock"][0])


@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
def test_a_batch_past_the_grid_cap(hip, dtype):
    """B = 2 cap x block + block / 2 + 1 rows of 3 columns: with one lane per row (fp32) every workgroup makes two full
    trips and a ragged third, with two lanes per row (fp64) four and a ragged fifth.  The rows of the last trips and the
    rows across the first boundary, run again as batches of their own, give the same bits."""
    cap, block = grid_cap()
    d, columns, levels = 3, [1], [5]
    lanes = gc.pick_lanes(-(-d // (2 if dtype == torch.float64 else 4)))
    assert lanes == (2 if dtype == torch.float64 else 1)
    b = 2 * cap * block + block // 2 + 1
    assert -(-b // (block // lanes)) > 2 * cap and b * d <= gc.MAX_ELEMENTS
    g = torch.Generator(device="cuda").manual_seed(3)
    x = torch.randn(b, d, dtype=dtype, device="cuda", generator=g)
    x[:, 1] = torch.randint(0, 5, (b,), device="cuda", generator=g).to(dtype)
    w = 4 * torch.randn(b, 1, dtype=dtype, device="cuda", generator=g)
    u = torch.rand(b, 1, dtype=dtype, device="cuda", generator=g)
    slot, lv = tables(x, columns, levels)
    out, ld = _lib.dequant_merge(x, slot, lv, w, True, 1e-5)
    v, ctx, ld_p = _lib.dequant_prepare(x, slot, lv, u, 1e-5)
    codes, ld_q = _lib.quantize(out, slot, lv, 1e-5)
    g_out, g_ld = torch.randn_like(x), torch.randn(b, dtype=dtype, device="cuda")
    d_w, d_x = _lib.dequant_merge_bwd(x, slot, lv, w, True, 1e-5, g_out, g_ld, want_x=True)
    trip = cap * (block // lanes)
    for lo, hi in ((b - trip - 300, b), (trip - gc.STRADDLE // 2, trip + gc.STRADDLE // 2 + 1), (0, 64)):
        xs, ws, us = x[lo:hi].contiguous(), w[lo:hi].contiguous(), u[lo:hi].contiguous()
        a, a_ld = _lib.dequant_merge(xs, slot, lv, ws, True, 1e-5)
        assert torch.equal(a, out[lo:hi]) and torch.equal(a_ld, ld[lo:hi]), (lo, hi)
        for p, q in zip(_lib.dequant_prepare(xs, slot, lv, us, 1e-5), (v[lo:hi], ctx[lo:hi], ld_p[lo:hi])):
            assert torch.equal(p, q), (lo, hi)
        for p, q in zip(_lib.quantize(a, slot, lv, 1e-5), (codes[lo:hi], ld_q[lo:hi])):
            assert torch.equal(p, q), (lo, hi)
        for p, q in zip(_lib.dequant_merge_bwd(xs, slot, lv, ws, True, 1e-5, g_out[lo:hi].contiguous(), g_ld[lo:hi].contiguous(),
                                               want_x=True), (d_w[lo:hi], d_x[lo:hi])):
            assert torch.equal(p, q), (lo, hi)
    # every row against the restatement on the device
    out64, ld64 = ref.merge(x.double(), columns, levels, w.double(), True, 1e-5)
    out32, ld32 = ref.merge(x.float(), columns, levels, w.float(), True, 1e-5)
    mags, cond_sum = ref.merge_terms(x.double(), columns, levels, w.double(), True, 1e-5)
    assert torch.equal(out[:, [0, 2]], x[:, [0, 2]])
    check(out[:, 1], out32[:, 1], out64[:, 1], 1 + out64[:, 1].abs() + cond_sum, dtype, "past the cap: merge out")
    check(ld, ld32, ld64, 1 + mags + cond_sum, dtype, "past the cap: merge ld")
    # codes come back wherever the noise is not within rounding of a level's edge
    inner = (torch.sigmoid(w[:, 0]) > 0.05) & (torch.sigmoid(w[:, 0]) < 0.95)
    assert torch.equal(codes[inner], x[inner]) and int(inner.sum()) > b // 4
    assert torch.equal(d_x[:, [0, 2]], g_out[:, [0, 2]]) and not bool(d_x[:, 1].any()) and bool(torch.isfinite(d_w).all())


# ---------------------------------------------------------------- the merge VJP
def _ref_grads(x, columns, levels, w, logit, alpha, g_out, g_ld, dtype):
    w = w.detach().to(dtype).clone().requires_grad_()
    out, ld = ref.merge(x.to(dtype), columns, levels, w, logit, alpha)
    grad, = torch.autograd.grad((out * g_out.to(dtype)).sum() + (ld * g_ld.to(dtype)).sum(), w)
    return grad.double()


@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
@pytest.mark.parametrize("logit", [True, False], ids=["variational", "uniform"])
@pytest.mark.parametrize("name, alpha", [(n, a) for n, a in CASE_ALPHAS if a > 0])
def test_merge_vjp_against_the_restatements_autograd(hip, name, alpha, logit, dtype):
    columns, levels, x, u, n, w = on_device(name, dtype)
    if not logit:
        w = n
    slot, lv = tables(x, columns, levels)
    g = torch.Generator(device="cuda").manual_seed(4)
    g_out = torch.randn(x.shape, dtype=torch.float64, device="cuda", generator=g).to(dtype)
    g_ld = torch.randn(len(x), dtype=torch.float64, device="cuda", generator=g).to(dtype)
    d_w, d_x = _lib.dequant_merge_bwd(x, slot, lv, w, logit, alpha, g_out, g_ld, want_x=True)
    assert d_w.shape == w.shape and d_w.dtype == dtype and d_x.shape == x.shape
    again = _lib.dequant_merge_bwd(x, slot, lv, w, logit, alpha, g_out, g_ld, want_x=True)
    assert torch.equal(d_w, again[0]) and torch.equal(d_x, again[1])
    rest = [c for c in range(x.shape[1]) if c not in columns]
    assert torch.equal(d_x[:, rest], g_out[:, rest]) and not bool(d_x[:, columns].any())
    assert _lib.dequant_merge_bwd(x, slot, lv, w, logit, alpha, g_out, g_ld)[1] is None
    if not len(x):
        return
    g64 = _ref_grads(x, columns, levels, w, logit, alpha, g_out, g_ld, torch.float64)
    g32 = _ref_grads(x, columns, levels, w, logit, alpha, g_out, g_ld, torch.float32)
    scale = EPS[dtype] / EPS[torch.float32]
    for j in range(len(columns)):
        measure = (g32[:, j] - g64[:, j]).abs().max().item()
        top = g64[:, j].abs().max().item()
        err = (d_w[:, j].double() - g64[:, j]).abs()
        bound = 4 * scale * measure + 8 * EPS[dtype] * (1 + g64[:, j].abs())
        worst = int((err - bound).argmax())
        print("VARQUANT merge VJP %s %s alpha %g %s column %d (K = %d): err %.3e bound %.3e  fp32 restatement's error %.3e of max |g| %.3e" % (
            "variational" if logit else "uniform", name, alpha, _ids(dtype), columns[j], levels[j], err[worst].item(),
            bound[worst].item(), measure, top))
        assert measure <= 1e-2 * top, "the fp32 restatement's own error leaves the bound empty"
        assert bool((err <= bound).all())
    if logit:
        # n (1 - n) = 0 at w = +-104: what is left is g_ld (1 - 2 n)
        for r, v in enumerate(PLANTED[:min(4, len(x))]):
            want = -g_ld[r] if v > 0 else g_ld[r]
            assert bool((d_w[r] == want).all()), "row %d, w = %g" % (r, v)
    # either cotangent may be missing
    zeros_out, zeros_ld = torch.zeros_like(g_out), torch.zeros_like(g_ld)
    assert torch.equal(_lib.dequant_merge_bwd(x, slot, lv, w, logit, alpha, None, g_ld)[0],
                       _lib.dequant_merge_bwd(x, slot, lv, w, logit, alpha, zeros_out, g_ld)[0])
    only_out = _lib.dequant_merge_bwd(x, slot, lv, w, logit, alpha, g_out, None, want_x=True)
    with_zero = _lib.dequant_merge_bwd(x, slot, lv, w, logit, alpha, g_out, zeros_ld, want_x=True)
    assert torch.equal(only_out[0], with_zero[0]) and torch.equal(only_out[1], with_zero[1])


class _Launches:
    """Names and arguments of the entry points called while it is active."""

    def __init__(self, monkeypatch):
        self.calls = []
        inner = _lib._launch

        def launch(name, *args):
            self.calls.append((name, args))
            return inner(name, *args)
        monkeypatch.setattr(_lib, "_launch", launch)

    def names(self):
        return [n for n, _ in self.calls]


@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
def test_the_merge_node(hip, dtype, monkeypatch):
    """One node: forward one launch, backward one launch whichever cotangents arrive, none when neither does."""
    sfx = "_f64" if dtype == torch.float64 else "_f32"
    columns, levels, x, u, n, w = on_device("adult", dtype)
    slot, lv = tables(x, columns, levels)
    seen = _Launches(monkeypatch)
    for used in ("both", "out", "ld"):
        leaf = w.clone().requires_grad_()
        del seen.calls[:]
        out, ld = autograd.DequantMergeFn.apply(x, leaf, slot, lv, True, 0.05)
        assert seen.names() == ["vcnf_dequant_merge" + sfx]
        g_out, g_ld = torch.randn_like(out), torch.randn_like(ld)
        loss = ((out * g_out).sum() if used != "ld" else 0) + ((ld * g_ld).sum() if used != "out" else 0)
        loss.backward()
        assert seen.names()[1:] == ["vcnf_dequant_merge_bwd" + sfx]
        want = _lib.dequant_merge_bwd(x, slot, lv, w, True, 0.05, g_out if used != "ld" else None, g_ld if used != "out" else None)[0]
        assert torch.equal(leaf.grad, want), used

    class Ctx:
        saved_tensors = (x, w, slot, lv)
        args = (True, 0.05)
        needs_input_grad = (False, True, False, False, False, False)
    del seen.calls[:]
    assert autograd.DequantMergeFn.backward(Ctx(), None, None) == (None,) * 6 and seen.names() == []
    # the raw wrappers refuse a tensor that requires grad
    with pytest.raises(NotImplementedError):
        _lib.dequant_merge(x, slot, lv, w.clone().requires_grad_(), True, 0.05)
    with pytest.raises(NotImplementedError):
        _lib.quantize(x.clone().requires_grad_(), slot, lv, 0.05)
    # a row that asks for its gradient gets the cotangent through its continuous columns
    rows = x.clone().requires_grad_()
    out, ld = autograd.DequantMergeFn.apply(rows, w, slot, lv, True, 0.05)
    g_out = torch.randn_like(out)
    (out * g_out).sum().backward()
    rest = [c for c in range(x.shape[1]) if c not in columns]
    assert torch.equal(rows.grad[:, rest], g_out[:, rest]) and not bool(rows.grad[:, columns].any())


def test_gradcheck_through_the_merge_node(hip):
    columns, levels, x, u, n, w = on_device("one_of_three", torch.float64)
    slot, lv = tables(x, columns, levels)
    w = torch.randn(len(x), 1, dtype=torch.float64, device="cuda", generator=torch.Generator(device="cuda").manual_seed(5))
    for logit, point in ((True, w), (False, n)):
        assert torch.autograd.gradcheck(lambda t: autograd.DequantMergeFn.apply(x, t, slot, lv, logit, 0.05),
                                        (point.clone().requires_grad_(),), nondet_tol=0.0)


# ---------------------------------------------------------------- quantize
@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
@pytest.mark.parametrize("alpha", [1e-5, 0.05], ids=_ids)
@pytest.mark.parametrize("name", list(CASES))
def test_quantize_returns_the_codes(hip, name, alpha, dtype):
    columns, levels, x, u, n, w = on_device(name, dtype)
    slot, lv = tables(x, columns, levels)
    z = _lib.dequant_merge(x, slot, lv, n, False, alpha)[0]
    codes, ld = _lib.quantize(z, slot, lv, alpha)
    assert torch.equal(codes, x), "every code and every continuous column, no entry left out"
    again = _lib.quantize(z, slot, lv, alpha)
    assert torch.equal(codes, again[0]) and torch.equal(ld, again[1])
    t = z[:, columns].double()
    ld64 = ref.quantize(z.double(), columns, levels, alpha)[1]
    ld32 = ref.quantize(z.float(), columns, levels, alpha)[1]
    lsg = torch.nn.functional.logsigmoid(t) + torch.nn.functional.logsigmoid(-t)
    mags = (lsg.abs() + abs(torch.log1p(torch.tensor(-alpha)).item()) + torch.log(ref.level_row(levels, t))).sum(1)
    got, r32, r64, scale = (v.double().cpu() for v in (ld, ld32, ld64, 1 + mags))
    if len(x):
        ratio = ((got - r64).abs() / (EPS[dtype] * scale)).max().item()
        print("VARQUANT quantize ld %s alpha %g %s: kernel %.3f of eps x sum of magnitudes (allowed 4)  fp32 restatement %.3f" % (
            name, alpha, _ids(dtype), ratio, ((r32 - r64).abs() / (EPS[torch.float32] * scale)).max().item()))
        assert ratio <= 4.0
        for sign in (1.0, -1.0):
            log_q0 = torch.linspace(-3, 3, len(x), dtype=dtype, device="cuda")
            log_q = log_q0.clone()
            got_codes, got_ld = _lib.quantize(z, slot, lv, alpha, logdet=log_q, sign=sign)
            assert got_ld is log_q and torch.equal(got_codes, codes) and torch.equal(log_q, log_q0 + sign * ld)
        far = z.clone()
        far[0::2, :], far[1::2, :] = 104.0, -104.0
        top = far.clone()
        top[:, columns] = (ref.level_row(levels, x) - 1).expand(len(x), -1).clone()
        top[1::2, columns] = 0.0
        far_codes, far_ld = _lib.quantize(far, slot, lv, alpha)
        assert torch.equal(far_codes, top) and bool(torch.isfinite(far_ld).all())


# ---------------------------------------------------------------- the model container
COLUMNS, LEVELS = [0, 2, 5], [3, 2, 7]


def _model(dtype, variational=True, seed=6):
    torch.manual_seed(seed)
    flows = [nf.flows.CoupledRationalQuadraticSpline(6, 1, 16) for _ in range(2)]
    var_flows = [nf.flows.CoupledRationalQuadraticSpline(3, 1, 16, num_context_channels=3) for _ in range(2)]
    for p in [q for f in flows + var_flows for q in f.parameters()]:
        torch.nn.init.normal_(p.data, std=0.3) if p.dim() > 1 else torch.nn.init.normal_(p.data, std=0.1)
    q0 = nf.distributions.DiagGaussian(6, trainable=False)
    model = nf.NormalizingFlow(q0, flows, categoricals=COLUMNS, catlevels=LEVELS,
                               catvdeqs=nf.nets.VariationalDequantization(var_flows) if variational else None)
    plain = nf.NormalizingFlow(q0, flows)
    return model.to("cuda", dtype), plain.to("cuda", dtype)


def _model_rows(dtype):
    x = ref.rows(33, 6, COLUMNS, LEVELS, 7).to(dtype).cuda()
    u = torch.rand(33, 3, dtype=torch.float64, generator=torch.Generator().manual_seed(8)).to(dtype).cuda()
    return x, u


@pytest.mark.parametrize("variational", [True, False], ids=["variational", "uniform"])
@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
def test_model_log_prob_is_the_plain_model_on_the_dequantised_rows(hip, dtype, variational, monkeypatch):
    model, plain = _model(dtype, variational)
    x, u = _model_rows(dtype)
    eps = EPS[dtype]
    with torch.no_grad():
        xt, ld = model.dequantize(x, noise=u)
        got = model.log_prob(x, noise=u)
        inner = plain.log_prob(xt)
        _, _, lds, _ = plain.forward_kld(xt, extended=True)
        mags = ld.abs() + sum(torch.as_tensor(l).to(ld).abs() for l in lds) + inner.abs() + 1
        err = (got - (inner + ld)).abs()
        print("VARQUANT model.log_prob %s %s: max err / (eps x magnitudes) %.3f (allowed 4)" % (
            "variational" if variational else "uniform", _ids(dtype), (err / (eps * mags)).max().item()))
        assert bool((err <= 4 * eps * mags).all()) and bool(torch.isfinite(got).all())
        assert torch.equal(model.forward_kld(x, noise=u), -torch.mean(got))
        assert model.categoricals == COLUMNS and plain.categoricals is None
        # drawn noise: one seed, one value
        torch.manual_seed(9)
        first = model.log_prob(x)
        torch.manual_seed(9)
        assert torch.equal(first, model.log_prob(x)) and not torch.equal(first, model.log_prob(x))
        # the uniform class is ONE launch; the variational one is prepare, its flows' run, merge
        seen = _Launches(monkeypatch)
        model.dequantize(x, noise=u)
        sfx = "_f64" if dtype == torch.float64 else "_f32"
        if variational:
            assert seen.names()[0] == "vcnf_dequant_prepare" + sfx and seen.names()[-1] == "vcnf_dequant_merge" + sfx
            assert sum("dequant" in name for name in seen.names()) == 2
            fused = len(seen.names())
            model.catvdeqs.fuse_rqs_stacks = False
            del seen.calls[:]
            xt2, ld2 = model.dequantize(x, noise=u)
            print("VARQUANT dequantize launches: %d with the flows' run fused, %d without" % (fused, len(seen.names())))
            assert fused <= len(seen.names())
            model.catvdeqs.fuse_rqs_stacks = True
            # the same kernels' values added in another order: the terms are prepare's, each flow's and merge's
            slot, lv = tables(x, COLUMNS, LEVELS)
            w, ctx, part = _lib.dequant_prepare(x, slot, lv, u, model.catvdeqs.alpha)
            terms = part.abs() + 1
            for flow in model.catvdeqs.flows:
                w, part = flow(w, context=ctx)
                terms = terms + part.abs()
            terms = terms + _lib.dequant_merge(x, slot, lv, w.contiguous(), True, model.catvdeqs.alpha)[1].abs()
            err = (ld2 - ld).abs()
            print("VARQUANT fuse_rqs_stacks off: ld max err / (eps x magnitudes) %.3f (allowed 4), rows equal: %s" % (
                (err / (eps * terms)).max().item(), torch.equal(xt2, xt)))
            assert bool((err <= 4 * eps * terms).all()) and torch.equal(xt2, xt)
        else:
            assert seen.names() == ["vcnf_dequant_merge" + sfx]


@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
def test_model_samples_are_codes(hip, dtype):
    model, plain = _model(dtype)
    noise = torch.randn(33, 6, dtype=torch.float64, generator=torch.Generator().manual_seed(10)).to(dtype).cuda()
    with torch.no_grad():
        z, log_q = model.sample_from(noise)
        z0, log_q0 = plain.sample_from(noise)
        codes, ld = model.quantize(z0)
    rest = [c for c in range(6) if c not in COLUMNS]
    assert torch.equal(z[:, rest], z0[:, rest]) and torch.equal(z, codes)
    cat = z[:, COLUMNS]
    assert torch.equal(cat, cat.round()) and bool((cat >= 0).all()) and bool((cat <= ref.level_row(LEVELS, cat) - 1).all())
    assert torch.equal(log_q, log_q0 - ld)
    with torch.no_grad():
        z, log_q = model.sample(17)
    assert z.shape == (17, 6) and torch.equal(z[:, COLUMNS], z[:, COLUMNS].round()) and bool(torch.isfinite(log_q).all())


# ---------------------------------------------------------------- training
def _grads(model, x, u):
    model.zero_grad(set_to_none=True)
    loss = model.forward_kld(x, noise=u)
    loss.backward(retain_graph=True)
    first = {k: p.grad.clone() for k, p in model.named_parameters() if p.requires_grad}
    model.zero_grad(set_to_none=True)
    loss.backward()
    second = {k: p.grad.clone() for k, p in model.named_parameters() if p.requires_grad}
    return first, second


@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
def test_training_step_reaches_the_dequantisers_flows(hip, dtype):
    model, _ = _model(dtype)
    x, u = _model_rows(dtype)
    kernel, again = _grads(model, x, u)
    assert any(k.startswith("catvdeqs.flows.") for k in kernel) and any(k.startswith("flows.") for k in kernel)
    for k in kernel:
        assert bool(torch.isfinite(kernel[k]).all()), k
        assert torch.equal(kernel[k], again[k]), k + ": a second backward through the retained graph"
    assert any(bool(g.any()) for k, g in kernel.items() if k.startswith("catvdeqs.flows."))
    # the same model with the dequantiser's torch composition in place of the kernels, in fp32 and in fp64
    twin32, twin64 = copy.deepcopy(model).float(), copy.deepcopy(model).double()
    twin32.catvdeqs.use_kernels = twin64.catvdeqs.use_kernels = False
    comp32, _ = _grads(twin32, x.float(), u.float())
    comp64, _ = _grads(twin64, x.double(), u.double())
    scale = EPS[dtype] / EPS[torch.float32]
    for k in kernel:
        g = comp64[k]
        err = (kernel[k].double() - g).abs().max().item()
        measure = (comp32[k].double() - g).abs().max().item()
        bound = 4 * scale * measure + 8 * EPS[dtype] * (1 + g.abs().max().item())
        print("VARQUANT training %s %-44s err %.3e  bound %.3e  composition fp32 vs fp64 %.3e  max |g| %.3e" % (
            _ids(dtype), k, err, bound, measure, g.abs().max().item()))
        assert err <= bound, k
