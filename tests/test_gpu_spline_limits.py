"""Tensor interval limits of the functional spline (splines.py:99-102): ``rational_quadratic_spline`` with tensor
``left / right / bottom / top`` on vcnf_rqs_elementwise_limits_* and its VJP vcnf_rqs_elementwise_limits_bwd_*,
forward and inverse, fp32 and fp64, against the oracle's tensor branch (oracle/rqs.py::_partition) run on the CPU in
fp32 and fp64 on the same inputs.

Bounds: values in fp32 as the other spline kernels (max|y - y64| <= 1e-4 + 8 x the oracle's own fp32 error on the same
inputs, test_gpu_grad.py), fp32 gradients through test_gpu_grad.close (the oracle's fp32 gradients as the noise
yardstick, at most 2e-3 of the elements outside - the bin-boundary cap); fp64 values within 1e-10, fp64 gradients
through test_gpu_f64_grad.tight (every element).  Broadcast layouts: bitwise the full-shape call's values, reduced
limit gradients within m u sum|terms| of the sum of the full-shape call's per-element gradients (summation in any
order: m terms, unit roundoff u)."""
import pytest
import torch

import vcnf_amd as nf
from vcnf_amd import _lib
from vcnf_amd.utils import splines
from oracle import rqs as orqs
from test_gpu_grad import close
from test_gpu_f64_grad import tight

pytestmark = pytest.mark.gpu

GRAD_NAMES = ("g_x", "g_uw", "g_uh", "g_ud", "g_left", "g_right", "g_bottom", "g_top")


def _limits(shape, g, dtype):
    """left ~ U(-3, -1), right = left + U(0.5, 4); bottom, top drawn the same way."""
    out = []
    for _ in range(2):
        lo = torch.rand(shape, generator=g, dtype=torch.float64) * 2 - 3
        hi = lo + 0.5 + 3.5 * torch.rand(shape, generator=g, dtype=torch.float64)
        out += [lo.to(dtype), hi.to(dtype)]
    return out


def _problem(k, shape, dtype, inverse, seed, lim_shape=None):
    """Inputs lo + (hi - lo) U(0.001, 0.999) on the direction's own interval, logits N(0, 1.5^2), random cotangents.
    ``lim_shape``: shape of the four limit tensors (default: the inputs' shape)."""
    g = torch.Generator().manual_seed(seed)
    shape = tuple(shape)
    lims = _limits(shape if lim_shape is None else lim_shape, g, dtype)
    lo, hi = (lims[2], lims[3]) if inverse else (lims[0], lims[1])
    u = torch.rand(shape, generator=g, dtype=torch.float64) * 0.998 + 0.001
    x = (lo.double() + (hi.double() - lo.double()) * u).to(dtype)
    uw, uh, ud = (torch.randn(shape + (m,), generator=g, dtype=torch.float64).mul(1.5).to(dtype) for m in (k, k, k + 1))
    gy, gl = (torch.randn(shape, generator=g, dtype=torch.float64).to(dtype) for _ in range(2))
    return x, uw, uh, ud, lims, gy, gl


def _oracle(x, uw, uh, ud, lims, gy, gl, inverse, dtype, grads=True):
    leaves = [t.detach().to(dtype).clone().requires_grad_(grads) for t in (x, uw, uh, ud, *lims)]
    with torch.set_grad_enabled(grads):
        y, lad = orqs.rq_spline(*leaves[:4], inverse=inverse, left=leaves[4], right=leaves[5], bottom=leaves[6],
                                top=leaves[7])
    if not grads:
        return y, lad, None
    return y.detach(), lad.detach(), torch.autograd.grad([y, lad], leaves, [gy.to(dtype), gl.to(dtype)])


def _hip(x, uw, uh, ud, lims, gy, gl, inverse, grads=True, check=True):
    """(y, lad, gradients of the 8 inputs) of the build; limits on the device unless they are 0-dim host tensors."""
    dl = [t.cuda() for t in (x, uw, uh, ud)] + [t if (t.dim() == 0 and not t.is_cuda) else t.cuda() for t in lims]
    dl = [t.detach().requires_grad_(grads) for t in dl]
    with torch.set_grad_enabled(grads):
        y, lad = splines.rational_quadratic_spline(*dl[:4], inverse=inverse, left=dl[4], right=dl[5], bottom=dl[6],
                                                   top=dl[7])
    if inverse and check:
        _lib.check_discriminant()
    if not grads:
        assert not y.requires_grad
        return y, lad, None
    assert y.requires_grad and lad.requires_grad
    return y.detach(), lad.detach(), torch.autograd.grad([y, lad], dl, [gy.cuda(), gl.cuda()])


def _maxerr(a, b):
    return float((a.detach().cpu().double() - b.detach().cpu().double()).abs().max())


# ---------------------------------------------------------------- 1. values, fp32, per-element limits
@pytest.mark.parametrize("inverse", [False, True])
@pytest.mark.parametrize("k", [5, 8, 10, 16])
def test_values_f32_per_element_limits(hip, k, inverse):
    prob = _problem(k, (20480,), torch.float32, inverse, seed=1000 + k)
    y64, lad64, _ = _oracle(*prob, inverse, torch.float64, grads=False)
    y32, lad32, _ = _oracle(*prob, inverse, torch.float32, grads=False)
    y, lad, _ = _hip(*prob, inverse, grads=False)
    assert y.dtype == torch.float32 and y.shape == (20480,)
    for what, got, r64, r32 in (("y", y, y64, y32), ("logabsdet", lad, lad64, lad32)):
        noise = _maxerr(r32, r64)
        err = _maxerr(got, r64)
        print("K=%d inverse=%s %s: max err %.3e, oracle fp32 noise %.3e" % (k, inverse, what, err, noise))
        assert err <= 1e-4 + 8 * noise, (what, err, noise)


# ---------------------------------------------------------------- 2. gradients, fp32
@pytest.mark.parametrize("inverse", [False, True])
@pytest.mark.parametrize("k", [5, 8, 10, 16])
def test_gradients_f32_per_element_limits(hip, k, inverse):
    prob = _problem(k, (20480,), torch.float32, inverse, seed=1000 + k)
    _, _, want64 = _oracle(*prob, inverse, torch.float64)
    _, _, want32 = _oracle(*prob, inverse, torch.float32)
    _, _, got = _hip(*prob, inverse)
    for a, b, b32, nm in zip(got, want64, want32, GRAD_NAMES):
        assert a.dtype == torch.float32
        close(a, b, "%s K=%d inverse=%s" % (nm, k, inverse), want32=b32)


# ---------------------------------------------------------------- 3. fp64
@pytest.mark.parametrize("inverse", [False, True])
@pytest.mark.parametrize("k", [5, 8, 10, 16])
def test_values_and_gradients_f64_per_element_limits(hip, k, inverse):
    prob = _problem(k, (20480,), torch.float64, inverse, seed=2000 + k)
    y64, lad64, want = _oracle(*prob, inverse, torch.float64)
    y, lad, got = _hip(*prob, inverse)
    assert y.dtype == torch.float64
    for what, a, b in (("y", y, y64), ("logabsdet", lad, lad64)):
        err = _maxerr(a, b)
        print("K=%d inverse=%s %s: max err %.3e" % (k, inverse, what, err))
        assert err <= 1e-10, (what, err)
    for a, b, nm in zip(got, want, GRAD_NAMES):
        tight(a, b, "%s K=%d inverse=%s" % (nm, k, inverse))


# ---------------------------------------------------------------- 4. broadcast layouts
# (inputs' shape, shape of the four limits, (period, inner) the wrapper must read them in place with)
LAYOUTS = [
    ((64, 48), (48,), (48, 1)),                 # [D] against [B, D]
    ((64, 48), (64, 1), (64, 48)),              # [B, 1]
    ((64, 48), (), (1, 1)),                     # 0-dim
    ((16, 3, 8, 10), (3, 1, 1), (3, 80)),       # [C, 1, 1] against [B, C, H, W]
    ((16, 3, 8, 10), (8, 10), (80, 1)),         # [H, W] against [B, C, H, W]
]


@pytest.mark.parametrize("inverse", [False, True])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("layout", LAYOUTS, ids=lambda l: "%s-vs-%s" % (list(l[1]), list(l[0])))
def test_broadcast_layouts_match_the_full_shape_call(hip, layout, dtype, inverse):
    shape, lshape, in_place = layout
    k = 8
    prob = _problem(k, shape, dtype, inverse, seed=3000, lim_shape=lshape)
    x, uw, uh, ud, lims, gy, gl = prob
    for t in lims:
        assert _lib.limit_layout(t, shape)[1:] == in_place       # read in place, nothing materialised
    full = [t.expand(shape).contiguous() for t in lims]
    y, lad, got = _hip(x, uw, uh, ud, lims, gy, gl, inverse)
    yf, ladf, gotf = _hip(x, uw, uh, ud, full, gy, gl, inverse)
    assert torch.equal(y, yf) and torch.equal(lad, ladf)
    for a, b, nm in zip(got[:4], gotf[:4], GRAD_NAMES):
        assert torch.equal(a, b), nm
    u = torch.finfo(dtype).eps / 2
    for a, b, t, nm in zip(got[4:], gotf[4:], lims, GRAD_NAMES[4:]):
        assert a.shape == t.shape and a.dtype == dtype, nm
        terms = b.detach().cpu().double()
        want = terms.sum_to_size(t.shape)
        m = terms.numel() // max(1, t.numel())
        bound = m * u * terms.abs().sum_to_size(t.shape)
        err = (a.detach().cpu().double() - want).abs()
        print("%s %s %s inverse=%s: max err %.3e, max bound %.3e" % (nm, list(lshape), dtype, inverse,
                                                                    float(err.max()), float(bound.max())))
        assert bool((err <= bound).all()), (nm, float(err.max()), float(bound.max()))


def test_zero_dim_host_limits(hip):
    """0-dim host tensors mix with device tensors as in torch; their gradients come back on the host."""
    k, shape = 8, (32, 16)
    for dtype in (torch.float32, torch.float64):
        x, uw, uh, ud, lims, gy, gl = _problem(k, shape, dtype, False, seed=77, lim_shape=())
        y, lad, got = _hip(x, uw, uh, ud, lims, gy, gl, False)
        yd, ladd, gotd = _hip(x, uw, uh, ud, [t.cuda() for t in lims], gy, gl, False)
        assert torch.equal(y, yd) and torch.equal(lad, ladd)
        for a, b in zip(got[4:], gotd[4:]):
            assert a.device.type == "cpu" and a.shape == () and torch.equal(a, b.cpu())


# ---------------------------------------------------------------- 5. consistency with the scalar path
@pytest.mark.parametrize("inverse", [False, True])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("k", [5, 8])
def test_exact_limits_match_the_scalar_path_bitwise(hip, k, dtype, inverse):
    lo_x, hi_x, lo_y, hi_y = -3.0, 3.0, -2.5, 1.5
    n = 4096
    g = torch.Generator().manual_seed(5000 + k)
    lo, hi = (lo_y, hi_y) if inverse else (lo_x, hi_x)
    x = lo + (hi - lo) * torch.rand(n, generator=g, dtype=torch.float64)
    # a few inputs outside the interval (evaluated in the edge bins) and the two ends themselves
    x[:8] = torch.tensor([lo - 0.05, lo - 1e-3, hi + 1e-3, hi + 0.05, lo, hi, lo - 0.01, hi + 0.01],
                         dtype=torch.float64)
    x = x.to(dtype)
    uw, uh, ud = (torch.randn(n, m, generator=g, dtype=torch.float64).mul(1.5).to(dtype) for m in (k, k, k + 1))
    gy, gl = (torch.randn(n, generator=g, dtype=torch.float64).to(dtype) for _ in range(2))
    lims = [torch.full((n,), v, dtype=dtype) for v in (lo_x, hi_x, lo_y, hi_y)]
    y, lad, got = _hip(x, uw, uh, ud, lims, gy, gl, inverse, check=False)
    dl = [t.cuda().requires_grad_() for t in (x, uw, uh, ud)]
    ys, lads = splines.rational_quadratic_spline(*dl, inverse=inverse, left=lo_x, right=hi_x, bottom=lo_y, top=hi_y)
    want = torch.autograd.grad([ys, lads], dl, [gy.cuda(), gl.cuda()])
    _lib.bad_discriminant_counter("cuda").zero_()     # outside points of the inverse may leave the quadratic's range

    def bits(t):          # bitwise, NaN included
        return t.detach().contiguous().view(torch.int64 if dtype == torch.float64 else torch.int32)
    assert torch.equal(bits(y), bits(ys)) and torch.equal(bits(lad), bits(lads))
    for a, b, nm in zip(got[:4], want, GRAD_NAMES):
        assert torch.equal(bits(a), bits(b)), nm


# ---------------------------------------------------------------- 6. errors
def _small(dtype=torch.float32, k=8, shape=(16, 4)):
    x, uw, uh, ud, lims, _, _ = _problem(k, shape, dtype, False, seed=9)
    return [t.cuda() for t in (x, uw, uh, ud)], [t.cuda() for t in lims]


def _call(args, lims, **kw):
    return splines.rational_quadratic_spline(*args, left=lims[0], right=lims[1], bottom=lims[2], top=lims[3], **kw)


def test_errors(hip):
    args, lims = _small()
    # left a tensor, any other limit a Python number: the reference fails indexing it
    for j in (1, 2, 3):
        mixed = list(lims)
        mixed[j] = 1.0
        with pytest.raises(TypeError):
            _call(args, mixed)
    # limits that do not broadcast to the inputs' shape
    for bad in (torch.zeros(5, device="cuda"), torch.zeros(16, 1, 4, device="cuda"), torch.zeros(3, 4, device="cuda")):
        wrong = list(lims)
        wrong[1] = bad + 1.0
        with pytest.raises(nf.VcnfError):
            _call(args, wrong)
    # another dtype than the inputs
    for j in range(4):
        other = list(lims)
        other[j] = other[j].double()
        with pytest.raises(nf.VcnfError):
            _call(args, other)
    args64, lims64 = _small(torch.float64)
    with pytest.raises(nf.VcnfError):
        _call(args64, [lims64[0].float()] + lims64[1:])
    # limits on the host (0-dim host tensors are accepted: test_zero_dim_host_limits)
    for j in range(4):
        host = list(lims)
        host[j] = host[j].cpu()
        with pytest.raises(nf.VcnfError):
            _call(args, host)
    # bin minima (splines.py:104-107)
    with pytest.raises(ValueError):
        _call(args, lims, min_bin_width=0.2)
    with pytest.raises(ValueError):
        _call(args, lims, min_bin_height=0.2)
    # a well-formed call still works, with and without gradients
    y, lad = _call(args, lims)
    assert torch.isfinite(y).all() and torch.isfinite(lad).all()
