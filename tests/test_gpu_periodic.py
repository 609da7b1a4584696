"""Circular flows on the device (csrc/periodic.hip): PeriodicWrap / PeriodicShift against the same-dtype plain-torch
restatement (periodic_ref.py) run on the same device, bit for bit - every step of the map is one correctly rounded add
or an exact fmod, so a tolerance would only hide a wrong branch at the wrap; UniformGaussian against the restatement in
fp64 on the CPU; and the reference's circular spline model built twice over the same couplings, once with the package's
classes and once with the restatement's.

The fp32 tolerance of the base is a measurement, taken per case: the largest error of the fp32 restatement on the
device against the fp64 values over the case's inputs (both batches), times 4 (absolute; it is printed).  The fp64
tolerance is rtol = atol = 1e-12."""
import math

import pytest
import torch

import periodic_ref as ref
import vcnf_amd as nf
from helpers import assert_close
from vcnf_amd import _lib

pytestmark = pytest.mark.gpu
DTYPES = [torch.float32, torch.float64]
PI = math.pi


# ---------------------------------------------------------------- the periodic layers
# (features, ind, bound, shift, input shapes).  3: the scalar path with one wrapped column; 5: per-index tensors; 8: the
# pack path (16-byte packs of fp32, 8-byte pairs of fp64), also with the index on the last axis of a 3-D input; 7: a
# negative index on the scalar path, one row and more than one workgroup (257 rows of one lane each); 6: 8-byte pairs of
# fp32 as well
LAYER_CASES = {
    "d3": (3, [1], PI, 0.7, [(257, 3)]),
    "d6_pairs": (6, [1, 4], 2.0, 0.7, [(257, 6)]),
    "d5_tensors": (5, torch.tensor([0, 3, 4]), torch.tensor([1.0, PI, 2.5]), torch.tensor([0.3, -4.0, 1.0]), [(257, 5)]),
    "d8_pack": (8, [0, 2, 5, 7], 2.0, -1.3, [(257, 8), (5, 7, 8)]),
    "d7_negative": (7, [-1], 1.0, 0.25, [(1, 7), (257, 7)]),
    # more chunks than the 64 lanes of a row's group: a lane walks several, the last of them ragged (517: one column,
    # scalar path; 520: the pack path, 130 chunks of fp32 and 260 of fp64)
    "d517_wide": (517, list(range(0, 517, 3)), 1.5, 0.4, [(3, 517)]),
    "d520_wide_pack": (520, list(range(1, 520, 2)), 1.5, 0.4, [(3, 520)]),
}


def _columns(d, ind, bound):
    """[(column, its bound)] of the wrapped columns."""
    idx = [i % d for i in torch.as_tensor(ind).reshape(-1).tolist()]
    b = torch.as_tensor(bound, dtype=torch.float64).reshape(-1)
    return [(c, float(b[k if len(b) > 1 else 0])) for k, c in enumerate(idx)]


def _layer_input(shape, d, ind, bound, dtype):
    """N(0, (3 bound)^2) on the wrapped columns (N(0, 9) on the others), with the values where the map can go wrong planted
    at the top of every wrapped column, as far as the rows go: +-bound, the two floats next to each, 0, -0., +-7.3 bound
    and 2 bound exactly."""
    g = torch.Generator().manual_seed(1234 + d + len(shape))
    z = 3 * torch.randn(shape, generator=g, dtype=torch.float64)
    rows = z.view(-1, d)
    for c, b in _columns(d, ind, bound):
        rows[:, c] *= b
    z = z.to(dtype)
    rows = z.view(-1, d)
    for c, b in _columns(d, ind, bound):
        bt = torch.tensor(b, dtype=torch.float64).to(dtype)          # the bound as the layer rounds it
        inf = torch.tensor(math.inf, dtype=dtype)
        planted = torch.stack([bt, -bt, torch.nextafter(bt, inf), torch.nextafter(bt, -inf), torch.nextafter(-bt, inf),
                               torch.nextafter(-bt, -inf), torch.tensor(0.0, dtype=dtype), torch.tensor(-0.0, dtype=dtype),
                               (7.3 * bt.double()).to(dtype), (-7.3 * bt.double()).to(dtype), 2 * bt])
        n = min(len(rows), len(planted))
        rows[:n, c] = planted[:n]
        if len(rows) == 1:                                             # one row: a different planted value per column
            rows[0, c] = planted[c % len(planted)]
    return z


def _pairs(case, dtype, dev):
    d, ind, bound, shift, shapes = LAYER_CASES[case]
    cast = lambda v: v.to(dtype) if torch.is_tensor(v) and v.is_floating_point() else v
    pairs = [(nf.flows.PeriodicWrap(ind, cast(bound)), ref.PeriodicWrap(ind, cast(bound))),
             (nf.flows.PeriodicShift(ind, cast(bound), cast(shift)), ref.PeriodicShift(ind, cast(bound), cast(shift)))]
    return d, ind, bound, shapes, [(a.to(dev), b.to(dev)) for a, b in pairs]


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("case", list(LAYER_CASES))
def test_periodic_layers_have_the_restatements_bits(hip, case, dtype):
    d, ind, bound, shapes, pairs = _pairs(case, dtype, hip)
    for shape in shapes:
        z = _layer_input(shape, d, ind, bound, dtype).to(hip)
        for mine, want in pairs:
            for direction in ("forward", "inverse"):
                what = "%s.%s %s" % (type(mine).__name__, direction, shape)
                got, ld = getattr(mine, direction)(z)
                exp, _ = getattr(want, direction)(z)
                differ = int((got != exp).sum())
                print("%s: %d of %d elements differ" % (what, differ, got.numel()))
                assert torch.equal(got, exp), what
                assert ld.dtype == dtype and tuple(ld.shape) == (shape[0],) and not ld.any() and ld.device == z.device
                log_q = torch.full((shape[0],), 2.0, dtype=dtype, device=hip)
                assert torch.equal(getattr(mine, direction + "_into")(z, log_q), exp) and bool((log_q == 2.0).all())
                if direction == "forward" and isinstance(mine, nf.flows.PeriodicWrap):
                    assert got is z and mine.forward_into(z, log_q) is z
                    continue
                # the kernel ran (no table means the torch composition), and in place it gives the same bits
                half, shift = mine._tables(z)
                assert half is not None and half.dtype == dtype and tuple(half.shape) == (d,)
                sign = -1.0 if (direction == "inverse" and shift is not None) else 1.0
                same = z.clone()
                assert _lib.periodic(same, half, shift, sign, out=same) is same and torch.equal(same, exp), what + " in place"
                # under autograd: one node, the gradient handed on unchanged on every column
                zg = z.clone().requires_grad_()
                out, _ = getattr(mine, direction)(zg)
                assert torch.equal(out, exp) and type(out.grad_fn).__name__ == "PeriodicFnBackward"
                g = torch.randn(shape, dtype=dtype, device=hip)
                assert torch.equal(torch.autograd.grad(out, zg, g)[0], g)
        # the wrap lands in [-bound, bound] and leaves the other columns alone
        wrapped = pairs[0][0].inverse(z)[0].view(-1, d)
        for c, b in _columns(d, ind, bound):
            assert float(wrapped[:, c].abs().max()) <= float(torch.tensor(b, dtype=torch.float64).to(dtype))
        others = [j for j in range(d) if j not in [c for c, _ in _columns(d, ind, bound)]]
        assert torch.equal(wrapped[:, others], z.view(-1, d)[:, others])


@pytest.mark.parametrize("dtype", DTYPES + [torch.float16], ids=["f32", "f64", "f16"])
def test_periodic_layers_off_the_kernel_path_take_the_composition(hip, dtype):
    """Half precision, a non-contiguous input: the restatement's values; a mis-shaped bound or a per-index bound of a wider
    dtype: torch's own error; an index out of range: an IndexError raised on the host (the restatement is not called
    with one: on the device torch's index check is an assertion inside its kernel)."""
    z = _layer_input((33, 8), 8, [0, 2, 5, 7], 2.0, torch.float64).to(dtype).to(hip)
    mine, want = nf.flows.PeriodicShift([0, 2, 5, 7], 2.0, -1.3), ref.PeriodicShift([0, 2, 5, 7], 2.0, -1.3)
    assert torch.equal(mine.forward(z)[0], want.forward(z)[0])
    zt = z.t().contiguous().t()
    assert not zt.is_contiguous() and torch.equal(mine.inverse(zt)[0], want.inverse(zt)[0])
    # a per-index bound of a wider dtype: torch computes in that dtype and refuses to store the result
    wide = torch.tensor([1.0, 2.0, 3.0, 4.0], dtype=torch.float64, device=hip)
    if dtype == torch.float64:
        assert torch.equal(nf.flows.PeriodicWrap([0, 2, 5, 7], wide).inverse(z)[0], ref.PeriodicWrap([0, 2, 5, 7], wide).inverse(z)[0])
    else:
        for layer in (nf.flows.PeriodicWrap([0, 2, 5, 7], wide), ref.PeriodicWrap([0, 2, 5, 7], wide)):
            with pytest.raises(RuntimeError, match="dtypes match"):
                layer.inverse(z)
    narrow = torch.tensor([1.0, 2.0, 3.0, 4.0], dtype=torch.float16, device=hip)       # a narrower one is converted exactly
    assert torch.equal(nf.flows.PeriodicWrap([0, 2, 5, 7], narrow).inverse(z)[0], ref.PeriodicWrap([0, 2, 5, 7], narrow).inverse(z)[0])
    with pytest.raises(IndexError):
        nf.flows.PeriodicWrap([8]).inverse(z)
    with pytest.raises(RuntimeError):
        nf.flows.PeriodicShift([0, 1], 1.0, torch.ones(3, dtype=dtype, device=hip)).forward(z)
    zg = z.clone().requires_grad_()
    out = mine.inverse(zg.t().contiguous().t())[0]
    g = torch.randn_like(out)
    assert torch.equal(torch.autograd.grad(out, zg, g)[0], g)


# ---------------------------------------------------------------- UniformGaussian
UG_CASES = {
    "2_[1]": (2, [1], torch.tensor([0.7, 3.0])),
    "3_[0,2]": (3, [0, 2], torch.tensor([2 * PI, 0.5, 3.0])),
    "8_[1,4]": (8, [1, 4], torch.tensor([0.5, 2 * PI, 1.5, 2.0, 1.0, 0.25, 3.0, 1.25])),
    "5_[]": (5, [], torch.tensor([1.0, 2.0, 0.5, 1.5, 3.0])),
    "2_[0,1]": (2, [0, 1], torch.tensor([2.0, 2 * PI])),
    "3_[1]_model": (3, [1], torch.tensor([5.0, 2 * PI, 5.0])),                    # the base of the model below
    # more chunks than the 64 lanes of a row's group, the last one ragged
    "517_wide": (517, list(range(1, 517, 5)), 0.5 + torch.rand(517, generator=torch.Generator().manual_seed(3))),
}
BATCHES = (1, 257)
_REF64 = {}


def _ug_inputs(case, batch):
    """(eps in the order drawn, points x, weights w, log_prob(x) and the gradient of sum(w log_prob(x)) in fp64 on the CPU),
    computed once.  x is drawn 2 scale wide: most uniform columns lie outside their range."""
    key = (case, batch)
    if key not in _REF64:
        ndim, ind, scale = UG_CASES[case]
        g = torch.Generator().manual_seed(77 + 13 * list(UG_CASES).index(case) + batch)
        k = len(ind)
        eps = torch.cat((torch.rand(batch, k, generator=g, dtype=torch.float64),
                         torch.randn(batch, ndim - k, generator=g, dtype=torch.float64)), -1)
        x = (2 * scale.double() * torch.randn(batch, ndim, generator=g, dtype=torch.float64)).float()   # exact in both dtypes
        w = torch.randn(batch, generator=g, dtype=torch.float64).float()
        q = ref.UniformGaussian(ndim, ind, scale.double())
        xg = x.double().requires_grad_()
        lp = q.log_prob(xg)
        grad = torch.autograd.grad((lp * w.double()).sum(), xg)[0]
        _REF64[key] = (eps.float(), x, w, lp.detach(), grad)
    return _REF64[key]


@pytest.fixture(scope="module")
def tol(hip):
    """{(case, dtype): (rtol, atol)} of the base: fp32 from the measurement the module's docstring describes."""
    out = {}
    for case in UG_CASES:
        ndim, ind, scale = UG_CASES[case]
        q = ref.UniformGaussian(ndim, ind, scale).to(hip)
        worst = 0.0
        for batch in BATCHES:
            _, x, _, lp64, _ = _ug_inputs(case, batch)
            worst = max(worst, float((q.log_prob(x.to(hip)).cpu().double() - lp64).abs().max()))
        print("UniformGaussian %s: fp32 restatement on the device against fp64, largest error %.3e; tolerance 4 x that" % (case, worst))
        assert worst > 0.0
        out[case, torch.float32] = (0.0, 4 * worst)
        out[case, torch.float64] = (1e-12, 1e-12)
    return out


def _ug_pair(case, dtype, dev):
    ndim, ind, scale = UG_CASES[case]
    return nf.distributions.UniformGaussian(ndim, ind, scale).to(dtype).to(dev), ref.UniformGaussian(ndim, ind, scale).to(dtype).to(dev)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("case", list(UG_CASES))
def test_uniform_gaussian(hip, tol, case, dtype):
    rtol, atol = tol[case, dtype]
    mine, want = _ug_pair(case, dtype, hip)
    for batch in BATCHES:
        eps, x, w, lp64, grad64 = _ug_inputs(case, batch)
        eps, x, w = eps.to(dtype).to(hip), x.to(dtype).to(hip), w.to(dtype).to(hip)
        what = "%s B=%d %s" % (case, batch, dtype)
        # sampling: one subtract and one multiply per element, so the restatement's bits; log p of that z
        z, lp = mine.from_noise(eps)
        wz, _ = want.with_noise(eps)
        assert torch.equal(z, wz) and z.dtype == lp.dtype == dtype and tuple(lp.shape) == (batch,), what
        z64 = ref.UniformGaussian(*UG_CASES[case][:2], UG_CASES[case][2].double()).log_prob(z.cpu().double())
        assert_close(lp, z64, rtol, atol, what + " from_noise log p")
        # density, also outside the uniform range
        got = mine.log_prob(x)
        print("%s: log_prob error %.3e (atol %.3e)" % (what, float((got.cpu().double() - lp64).abs().max()), atol))
        assert torch.isfinite(got).all() and got.dtype == dtype
        assert_close(got, lp64, rtol, atol, what + " log_prob")
        out = torch.randn(batch, dtype=dtype, device=hip)
        start = out.clone()
        assert mine.log_prob(x, out=out) is out and torch.equal(out, start + got), what + " out="
        # gradient: one node, one launch
        xg = x.clone().requires_grad_()
        lpg = mine.log_prob(xg)
        assert torch.equal(lpg, got) and type(lpg.grad_fn).__name__ == "UniformGaussianLogProbFnBackward"
        grad = torch.autograd.grad((lpg * w).sum(), xg)[0]
        assert_close(grad, grad64, rtol, atol, what + " gradient")
        xg = x.clone().requires_grad_()
        acc = mine.log_prob(xg, out=start.clone())
        assert_close(torch.autograd.grad((acc * w).sum(), xg)[0], grad64, rtol, atol, what + " gradient through out=")
    # fresh draws: the reference's two draws in its order
    torch.manual_seed(5)
    z, lp = mine(257)
    torch.manual_seed(5)
    wz = want.sample(257)
    assert torch.equal(z, wz) and tuple(z.shape) == (257, UG_CASES[case][0])
    assert_close(lp, ref.UniformGaussian(*UG_CASES[case][:2], UG_CASES[case][2].double()).log_prob(z.cpu().double()), rtol, atol,
                 case + " forward log p")
    torch.manual_seed(5)
    assert torch.equal(mine.sample(257), wz)
    k = len(UG_CASES[case][1])
    if k:
        half = (UG_CASES[case][2][UG_CASES[case][1]] / 2).to(dtype).to(hip)
        assert bool((z[:, UG_CASES[case][1]].abs() <= half).all())


def test_uniform_gaussian_off_the_kernel_path_takes_the_composition(hip):
    mine, want = _ug_pair("8_[1,4]", torch.float16, hip)
    _, x, _, _, _ = _ug_inputs("8_[1,4]", 257)
    x = x.to(torch.float16).to(hip)
    assert torch.equal(mine.log_prob(x), want.log_prob(x))
    mine, want = _ug_pair("8_[1,4]", torch.float32, hip)
    eps = _ug_inputs("8_[1,4]", 257)[0].to(hip).requires_grad_()          # a draw that requires grad: differentiable in eps
    z, lp = mine.from_noise(eps)
    wz, wlp = want.with_noise(eps)
    assert torch.equal(z, wz) and torch.equal(lp, wlp) and z.requires_grad


# ---------------------------------------------------------------- the reference's circular spline model
B = 129


def _models(dtype, dev):
    """The model with the package's classes and its twin with the restatement's, over the same coupling objects."""
    torch.manual_seed(21)
    bound = torch.tensor([2.5, PI, 2.5])
    couplings = [nf.flows.CircularCoupledRationalQuadraticSpline(3, 1, 16, [1], num_bins=4, tail_bound=bound, reverse_mask=i % 2,
                                                                 init_identity=False) for i in range(4)]
    scale = torch.tensor([5.0, 2 * PI, 5.0])
    mine, twin = [], []
    for i, c in enumerate(couplings):
        mine += [c, nf.flows.PeriodicShift([1], PI, 0.5 + i)]
        twin += [c, ref.PeriodicShift([1], PI, 0.5 + i)]
    mine.append(nf.flows.PeriodicWrap([1], PI))
    twin.append(ref.PeriodicWrap([1], PI))
    model = nf.NormalizingFlow(nf.distributions.UniformGaussian(3, [1], scale), mine).to(dtype).to(dev)
    other = nf.NormalizingFlow(ref.UniformGaussian(3, [1], scale), twin).to(dtype).to(dev)
    g = torch.Generator().manual_seed(8)
    x = torch.stack([1.5 * torch.randn(B, generator=g, dtype=torch.float64),
                     PI * (2 * torch.rand(B, generator=g, dtype=torch.float64) - 1),
                     1.5 * torch.randn(B, generator=g, dtype=torch.float64)], 1).to(dtype).to(dev)
    eps = torch.cat((torch.rand(B, 1, generator=g, dtype=torch.float64), torch.randn(B, 2, generator=g, dtype=torch.float64)), 1)
    return model, other, x, eps.to(dtype).to(dev)


def _twin_sample(twin, eps):
    z, log_q = twin.q0.with_noise(eps)
    return twin._walk(z, log_q, None, False)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_circular_spline_model(hip, tol, dtype):
    rtol, atol = tol["3_[1]_model", dtype]
    model, twin, x, eps = _models(dtype, hip)
    with torch.no_grad():
        # density: every layer in between bit-equal, log q within the base's tolerance
        a = b = x
        for mine, theirs in zip(reversed(model.flows), reversed(twin.flows)):
            a, lda = mine.inverse(a)
            b, ldb = theirs.inverse(b)
            assert torch.equal(a, b) and torch.equal(lda, ldb), type(mine).__name__
        assert not torch.equal(a, x)
        lp, lp_twin = model.log_prob(x), twin.log_prob(x)
        assert torch.isfinite(lp).all() and lp.dtype == dtype
        assert_close(lp, lp_twin, rtol, atol, "model log_prob")
        # sampling from the same draws
        z, lq = model.sample_from(eps)
        zt, lqt = _twin_sample(twin, eps)
        assert torch.equal(z, zt) and bool((z[:, 1].abs() <= torch.tensor(PI, dtype=dtype)).all())
        assert_close(lq, lqt, rtol, atol, "model sample log q")
        # the round trip, against the twin's own
        mine_rt = float((model.log_prob(z) - lq).abs().max())
        twin_rt = float((twin.log_prob(zt) - lqt).abs().max())
        print("%s: log_prob(sample) - log_q: model %.3e, twin %.3e" % (dtype, mine_rt, twin_rt))
        assert mine_rt <= 2 * twin_rt
        zs, lqs = model.sample(B)
        assert tuple(zs.shape) == (B, 3) and torch.isfinite(lqs).all() and bool((zs[:, 1].abs() <= torch.tensor(PI, dtype=dtype)).all())
    # training: the coupling parameters' gradients of forward_kld
    params = [p for p in model.parameters()]
    assert params and len(params) == len(list(twin.parameters()))
    grads = []
    for m in (model, twin):
        for p in params:
            p.grad = None
        loss = m.forward_kld(x)
        loss.backward()
        grads.append((float(loss.detach()), [p.grad.clone() for p in params]))
    assert abs(grads[0][0] - grads[1][0]) <= atol + rtol * abs(grads[1][0])
    assert any(float(g.abs().max()) > 0 for g in grads[0][1])
    for (name, _), g, gt in zip(model.named_parameters(), grads[0][1], grads[1][1]):
        assert_close(g, gt, rtol, atol, "d forward_kld / d " + name)


@pytest.mark.parametrize("kind", ["scalar", "tensor"])
def test_g18_circular_coupled_layer_fp64(hip, kind):
    """What the model above needs of its couplings under .double(): the per-feature unconditional spline of the identity
    half without autograd in fp64.  The layer of fixture G18 against the reference's fp64 run, at the standing figures of
    the fp64 layer tests (z 1e-10, log-det 1e-9)."""
    from helpers import T, fixture, state_for
    fx = fixture("g18_per_feature_tails")
    sd, _ = state_for(fx, "layer/" + kind, 1801, torch.float64, final_gain=2.0)
    tb = 3.0 if kind == "scalar" else T(fx["layer/bound"])
    lay = nf.flows.CircularCoupledRationalQuadraticSpline(7, 1, 32, ind_circ=[0, 3, 4], num_bins=8, tail_bound=tb,
                                                          init_identity=False).double()
    lay.load_state_dict(sd, strict=False)              # tail-bound / scale buffers keep their constructor values
    lay = lay.to(hip)
    x = T(fx["layer/x"], torch.float64).to(hip)
    with torch.no_grad():
        for dirn, fn in (("fwd", lay.forward), ("inv", lay.inverse)):
            z, ld = fn(x)
            assert z.dtype == ld.dtype == torch.float64
            assert_close(z, fx["layer/%s/%s_z64" % (kind, dirn)], 1e-10, 1e-10, dirn + " z")
            assert_close(ld, fx["layer/%s/%s_ld64" % (kind, dirn)], 1e-9, 1e-9, dirn + " ld")
    nf.check_discriminant()
