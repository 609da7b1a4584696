"""Circular flows without a GPU: the vcnf_periodic_* and vcnf_uniform_gaussian_* symbols are exported and bound, their
host-side validation returns the documented status codes in the documented order before anything is launched, the
modules carry the reference's attribute and buffer names, CPU tensors get the values of the plain-torch restatement
(periodic_ref.py) bit for bit, and the restatement itself is pinned in fp64.  No call here passes validation with work to
do: nothing is ever launched on the fake pointers."""
import ctypes
import math

import pytest
import torch

import periodic_ref as ref
import vcnf_amd as nf
from vcnf_amd import _lib

FAKE = ctypes.c_void_p(0x1000)         # never dereferenced: validation fails first / the batch is empty
ODD = ctypes.c_void_p(0x1002)          # not aligned to a float, a double or an int32
DTYPES = [torch.float32, torch.float64]
STEMS = ("vcnf_periodic", "vcnf_uniform_gaussian_log_prob", "vcnf_uniform_gaussian_sample",
         "vcnf_uniform_gaussian_log_prob_bwd")
OK, NULL, SHAPE, ALIGN, UNSUPPORTED = 0, 1, 2, 3, 5


def test_symbols_exported_and_bound():
    handle = ctypes.CDLL(_lib.lib_path())
    for stem in STEMS:
        for sfx in ("_f32", "_f64"):
            name = stem + sfx
            assert hasattr(handle, name), "libvcnf_hip.so does not export " + name
            assert name in _lib.PROTOTYPES and getattr(nf.lib(), name).argtypes == _lib.PROTOTYPES[name][0]
    for sfx, scalar in (("_f32", ctypes.c_float), ("_f64", ctypes.c_double)):
        other = ctypes.c_double if scalar is ctypes.c_float else ctypes.c_float
        for stem, at, n_args in (("vcnf_periodic", 6, 8), ("vcnf_uniform_gaussian_log_prob", 2, 8),
                                 ("vcnf_uniform_gaussian_sample", 4, 11)):
            args = _lib.PROTOTYPES[stem + sfx][0]
            assert len(args) == n_args and args[at] is scalar and other not in args, stem + sfx
        args = _lib.PROTOTYPES["vcnf_uniform_gaussian_log_prob_bwd" + sfx][0]
        assert len(args) == 7 and ctypes.c_float not in args and ctypes.c_double not in args
    assert (_lib.OK, _lib.ERR_NULL, _lib.ERR_SHAPE, _lib.ERR_ALIGN, _lib.ERR_UNSUPPORTED) == (OK, NULL, SHAPE, ALIGN, UNSUPPORTED)
    for wrapper in ("periodic", "uniform_gaussian_log_prob", "uniform_gaussian_sample", "uniform_gaussian_log_prob_bwd"):
        assert callable(getattr(_lib, wrapper))


# name -> (pointer arguments in order, those that may be NULL, the arguments after the pointers given (rows, features))
def _periodic(L, sfx, z=FAKE, half=FAKE, shift=FAKE, out=FAKE, b=4, d=3):
    return getattr(L, "vcnf_periodic" + sfx)(z, half, shift, out, b, d, 1.0, None)


def _log_prob(L, sfx, z=FAKE, inv=FAKE, logp=FAKE, b=4, d=3, mode=0):
    return getattr(L, "vcnf_uniform_gaussian_log_prob" + sfx)(z, inv, -1.5, logp, b, d, mode, None)


def _sample(L, sfx, eps=FAKE, src=FAKE, offset=FAKE, scale=FAKE, inv=FAKE, z=FAKE, logp=FAKE, b=4, d=3):
    return getattr(L, "vcnf_uniform_gaussian_sample" + sfx)(eps, src, offset, scale, -1.5, inv, z, logp, b, d, None)


def _bwd(L, sfx, z=FAKE, inv=FAKE, g=FAKE, d_z=FAKE, b=4, d=3):
    return getattr(L, "vcnf_uniform_gaussian_log_prob_bwd" + sfx)(z, inv, g, d_z, b, d, None)


CALLS = {"periodic": (_periodic, ("z", "half", "out"), ("shift",)),
         "log_prob": (_log_prob, ("z", "inv", "logp"), ()),
         "sample": (_sample, ("eps", "src", "offset", "scale", "inv", "z", "logp"), ()),
         "bwd": (_bwd, ("z", "inv", "g", "d_z"), ())}


@pytest.mark.parametrize("sfx", ["_f32", "_f64"])
@pytest.mark.parametrize("entry", list(CALLS))
def test_validation_status_codes_in_the_documented_order(entry, sfx):
    call, required, optional = CALLS[entry]
    L = nf.lib()
    for name in required:
        assert call(L, sfx, **{name: None}) == NULL, name
        assert call(L, sfx, **{name: None}, d=0) == NULL and call(L, sfx, **{name: None}, b=0) == NULL      # NULL comes first
    for bad in (dict(d=0), dict(d=-3), dict(b=-1), dict(b=1 << 62, d=4)):                      # counts; rows * features overflows
        assert call(L, sfx, **bad) == SHAPE, bad
    # work beyond a grid: one lane per row of 3 or 4 columns, 256 rows per workgroup, 2^31 - 1 workgroups
    assert call(L, sfx, b=256 * (2 ** 31 - 1) + 1, d=3) == SHAPE
    assert call(L, sfx, b=-1, **{required[0]: ODD}) == SHAPE                                   # shape before alignment
    for name in required + optional:
        assert call(L, sfx, **{name: ODD}) == ALIGN, name
        assert call(L, sfx, **{name: ODD}, b=0) == OK                                          # an empty batch before alignment
    assert call(L, sfx, b=0) == OK and call(L, sfx, b=0, d=1 << 30) == OK                      # any number of features
    for name in optional:
        assert call(L, sfx, **{name: None}, b=0) == OK
    if entry == "log_prob":
        assert call(L, sfx, b=0, mode=_lib.LD_STORE) == OK and call(L, sfx, b=0, mode=_lib.LD_ACCUM) == OK
        for mode in (2, -1, 1 << 20):
            assert call(L, sfx, mode=mode) == UNSUPPORTED and call(L, sfx, mode=mode, b=0) == UNSUPPORTED
            assert call(L, sfx, mode=mode, d=0) == SHAPE and call(L, sfx, mode=mode, z=None) == NULL
            assert call(L, sfx, mode=mode, z=ODD) == UNSUPPORTED


# ---------------------------------------------------------------- the modules
def test_exports():
    assert nf.flows.periodic.PeriodicWrap is nf.flows.PeriodicWrap and nf.flows.periodic.PeriodicShift is nf.flows.PeriodicShift
    assert nf.distributions.base.UniformGaussian is nf.distributions.UniformGaussian
    assert issubclass(nf.flows.PeriodicWrap, nf.flows.Flow) and issubclass(nf.flows.PeriodicShift, nf.flows.Flow)
    assert issubclass(nf.distributions.UniformGaussian, nf.distributions.BaseDistribution)


def test_periodic_layers_attributes_and_state_dicts():
    w = nf.flows.PeriodicWrap([1, 2])
    assert w.ind == [1, 2] and w.bound == 1.0 and isinstance(w.bound, float)
    assert list(w.state_dict()) == [] and not list(w.parameters()) and not list(w.buffers())
    w = nf.flows.PeriodicWrap(2, math.pi)
    assert w.ind == 2 and w.bound == math.pi and list(w.state_dict()) == []
    w = nf.flows.PeriodicWrap(torch.tensor([0, 3], dtype=torch.int32), torch.tensor([1.0, 2.0]))
    assert list(w.state_dict()) == ["ind", "bound"] and w.ind.dtype == torch.int64 and w.bound.dtype == torch.float32
    assert w.double().bound.dtype == torch.float64 and w.ind.dtype == torch.int64 and not list(w.parameters())

    s = nf.flows.PeriodicShift([0])
    assert s.ind == [0] and s.bound == 1.0 and s.shift == 0.0 and list(s.state_dict()) == [] and not list(s.buffers())
    s = nf.flows.PeriodicShift([0], 2.0, torch.tensor(0.5))
    assert list(s.state_dict()) == ["shift"] and s.bound == 2.0
    s = nf.flows.PeriodicShift(torch.tensor([0, 1]), torch.tensor([1.0, 2.0]), torch.tensor([0.5, 0.25]))
    assert list(s.state_dict()) == ["ind", "bound", "shift"] and not list(s.parameters())
    assert s.ind.dtype == torch.int64
    other = nf.flows.PeriodicShift(torch.tensor([1, 0]), torch.ones(2), torch.zeros(2))
    other.load_state_dict(s.state_dict())
    assert other.shift.tolist() == [0.5, 0.25] and other.ind.tolist() == [0, 1]
    for layer in (w, s):
        assert not layer.takes_context and callable(layer.forward_into) and callable(layer.inverse_into)


def test_uniform_gaussian_attributes_and_state_dict():
    for ind, rest, inv_perm in (([1], [0, 2], [1, 0, 2]), (1, [0, 2], [1, 0, 2]), (torch.tensor([2, 0], dtype=torch.int32), [1], [1, 2, 0]),
                                ([], [0, 1, 2], [0, 1, 2]), ([0, 1, 2], [], [0, 1, 2])):
        q = nf.distributions.UniformGaussian(3, ind)
        want = ref.UniformGaussian(3, ind)
        assert list(q.state_dict()) == ["ind", "ind_", "inv_perm", "scale"] == list(want.state_dict())
        assert list(dict(q.named_buffers())) == ["ind", "ind_", "inv_perm", "scale"] and not list(q.parameters())
        assert q.ndim == 3 and q.ind_.tolist() == rest and q.inv_perm.tolist() == inv_perm
        for name in ("ind", "ind_", "inv_perm"):
            assert getattr(q, name).dtype == torch.int64 and torch.equal(getattr(q, name), getattr(want, name)), name
        assert q.scale.dtype == torch.float32 and q.scale.tolist() == [1.0, 1.0, 1.0]
        assert q.double().scale.dtype == torch.float64 and q.ind.dtype == torch.int64
    scale = torch.tensor([5.0, 2 * math.pi, 5.0])
    q = nf.distributions.UniformGaussian(3, [1], scale)
    assert torch.equal(q.scale, scale)
    model = nf.NormalizingFlow(q, [nf.flows.PeriodicShift([1], math.pi, 0.5), nf.flows.PeriodicWrap([1], math.pi)])
    assert list(model.state_dict()) == ["q0.ind", "q0.ind_", "q0.inv_perm", "q0.scale"]


# ---------------------------------------------------------------- CPU tensors: the restatement's values, bit for bit
def _rows(shape, dtype, bound=math.pi):
    g = torch.Generator().manual_seed(11)
    z = 3 * bound * torch.randn(shape, generator=g, dtype=torch.float64)
    flat = z.view(-1)
    flat[:6] = torch.tensor([bound, -bound, 0.0, -0.0, 7.3 * bound, 2 * bound], dtype=torch.float64)
    return z.to(dtype)


LAYER_CASES = [(3, [1], math.pi, 0.7), (5, torch.tensor([0, 3, 4]), torch.tensor([1.0, math.pi, 2.5]), torch.tensor([0.3, -4.0, 1.0])),
               (8, [0, 2, 5, 7], 1.0, 0.25), (7, [-1], 2.0, -0.4), (4, 2, torch.tensor(1.5), torch.tensor(0.5))]


@pytest.mark.parametrize("dtype", DTYPES + [torch.float16])
@pytest.mark.parametrize("case", range(len(LAYER_CASES)))
def test_cpu_layers_have_the_restatements_bits(case, dtype):
    d, ind, bound, shift = LAYER_CASES[case]
    cast = lambda v: v.to(dtype) if torch.is_tensor(v) and v.dim() else v
    z = _rows((33, d), dtype)
    for mine, want in ((nf.flows.PeriodicWrap(ind, cast(bound)), ref.PeriodicWrap(ind, cast(bound))),
                       (nf.flows.PeriodicShift(ind, cast(bound), cast(shift)), ref.PeriodicShift(ind, cast(bound), cast(shift)))):
        for direction in ("forward", "inverse"):
            got, ld = getattr(mine, direction)(z)
            exp, exp_ld = getattr(want, direction)(z)
            assert torch.equal(got, exp), (type(mine).__name__, direction)
            assert torch.equal(ld, exp_ld) and ld.dtype == dtype and tuple(ld.shape) == (33,)
            log_q = torch.full((33,), 2.0, dtype=dtype)
            assert torch.equal(getattr(mine, direction + "_into")(z, log_q), exp) and bool((log_q == 2.0).all())
    assert nf.flows.PeriodicWrap(ind, bound).forward(z)[0] is z
    # differentiable in z, derivative 1 on every column
    zg = z.double().requires_grad_()
    out, _ = nf.flows.PeriodicShift(ind, bound, shift).inverse(zg)
    g = torch.randn(out.shape, dtype=torch.float64, generator=torch.Generator().manual_seed(1))
    assert torch.equal(torch.autograd.grad(out, zg, g)[0], g)


def test_cpu_layers_raise_torchs_own_errors():
    z = torch.zeros(4, 3)
    with pytest.raises(IndexError):
        nf.flows.PeriodicWrap([3]).inverse(z)
    with pytest.raises(IndexError):
        nf.flows.PeriodicShift([-4]).forward(z)
    with pytest.raises(RuntimeError):
        nf.flows.PeriodicWrap([0, 1], torch.ones(3)).inverse(z)
    with pytest.raises(RuntimeError):
        nf.flows.PeriodicShift([0, 1], 1.0, torch.ones(3)).forward(z)


UG_CASES = [(2, [1], None), (3, [0, 2], torch.tensor([2 * math.pi, 0.5, 3.0])), (5, [], None), (2, [0, 1], torch.tensor([2.0, 6.0])),
            (8, [1, 4], torch.tensor([0.5, 2 * math.pi, 1.5, 2.0, 1.0, 0.25, 3.0, 1.0]))]


@pytest.mark.parametrize("dtype", DTYPES + [torch.float16])
@pytest.mark.parametrize("case", range(len(UG_CASES)))
def test_cpu_uniform_gaussian_has_the_restatements_bits(case, dtype):
    ndim, ind, scale = UG_CASES[case]
    mine = nf.distributions.UniformGaussian(ndim, ind, scale).to(dtype)
    want = ref.UniformGaussian(ndim, ind, scale).to(dtype)
    k = len(ind)
    g = torch.Generator().manual_seed(5)
    eps = torch.cat((torch.rand(17, k, generator=g, dtype=torch.float64), torch.randn(17, ndim - k, generator=g, dtype=torch.float64)), -1).to(dtype)
    z, lp = mine.from_noise(eps)
    wz, wlp = want.with_noise(eps)
    assert torch.equal(z, wz) and torch.equal(lp, wlp) and z.dtype == lp.dtype == dtype
    x = (3 * torch.randn(17, ndim, generator=g, dtype=torch.float64)).to(dtype)           # beyond the uniform range: finite
    assert torch.equal(mine.log_prob(x), want.log_prob(x)) and torch.isfinite(mine.log_prob(x)).all()
    out = torch.ones(17, dtype=dtype)
    assert mine.log_prob(x, out=out) is out and torch.equal(out, 1 + want.log_prob(x))
    if dtype != torch.float16:                                                             # (no half-precision draws on the CPU)
        torch.manual_seed(3)
        z, lp = mine(9)
        torch.manual_seed(3)
        wz, wlp = want(9)
        assert torch.equal(z, wz) and torch.equal(lp, wlp) and tuple(z.shape) == (9, ndim)
        torch.manual_seed(3)
        assert torch.equal(mine.sample(9), wz)
        xg = x.clone().requires_grad_()
        wg = x.clone().requires_grad_()
        mine.log_prob(xg).sum().backward()
        want.log_prob(wg).sum().backward()
        assert torch.equal(xg.grad, wg.grad)


# ---------------------------------------------------------------- the restatement, pinned in fp64
def test_restated_uniform_gaussian_integrates_to_one():
    """ndim 2, the uniform column 1 of width 3 integrated over its support, the Gaussian column 0 (scale 0.7) over +-9
    standard deviations: a midpoint sum of exp(log_prob) is 1 within 1e-9."""
    q = ref.UniformGaussian(2, [1], torch.tensor([0.7, 3.0], dtype=torch.float64))
    n = 2000
    g = -6.3 + 12.6 / n * (torch.arange(n, dtype=torch.float64) + 0.5)
    u = -1.5 + 3.0 / 50 * (torch.arange(50, dtype=torch.float64) + 0.5)
    total = float(torch.exp(q.log_prob(torch.cartesian_prod(g, u))).sum()) * (12.6 / n) * (3.0 / 50)
    assert abs(total - 1.0) <= 1e-9, total
    z = q.sample(1000)
    assert float(z[:, 1].abs().max()) <= 1.5 and float(z[:, 0].abs().max()) > 1.5


def test_restated_shift_inverts_modulo_the_period_and_wrap_lands_in_range():
    for d, ind, bound, shift in LAYER_CASES:
        z = _rows((257, d), torch.float64)
        layer = ref.PeriodicShift(ind, bound, shift)
        back = layer.inverse(layer.forward(z)[0])[0]
        b = torch.as_tensor(bound, dtype=torch.float64)
        diff = (back - z)[..., ind]
        circ = torch.remainder(diff + b, 2 * b) - b
        # |z| + |shift| + bound < 64 here: each of the two directions rounds twice at that size, half an ulp (7.1e-15) each,
        # and twice more below 2 bound
        assert float(z.abs().max()) < 56 and float(circ.abs().max()) <= 4e-14
        others = [j for j in range(d) if j not in [i % d for i in torch.as_tensor(ind).reshape(-1).tolist()]]
        assert torch.equal(back[..., others], z[..., others])
        wrapped = ref.PeriodicWrap(ind, bound).inverse(z)[0][..., ind]
        assert bool(((wrapped >= -b) & (wrapped <= b)).all())
        assert torch.equal(ref.PeriodicWrap(ind, bound).inverse(z)[0][..., others], z[..., others])
