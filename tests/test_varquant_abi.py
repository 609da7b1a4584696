"""Categorical dequantisation without a GPU: the vcnf_dequant_* / vcnf_quantize_* symbols are declared in the header,
exported and bound, their host-side validation returns the documented status codes in the documented order before
anything is launched, the model constructor accepts and refuses what the specification says, a model without categorical
columns is what it was, and CPU tensors get the values of the plain-torch restatement (varquant_ref.py) bit for bit.
No call here passes validation with work to do: nothing is ever launched on the fake pointers."""
import ctypes
import os

import pytest
import torch

import varquant_ref as ref
import vcnf_amd as nf
from vcnf_amd import _lib

FAKE = ctypes.c_void_p(0x1000)         # never dereferenced: validation fails first / the batch is empty
ODD = ctypes.c_void_p(0x1002)          # not aligned to a float, a double or an int32
STEMS = ("vcnf_dequant_prepare", "vcnf_dequant_merge", "vcnf_dequant_merge_bwd", "vcnf_quantize")
OK, NULL, SHAPE, ALIGN, UNSUPPORTED = 0, 1, 2, 3, 5
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "vcnf_hip.h")


def test_symbols_declared_exported_and_bound():
    with open(HEADER) as f:
        header = f.read()
    handle = ctypes.CDLL(_lib.lib_path())
    for stem in STEMS:
        for sfx in ("_f32", "_f64"):
            name = stem + sfx
            assert ("int %s(" % name) in header, "the header does not declare " + name
            assert hasattr(handle, name), "libvcnf_hip.so does not export " + name
            assert name in _lib.PROTOTYPES and getattr(nf.lib(), name).argtypes == _lib.PROTOTYPES[name][0]
    for sfx, scalar in (("_f32", ctypes.c_float), ("_f64", ctypes.c_double)):
        for stem, n_args, has_ld in (("vcnf_dequant_prepare", 14, True), ("vcnf_dequant_merge", 14, True),
                                     ("vcnf_dequant_merge_bwd", 14, False), ("vcnf_quantize", 12, True)):
            args = _lib.PROTOTYPES[stem + sfx][0]
            assert len(args) == n_args, stem + sfx
            # alpha crosses the ABI in fp64 for both element types; ld_sign has the element type
            assert sum(a is ctypes.c_double for a in args) == 1 + (has_ld and scalar is ctypes.c_double), stem + sfx
            if has_ld:
                assert args[-2] is scalar, stem + sfx
    assert "csrc/dequant.hip" in header and "floor(y K)" in header and "logsigmoid(w) + logsigmoid(-w)" in header
    for wrapper in ("dequant_prepare", "dequant_merge", "dequant_merge_bwd", "quantize", "column_tables"):
        assert callable(getattr(_lib, wrapper))
    assert "dequant.hip" in nf._lib._build.SOURCES


def _prepare(L, sfx, x=FAKE, slot=FAKE, levels=FAKE, u=FAKE, v=FAKE, ctx=FAKE, ld=FAKE, b=4, d=3, c=2, mode=0):
    return getattr(L, "vcnf_dequant_prepare" + sfx)(x, slot, levels, u, 1e-5, v, ctx, ld, b, d, c, mode, 1.0, None)


def _merge(L, sfx, x=FAKE, slot=FAKE, levels=FAKE, w=FAKE, out=FAKE, ld=FAKE, b=4, d=3, c=2, mode=0, logit=1):
    return getattr(L, "vcnf_dequant_merge" + sfx)(x, slot, levels, w, logit, 1e-5, out, ld, b, d, c, mode, 1.0, None)


def _merge_bwd(L, sfx, x=FAKE, slot=FAKE, levels=FAKE, w=FAKE, g_out=FAKE, g_ld=FAKE, d_w=FAKE, d_x=FAKE, b=4, d=3, c=2,
               logit=1):
    return getattr(L, "vcnf_dequant_merge_bwd" + sfx)(x, slot, levels, w, logit, 1e-5, g_out, g_ld, d_w, d_x, b, d, c, None)


def _quantize(L, sfx, x=FAKE, slot=FAKE, levels=FAKE, out=FAKE, ld=FAKE, b=4, d=3, c=2, mode=0):
    return getattr(L, "vcnf_quantize" + sfx)(x, slot, levels, 1e-5, out, ld, b, d, c, mode, 1.0, None)


# name -> (call, required pointers, optional pointers, has an ld_mode); every pointer is held to its element's alignment
CALLS = {"prepare": (_prepare, ("x", "slot", "levels", "u", "v", "ctx", "ld"), (), True),
         "merge": (_merge, ("x", "slot", "levels", "w", "out", "ld"), (), True),
         "merge_bwd": (_merge_bwd, ("x", "slot", "levels", "w", "d_w"), ("g_out", "g_ld", "d_x"), False),
         "quantize": (_quantize, ("x", "slot", "levels", "out", "ld"), (), True)}


@pytest.mark.parametrize("sfx", ["_f32", "_f64"])
@pytest.mark.parametrize("entry", list(CALLS))
def test_validation_status_codes_in_the_documented_order(entry, sfx):
    call, required, optional, has_mode = CALLS[entry]
    L = nf.lib()
    for name in required:
        assert call(L, sfx, **{name: None}) == NULL, name
        assert call(L, sfx, **{name: None}, d=0) == NULL and call(L, sfx, **{name: None}, b=0) == NULL      # NULL comes first
    # sizes: features, the categorical count against them, the batch, rows * features beyond int64
    for bad in (dict(d=0), dict(d=-3), dict(b=-1), dict(c=-1), dict(c=4), dict(b=1 << 62, d=4)):
        assert call(L, sfx, **bad) == SHAPE, bad
        assert call(L, sfx, **bad, **{required[0]: ODD}) == SHAPE                                # shape before alignment
    for name in required + optional:
        assert call(L, sfx, **{name: ODD}) == ALIGN, name
        assert call(L, sfx, **{name: ODD}, b=0) == ALIGN                                         # alignment before the empty batch
    assert call(L, sfx, b=0) == OK and call(L, sfx, b=0, d=1 << 30, c=0) == OK                   # any number of features
    assert call(L, sfx, b=0, c=3) == OK and call(L, sfx, b=0, c=0) == OK                         # any C <= D
    for name in optional:
        assert call(L, sfx, **{name: None}, b=0) == OK
    if has_mode:
        assert call(L, sfx, b=0, mode=_lib.LD_STORE) == OK and call(L, sfx, b=0, mode=_lib.LD_ACCUM) == OK
        for mode in (2, -1, 1 << 20):
            assert call(L, sfx, mode=mode) == UNSUPPORTED and call(L, sfx, mode=mode, b=0) == UNSUPPORTED
            assert call(L, sfx, mode=mode, d=0) == SHAPE and call(L, sfx, mode=mode, ld=None) == NULL
            assert call(L, sfx, mode=mode, ld=ODD) == ALIGN                                      # alignment before the mode
    if "logit" in call.__code__.co_varnames:
        assert call(L, sfx, b=0, logit=0) == OK


def test_wrappers_refuse_what_the_kernels_cannot_take():
    x = torch.zeros(4, 3)
    with pytest.raises(nf.VcnfError):
        _lib.dequant_merge(x, torch.zeros(3, dtype=torch.int32), torch.ones(1, dtype=torch.int32), torch.zeros(4, 1), False, 1e-5)
    with pytest.raises(nf.VcnfError):
        _lib.column_tables([3], [2], 3, "cpu")
    with pytest.raises(nf.VcnfError):
        _lib.column_tables([1, 1], [2, 2], 3, "cpu")
    with pytest.raises(nf.VcnfError):
        _lib.column_tables([1], [0], 3, "cpu")
    slot, levels = _lib.column_tables([2, 0], [5, 7], 3, "cpu")
    assert slot.tolist() == [1, -1, 0] and levels.tolist() == [5, 7] and slot.dtype == levels.dtype == torch.int32
    assert _lib.column_tables([2, 0], [5, 7], 3, "cpu")[0] is slot, "the tables are built once and kept"


# ---------------------------------------------------------------- the constructor
def _q0(d=6):
    return nf.distributions.DiagGaussian(d)


def test_a_model_without_categoricals_is_what_it_was():
    model = nf.NormalizingFlow(_q0(), [])
    assert model.categoricals is None and model.catlevels is None and not hasattr(model, "catvdeqs")
    assert list(model.state_dict()) == ["q0.loc", "q0.log_scale"]
    with pytest.raises(RuntimeError):
        model.dequantize(torch.zeros(2, 6))
    with pytest.raises(RuntimeError):
        model.quantize(torch.zeros(2, 6))
    assert nf.ClassCondFlow(_q0(), []).categoricals is None


def test_constructor_accepts_the_forks_call():
    model = nf.NormalizingFlow(_q0(), [], None, [0, 2, 5], [3, 2, 7])
    assert model.categoricals == [0, 2, 5] and model.catlevels == [3, 2, 7]
    assert isinstance(model.catvdeqs, nf.nets.Dequantization) and model.catvdeqs.alpha == 1e-5
    assert not isinstance(model.catvdeqs, nf.nets.VariationalDequantization)
    assert list(model.state_dict()) == ["q0.loc", "q0.log_scale"]
    var_flows = [nf.flows.CoupledRationalQuadraticSpline(3, 1, 16, num_context_channels=3) for _ in range(2)]
    vdq = nf.nets.VariationalDequantization(var_flows)
    assert isinstance(vdq.flows, torch.nn.ModuleList) and vdq.alpha == 1e-5 and len(vdq.flows) == 2
    model = nf.NormalizingFlow(_q0(), [], categoricals=(0, 2, 5), catlevels=(3, 2, 7), catvdeqs=vdq)
    assert model.catvdeqs is vdq and model.categoricals == [0, 2, 5]
    keys = list(model.state_dict())
    assert any(k.startswith("catvdeqs.flows.0.") for k in keys) and any(k.startswith("catvdeqs.flows.1.") for k in keys)
    assert all(k.startswith(("q0.", "catvdeqs.flows.")) for k in keys)
    assert "lower bound" in nf.NormalizingFlow.log_prob.__doc__
    assert nf.nets.VariationalDequantization([], alpha=0.05).alpha == 0.05 and nf.nets.Dequantization(0).alpha == 0.0


@pytest.mark.parametrize("kwargs, error, word", [
    (dict(categoricals=[0, 1]), ValueError, "catlevels"),
    (dict(catlevels=[2, 3]), ValueError, "categoricals"),
    (dict(categoricals=[0, 1], catlevels=[2]), ValueError, "equal lengths"),
    (dict(categoricals=[0, 0], catlevels=[2, 2]), ValueError, "categoricals"),
    (dict(categoricals=[0, -1], catlevels=[2, 2]), ValueError, "categoricals"),
    (dict(categoricals=[0, 1.5], catlevels=[2, 2]), ValueError, "categoricals"),
    (dict(categoricals=[0, 1], catlevels=[2, 0]), ValueError, "catlevels"),
    (dict(categoricals=[0, 1], catlevels=[2, 2.0]), ValueError, "catlevels"),
    (dict(categoricals=[0, 1], catlevels=[2, 2], catvdeqs=[nf.nets.Dequantization()] * 2), TypeError, "one module covers all"),
    (dict(categoricals=[0, 1], catlevels=[2, 2], catvdeqs=(nf.nets.Dequantization(),)), TypeError, "one module covers all"),
    (dict(categoricals=[0, 1], catlevels=[2, 2], catvdeqs="uniform"), TypeError, "catvdeqs"),
])
def test_constructor_errors(kwargs, error, word):
    with pytest.raises(error, match=word):
        nf.NormalizingFlow(_q0(), [], **kwargs)


@pytest.mark.parametrize("alpha", [-0.1, 1.0, float("nan")])
def test_bad_alpha_raises(alpha):
    with pytest.raises(ValueError):
        nf.nets.Dequantization(alpha)
    with pytest.raises(ValueError):
        nf.nets.VariationalDequantization([], alpha)


# ---------------------------------------------------------------- CPU tensors: the composition
class _ShiftFlow(nf.flows.Flow):
    """A torch flow with a context, to stand between prepare and merge on the CPU."""
    takes_context = True

    def __init__(self):
        super().__init__()
        self.scale = torch.nn.Parameter(torch.tensor(0.3, dtype=torch.float64))

    def forward(self, z, context=None):
        return z * torch.exp(self.scale) + context, self.scale * z.shape[1] * torch.ones(len(z), dtype=z.dtype)

    def inverse(self, z, context=None):
        return (z - context) * torch.exp(-self.scale), -self.scale * z.shape[1] * torch.ones(len(z), dtype=z.dtype)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("alpha", [1e-5, 0.05, 0.0])
@pytest.mark.parametrize("name", list(ref.cases()))
def test_cpu_tensors_take_the_composition_with_the_restatements_bits(name, alpha, dtype):
    b, d, columns, levels = ref.cases()[name]
    x = ref.rows(b, d, columns, levels, 5, dtype)
    u = torch.rand(b, len(columns), dtype=torch.float64, generator=torch.Generator().manual_seed(6)).to(dtype)
    uniform, variational = nf.nets.Dequantization(alpha), nf.nets.VariationalDequantization([], alpha)
    out, ld = uniform.dequantize(x, columns, levels, noise=u)
    want, want_ld = ref.merge(x, columns, levels, u, False, alpha)
    assert out.dtype == dtype and ld.shape == (b,) and torch.equal(out, want) and torch.equal(ld, want_ld)
    v, ctx, ld_p = ref.prepare(x, columns, levels, u, alpha)
    out, ld = variational.dequantize(x, columns, levels, noise=u)
    want, want_ld = ref.merge(x, columns, levels, v, True, alpha)
    assert torch.equal(out, want) and torch.equal(ld, -(-ld_p - want_ld))
    codes, ld = uniform.quantize(want, columns, levels)
    want_codes, want_ld = ref.quantize(want, columns, levels, alpha)
    assert torch.equal(codes, want_codes) and torch.equal(ld, want_ld)
    # the accumulating form, a transposed (non-contiguous) input, drawn noise under one seed
    log_q = torch.arange(b, dtype=dtype)
    out2, got = uniform.dequantize(x, columns, levels, noise=u, log_q=log_q)
    assert got is log_q and torch.equal(log_q, torch.arange(b, dtype=dtype) + ref.merge(x, columns, levels, u, False, alpha)[1])
    xt = x.t().contiguous().t()
    assert torch.equal(uniform.dequantize(xt, columns, levels, noise=u)[0], ref.merge(x, columns, levels, u, False, alpha)[0])
    torch.manual_seed(9)
    a = variational.dequantize(x, columns, levels)
    torch.manual_seed(9)
    assert torch.equal(a[0], variational.dequantize(x, columns, levels, noise=torch.rand(b, len(columns), dtype=dtype))[0])
    with pytest.raises(ValueError):
        uniform.dequantize(x, columns, levels, noise=torch.rand(b, len(columns) + 1, dtype=dtype))


def test_cpu_composition_is_differentiable_in_the_flows_and_takes_the_context():
    b, d, columns, levels = ref.cases()["first_and_last"]
    x = ref.rows(b, d, columns, levels, 7)
    u = torch.rand(b, 2, dtype=torch.float64, generator=torch.Generator().manual_seed(8))
    flow = _ShiftFlow()
    vdq = nf.nets.VariationalDequantization([flow], 0.05)
    out, ld = vdq.dequantize(x, columns, levels, noise=u)
    v, ctx, ld_p = ref.prepare(x, columns, levels, u, 0.05)
    w, ld_f = flow(v, context=ctx)
    want, ld_m = ref.merge(x, columns, levels, w, True, 0.05)
    assert torch.equal(out, want) and (ld - (ld_p + ld_f + ld_m)).abs().max().item() <= 1e-12
    g_out, g_ld = torch.randn(b, d, dtype=torch.float64), torch.randn(b, dtype=torch.float64)
    got, = torch.autograd.grad((out * g_out).sum() + (ld * g_ld).sum(), flow.scale)
    want_g, = torch.autograd.grad((want * g_out).sum() + ((ld_p + ld_f + ld_m) * g_ld).sum(), flow.scale)
    assert got.item() != 0.0 and abs(got.item() - want_g.item()) <= 1e-10 * (1 + abs(want_g.item()))


def test_model_on_cpu_rows_adds_the_log_dets_and_quantises_samples():
    """The container's plumbing with a base that computes on the CPU."""
    class Base(torch.nn.Module):
        def log_prob(self, z):
            return -0.5 * (z ** 2).sum(1)

        def forward(self, n):
            z = torch.randn(n, 6, dtype=torch.float64, generator=torch.Generator().manual_seed(11))
            return z, self.log_prob(z)

    columns, levels = [0, 2, 5], [3, 2, 7]
    model = nf.NormalizingFlow(Base(), [], categoricals=columns, catlevels=levels, catvdeqs=nf.nets.VariationalDequantization([]))
    x = ref.rows(33, 6, columns, levels, 12)
    u = 0.05 + 0.9 * torch.rand(33, 3, dtype=torch.float64, generator=torch.Generator().manual_seed(13))
    xt, ld = model.dequantize(x, noise=u)
    assert torch.equal(model.log_prob(x, noise=u), ld + Base().log_prob(xt))
    assert torch.equal(model.forward_kld(x, noise=u), -torch.mean(ld + Base().log_prob(xt)))
    loss, zs, lds, log_q = model.forward_kld(x, extended=True, noise=u)
    assert zs == [] and lds == [] and torch.equal(log_q, Base().log_prob(xt) + ld)
    z, log_q = model.sample(20)
    z0, lq0 = Base()(20)
    want, ld_q = ref.quantize(z0, columns, levels)
    assert torch.equal(z, want) and torch.equal(log_q, lq0 - ld_q)
    codes = z[:, columns]
    assert torch.equal(codes, codes.round()) and bool((codes >= 0).all()) and bool((codes <= torch.tensor(levels) - 1).all())
    assert torch.equal(model.quantize(xt)[0], x)
