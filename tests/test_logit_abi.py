"""Image data end caps without a GPU: the vcnf_logit_* symbols are declared in the header, exported and bound, their
host-side validation returns the documented status codes in the documented order before anything is launched, the public
classes exist with the stated defaults, CPU tensors get the values of the plain-torch restatement (logit_ref.py) bit for
bit, and byte input without a Logit transform is refused.  No call here passes validation with work to do: nothing is
ever launched on the fake pointers."""
import ctypes
import math
import os

import pytest
import torch

import logit_ref as ref
import vcnf_amd as nf
from vcnf_amd import _lib

FAKE = ctypes.c_void_p(0x1000)         # never dereferenced: validation fails first / the batch is empty
ODD = ctypes.c_void_p(0x1002)          # not aligned to a float or a double
STEMS = ("vcnf_logit_inverse", "vcnf_logit_forward", "vcnf_logit_inverse_bwd", "vcnf_logit_forward_bwd",
         "vcnf_logit_inverse_u8")
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
        for stem, n_args, n_double in (("vcnf_logit_inverse", 9, 1), ("vcnf_logit_forward", 9, 1), ("vcnf_logit_inverse_bwd", 8, 1),
                                       ("vcnf_logit_forward_bwd", 8, 1), ("vcnf_logit_inverse_u8", 12, 3)):
            args = _lib.PROTOTYPES[stem + sfx][0]
            assert len(args) == n_args, stem + sfx
            # alpha (jitter, scale) cross the ABI in fp64 for both element types; ld_sign has the element type
            extra = 1 if (scalar is ctypes.c_double and not stem.endswith("_bwd")) else 0
            assert sum(a is ctypes.c_double for a in args) == n_double + extra, stem + sfx
            if not stem.endswith("_bwd"):
                assert args[-2] is scalar, stem + sfx
    for wrapper in ("logit", "logit_bwd", "logit_inverse_u8"):
        assert callable(getattr(_lib, wrapper))


def _direction(stem):
    def call(L, sfx, x=FAKE, out=FAKE, ld=FAKE, b=4, d=3, mode=0):
        return getattr(L, stem + sfx)(x, 0.05, out, ld, b, d, mode, 1.0, None)
    return call


def _bwd(stem):
    def call(L, sfx, x=FAKE, g_out=FAKE, g_ld=FAKE, d_x=FAKE, b=4, d=3):
        return getattr(L, stem + sfx)(x, 0.05, g_out, g_ld, d_x, b, d, None)
    return call


def _u8(L, sfx, x=FAKE, noise=FAKE, out=FAKE, ld=FAKE, b=4, d=3, mode=0):
    return getattr(L, "vcnf_logit_inverse_u8" + sfx)(x, noise, 1 / 256., 255 / 256., 0.05, out, ld, b, d, mode, 1.0, None)


# name -> (call, required pointers, optional pointers, pointers held to the element's alignment, has an ld_mode)
CALLS = {"inverse": (_direction("vcnf_logit_inverse"), ("x", "out", "ld"), (), ("x", "out", "ld"), True),
         "forward": (_direction("vcnf_logit_forward"), ("x", "out", "ld"), (), ("x", "out", "ld"), True),
         "inverse_bwd": (_bwd("vcnf_logit_inverse_bwd"), ("x", "d_x"), ("g_out", "g_ld"), ("x", "g_out", "g_ld", "d_x"), False),
         "forward_bwd": (_bwd("vcnf_logit_forward_bwd"), ("x", "d_x"), ("g_out", "g_ld"), ("x", "g_out", "g_ld", "d_x"), False),
         "inverse_u8": (_u8, ("x", "noise", "out", "ld"), (), ("noise", "out", "ld"), True)}


@pytest.mark.parametrize("sfx", ["_f32", "_f64"])
@pytest.mark.parametrize("entry", list(CALLS))
def test_validation_status_codes_in_the_documented_order(entry, sfx):
    call, required, optional, held, has_mode = CALLS[entry]
    L = nf.lib()
    for name in required:
        assert call(L, sfx, **{name: None}) == NULL, name
        assert call(L, sfx, **{name: None}, d=0) == NULL and call(L, sfx, **{name: None}, b=0) == NULL      # NULL comes first
    for bad in (dict(d=0), dict(d=-3), dict(b=-1), dict(b=1 << 62, d=4)):                      # counts; rows * features overflows
        assert call(L, sfx, **bad) == SHAPE, bad
    # work beyond a grid: at most 256 rows of 3 elements per workgroup, 2^31 - 1 workgroups
    assert call(L, sfx, b=256 * (2 ** 31 - 1) + 1, d=3) == SHAPE
    assert call(L, sfx, b=-1, **{held[0]: ODD}) == SHAPE                                       # shape before alignment
    for name in held:
        assert call(L, sfx, **{name: ODD}) == ALIGN, name
        assert call(L, sfx, **{name: ODD}, b=0) == OK                                          # an empty batch before alignment
    assert call(L, sfx, b=0) == OK and call(L, sfx, b=0, d=1 << 30) == OK                      # any number of features
    for name in optional:
        assert call(L, sfx, **{name: None}, b=0) == OK
    if has_mode:
        assert call(L, sfx, b=0, mode=_lib.LD_STORE) == OK and call(L, sfx, b=0, mode=_lib.LD_ACCUM) == OK
        for mode in (2, -1, 1 << 20):
            assert call(L, sfx, mode=mode) == UNSUPPORTED and call(L, sfx, mode=mode, b=0) == UNSUPPORTED
            assert call(L, sfx, mode=mode, d=0) == SHAPE and call(L, sfx, mode=mode, out=None) == NULL
            assert call(L, sfx, mode=mode, out=ODD) == UNSUPPORTED


# ---------------------------------------------------------------- the public surface
def test_exports_and_defaults():
    assert issubclass(nf.transforms.Logit, nf.flows.Flow) and issubclass(nf.transforms.Shift, nf.flows.Flow)
    t = nf.transforms.Logit()
    assert t.alpha == 0.05 and isinstance(t.alpha, float) and nf.transforms.Logit(0.1).alpha == 0.1
    assert list(t.state_dict()) == [] and not list(t.parameters()) and not list(t.buffers())
    assert not t.takes_context and callable(t.forward_into) and callable(t.inverse_into) and callable(t.inverse_u8)
    s = nf.transforms.Shift()
    assert s.shift == 0. and nf.transforms.Shift(0.5).shift == 0.5 and list(s.state_dict()) == []
    assert nf.utils.Logit().alpha == 0 and nf.utils.Jitter().scale == 1 / 256 and nf.utils.Scale().scale == 255 / 256
    assert nf.utils.preprocessing.Logit is nf.utils.Logit and nf.utils.eval.bits_per_dim is nf.utils.bits_per_dim
    assert not isinstance(nf.utils.Logit(), torch.nn.Module)
    assert nf.utils.bits_per_dim(0.0, 7) == 8.0 and "reference" in nf.utils.bits_per_dim.__doc__


@pytest.mark.parametrize("alpha", [-0.01, 0.5, 0.7, float("nan")])
def test_bad_alpha_raises(alpha):
    with pytest.raises(ValueError):
        nf.transforms.Logit(alpha)


def test_alpha_edges_are_accepted():
    assert nf.transforms.Logit(0).alpha == 0.0 and nf.transforms.Logit(0.499).alpha == 0.499


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64, torch.bfloat16])
@pytest.mark.parametrize("alpha", [0.05, 1e-6, 0.0])
def test_cpu_tensors_take_the_composition_with_the_restatements_bits(alpha, dtype):
    torch.manual_seed(3)
    mine, twin = nf.transforms.Logit(alpha), ref.LogitRef(alpha)
    x = torch.rand(5, 3, 4, 4, dtype=torch.float64).to(dtype)
    x[0, 0, 0, 0], x[0, 0, 0, 1] = 0.0, 1.0
    z = (4 * torch.randn(5, 3, 4, 4, dtype=torch.float64)).to(dtype)
    z[1, 0, 0, 0], z[1, 0, 0, 1], z[2, 0, 0, 0] = 88.0, -104.0, math.inf
    for point, got, want in ((x, mine.inverse, twin.inverse), (z, mine.forward, twin.forward)):
        (a, a_ld), (b, b_ld) = got(point), want(point)
        assert a.dtype == dtype and a_ld.shape == (5,)
        assert torch.equal(a, b) and torch.equal(a_ld, b_ld)
    # non-contiguous, a single axis, an empty batch
    xt = x.transpose(2, 3)
    assert torch.equal(mine.inverse(xt)[0], twin.inverse(xt)[0])
    assert mine.inverse(x[:, 0, 0, 0])[1].shape == (5,) and mine.inverse(x[:0])[1].shape == (0,)
    # the accumulating forms
    log_q = torch.arange(5, dtype=dtype)
    out = mine.inverse_into(x, log_q)
    assert torch.equal(out, twin.inverse(x)[0]) and torch.equal(log_q, torch.arange(5, dtype=dtype) + twin.inverse(x)[1])
    log_q = torch.arange(5, dtype=dtype)
    out = mine.forward_into(z, log_q)
    assert torch.equal(out, twin.forward(z)[0])
    assert torch.equal(log_q, torch.arange(5, dtype=dtype).add_(twin.forward(z)[1], alpha=-1.0))


def test_cpu_composition_is_differentiable_in_the_input():
    torch.manual_seed(4)
    mine = nf.transforms.Logit(0.05)
    x = (torch.rand(3, 5, dtype=torch.float64) * 0.9 + 0.05).requires_grad_()
    g_z, g_ld = torch.randn(3, 5, dtype=torch.float64), torch.randn(3, dtype=torch.float64)
    z, ld = mine.inverse(x)
    got, = torch.autograd.grad((z * g_z).sum() + (ld * g_ld).sum(), x)
    assert ((got - ref.inverse_vjp(x.detach(), 0.05, g_z, g_ld)).abs() / (1 + got.abs())).max().item() <= 1e-10
    assert torch.autograd.gradcheck(lambda v: mine.forward(v), (torch.randn(3, 5, dtype=torch.float64, requires_grad=True),))


def test_shift_and_preprocessing_on_cpu():
    z = torch.randn(4, 3)
    keep = z.clone()
    for mine, twin in ((nf.transforms.Shift(0.25), ref.ShiftRef(0.25)), (nf.transforms.Shift(torch.tensor(1.5)), ref.ShiftRef(torch.tensor(1.5)))):
        for a, b in ((mine.forward(z), twin.forward(z)), (mine.inverse(z), twin.inverse(z))):
            assert torch.equal(a[0], b[0]) and torch.equal(a[1], torch.zeros(4)) and a[1].dtype == z.dtype
    assert torch.equal(z, keep), "Shift must not write into its input"
    assert nf.transforms.Shift(1.0).forward(z.double())[1].dtype == torch.float64
    x = torch.rand(4, 3)
    assert torch.equal(nf.utils.Logit(0.05)(x), ref.PreLogit(0.05)(x))
    assert torch.equal(nf.utils.Logit(0.05).inverse(z), ref.PreLogit(0.05).inverse(z))
    assert torch.allclose(nf.utils.Logit(0.05).inverse(nf.utils.Logit(0.05)(x)), x, atol=1e-6)
    assert torch.equal(nf.utils.Scale()(x), ref.Scale()(x)) and torch.equal(nf.utils.Scale(0.5)(x), x * 0.5)
    torch.manual_seed(5)
    a = nf.utils.Jitter()(x)
    torch.manual_seed(5)
    assert torch.equal(a, ref.Jitter()(x)) and bool(((a - x) >= 0).all()) and bool(((a - x) < 1 / 256).all())


def test_inverse_u8_on_cpu_is_the_chain():
    torch.manual_seed(6)
    t = nf.transforms.Logit(0.05)
    x_u8 = torch.arange(256, dtype=torch.uint8).repeat(3).reshape(4, 3, 8, 8)
    for dtype in (torch.float32, torch.float64):
        noise = torch.rand(x_u8.shape, dtype=dtype)
        z, ld = t.inverse_u8(x_u8, noise, dtype=dtype)
        want_z, want_ld = ref.inverse_u8(x_u8, noise, 0.05)
        assert z.dtype == dtype and torch.equal(z, want_z) and torch.equal(ld, want_ld)
    torch.manual_seed(7)
    z = t.inverse_u8(x_u8)[0]
    torch.manual_seed(7)
    assert torch.equal(z, t.inverse_u8(x_u8, torch.rand(x_u8.shape))[0])
    with pytest.raises(TypeError):
        t.inverse_u8(x_u8.float())
    with pytest.raises(ValueError):
        t.inverse_u8(x_u8, torch.rand(4, 3, 8, 8, dtype=torch.float64))


class _Base(torch.nn.Module):
    """Stands where a base distribution goes: log_prob must refuse the bytes before it is asked anything."""

    def from_noise(self, eps):
        raise AssertionError("not reached")


@pytest.mark.parametrize("transform", [None, nf.transforms.Shift(0.5)])
def test_multiscale_flow_refuses_bytes_without_a_logit_transform(transform):
    model = nf.MultiscaleFlow([_Base()], [[]], [], transform=transform)
    x = torch.zeros(2, 3, 8, 8, dtype=torch.uint8)
    with pytest.raises(TypeError, match="None" if transform is None else "Shift"):
        model.log_prob(x)
    with pytest.raises(TypeError, match="None" if transform is None else "Shift"):
        model.forward_kld(x)
