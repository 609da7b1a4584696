"""Planar and Radial flows without a GPU: the vcnf_planar_radial_* symbols are exported and bound, their host-side argument
validation returns the documented status codes before anything is launched, the workspace size is a pure, bounded function
of the shape, the modules carry the stated parameter names, shapes, dtypes, initial ranges and error strings, CPU tensors
are refused, and the plain-torch restatement the GPU tests compare against (planar_radial_ref.py) is itself pinned in fp64:
its log_det against the Jacobian autograd builds, its leaky_relu inverse against its forward."""
import ctypes
import math

import pytest
import torch

import planar_radial_ref as ref
import vcnf_amd as nf
from helpers import assert_close
from vcnf_amd import _lib

FAKE = ctypes.c_void_p(0x1000)         # never dereferenced: validation fails first / batch == 0
ODD = ctypes.c_void_p(0x1002)          # not aligned to a float or a double
PIN = dict(rtol=1e-10, atol=1e-10)
LIMIT = 256


def kinds(*ks):
    return (ctypes.c_int32 * len(ks))(*ks)


def test_symbols_exported_and_bound():
    handle = ctypes.CDLL(_lib.lib_path())
    names = ["vcnf_planar_radial_stack%s%s" % (k, sfx) for k in ("", "_bwd") for sfx in ("_f32", "_f64")]
    for name in names + ["vcnf_planar_radial_supported", "vcnf_planar_radial_bwd_groups", "vcnf_planar_radial_checkpoint_every"]:
        assert hasattr(handle, name), "libvcnf_hip.so does not export " + name
        assert name in _lib.PROTOTYPES and getattr(nf.lib(), name).argtypes == _lib.PROTOTYPES[name][0]
    assert (_lib.PLANAR_TANH, _lib.PLANAR_LEAKY, _lib.RADIAL) == (0, 1, 2)
    assert callable(_lib.planar_radial_stack) and callable(_lib.planar_radial_stack_bwd)


def _fwd(L, sfx, z=FAKE, kind=kinds(0, 1, 2), b=4, d=8, k=3, inverse=0, ld_mode=0, out=FAKE, logdet=FAKE, vb=FAKE):
    return getattr(L, "vcnf_planar_radial_stack" + sfx)(z, out, logdet, None, None, kind, FAKE, FAKE, vb, FAKE, b, d, k, inverse,
                                                        ld_mode, 1.0, None)


def _bwd(L, sfx, z=FAKE, kind=kinds(0, 1, 2), b=4, d=8, k=3, g_out=FAKE, g_ld=FAKE, work=FAKE):
    return getattr(L, "vcnf_planar_radial_stack_bwd" + sfx)(z, FAKE, None, g_out, g_ld, kind, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE,
                                                            FAKE, FAKE, work, b, d, k, None)


@pytest.mark.parametrize("sfx", ["_f32", "_f64"])
def test_validation_status_codes(sfx):
    L = nf.lib()
    for call in (_fwd, _bwd):
        assert call(L, sfx, z=None) == 1                             # NULL required pointer
        assert call(L, sfx, kind=None) == 1
        assert call(L, sfx, b=-1) == 2
        assert call(L, sfx, d=0) == 2 and call(L, sfx, d=LIMIT + 1) == 2
        assert call(L, sfx, k=0) == 2
        assert call(L, sfx, z=ODD) == 3                              # misaligned buffer
        assert call(L, sfx, kind=kinds(0, 3, 2)) == 5 and call(L, sfx, kind=kinds(-1, 1, 2)) == 5      # unknown kind
        assert call(L, sfx, b=0) == 0                                # empty batch: no launch
        assert call(L, sfx, b=0, d=LIMIT) == 0
    assert _fwd(L, sfx, out=None) == 1 and _fwd(L, sfx, logdet=None) == 1
    assert _fwd(L, sfx, vb=None) == 1 and _fwd(L, sfx, vb=None, kind=kinds(2, 2, 2), b=0) == 0       # vb: planar rows only
    assert _fwd(L, sfx, ld_mode=2) == 5                              # unknown ld_mode
    assert _fwd(L, sfx, inverse=1) == 5 and _fwd(L, sfx, inverse=1, kind=kinds(1, 1, 0)) == 5          # inverse: kind 1 only
    assert _fwd(L, sfx, inverse=1, kind=kinds(1, 1, 1), b=0) == 0
    assert _bwd(L, sfx, work=None) == 1
    assert _bwd(L, sfx, g_out=ODD) == 3


def test_bwd_groups_and_supported():
    L = nf.lib()
    assert [L.vcnf_planar_radial_supported(d) for d in (-1, 0, 1, 2, 255, LIMIT, LIMIT + 1, 1 << 20)] == [0, 0, 1, 1, 1, 1, 0, 0]
    for b in (1, 63, 64, 65, 1000, 4096, 1 << 20, 1 << 40):
        for d in (1, 2, 5, 17, 130, LIMIT):
            for k in (1, 33, 200, 100000):
                g = L.vcnf_planar_radial_bwd_groups(b, d, k)
                assert g == L.vcnf_planar_radial_bwd_groups(b, d, k)                 # pure
                assert 1 <= g <= 1024                                                 # bounded
                assert g == 1 or g * k * (2 * d + 2) <= 1 << 22                       # and so is the workspace
    # the row checkpoints of the VJP are O(B K) like its trace: (K - 1) / every rows of D, at most 8 K values per sample
    assert [L.vcnf_planar_radial_checkpoint_every(d) for d in (0, 1, 4, 5, 32, 33, 64, 130, LIMIT, LIMIT + 1)] == [0, 4, 4, 4, 4, 5, 8, 17, LIMIT // 8, 0]
    assert all(d <= 8 * L.vcnf_planar_radial_checkpoint_every(d) for d in range(1, LIMIT + 1))
    assert L.vcnf_planar_radial_bwd_groups(1, 2, 1) == 1
    assert L.vcnf_planar_radial_bwd_groups(1 << 30, 2, 1) == 1024
    for bad in ((-1, 2, 1), (4, 0, 1), (4, LIMIT + 1, 1), (4, 2, 0)):
        assert L.vcnf_planar_radial_bwd_groups(*bad) == 0


# ---------------------------------------------------------------- the modules
@pytest.mark.parametrize("shape", [2, (7,), (2, 3, 3)])
def test_planar_module(shape):
    from vcnf_amd.flows import Planar
    tup = (shape,) if isinstance(shape, int) else tuple(shape)
    d = math.prod(tup)
    torch.manual_seed(5)
    for act in ("tanh", "leaky_relu"):
        for _ in range(20):
            f = Planar(shape, act=act)
            sd = f.state_dict()
            assert list(sd) == ["u", "w", "b"]
            assert tuple(sd["u"].shape) == (1,) + tup and tuple(sd["w"].shape) == (1,) + tup and tuple(sd["b"].shape) == (1,)
            assert all(v.dtype == torch.float32 for v in sd.values())
            assert all(isinstance(p, torch.nn.Parameter) and p.requires_grad for p in (f.u, f.w, f.b))
            assert float(sd["u"].abs().max()) <= math.sqrt(2.0) and float(sd["w"].abs().max()) <= math.sqrt(2.0 / d)
            assert float(sd["b"]) == 0.0
    u, w, b = torch.randn(1, *tup), torch.randn(1, *tup), torch.randn(1)
    f = Planar(shape, u=u, w=w, b=b)
    assert torch.equal(f.u.data, u) and torch.equal(f.w.data, w) and torch.equal(f.b.data, b)
    assert f.double().u.dtype == torch.float64


@pytest.mark.parametrize("shape", [2, (7,), (2, 3, 3)])
def test_radial_module(shape):
    from vcnf_amd.flows import Radial
    tup = (shape,) if isinstance(shape, int) else tuple(shape)
    d = math.prod(tup)
    torch.manual_seed(6)
    for _ in range(20):
        f = Radial(shape)
        sd = f.state_dict()
        # parameters before buffers, as torch orders every state dict (the reference's own modules included)
        assert list(sd) == ["beta", "alpha", "z_0", "d"] and list(f._parameters) == ["beta", "alpha", "z_0"]
        assert tuple(sd["beta"].shape) == (1,) and tuple(sd["alpha"].shape) == (1,) and tuple(sd["z_0"].shape) == (1,) + tup
        assert sd["d"].dtype == torch.int64 and sd["d"].dim() == 0 and int(sd["d"]) == d
        assert all(sd[n].dtype == torch.float32 for n in ("alpha", "beta", "z_0"))
        assert -1.0 / d - 1.0 <= float(sd["beta"]) <= 1.0 / d - 1.0
        assert -1.0 / d <= float(sd["alpha"]) <= 1.0 / d
    z_0 = torch.randn(1, *tup)
    assert torch.equal(Radial(shape, z_0=z_0).z_0.data, z_0)
    f = Radial(shape).double()
    assert f.z_0.dtype == torch.float64 and f.d.dtype == torch.int64


def test_error_strings_and_cpu_tensors():
    from vcnf_amd.flows import Planar, Radial
    with pytest.raises(NotImplementedError, match="Nonlinearity is not implemented."):
        Planar(2, act="relu")
    z = torch.zeros(3, 2)
    with pytest.raises(NotImplementedError, match="This flow has no algebraic inverse."):
        Planar(2).inverse(z)
    with pytest.raises(NotImplementedError, match="This flow has no algebraic inverse."):
        Radial(2).inverse(z)
    for call in (Planar(2), Planar(2, act="leaky_relu"), Planar(2, act="leaky_relu").inverse, Radial(2)):
        with pytest.raises(nf.VcnfError):
            call(z)
    model = nf.NormalizingFlow(nf.distributions.DiagGaussian(2), [Planar(2), Radial(2)])
    assert model.fuse_planar_stacks is True
    with pytest.raises(nf.VcnfError):
        model.sample_from(z)
    assert nf.flows.Planar is Planar and nf.flows.Radial is Radial


@pytest.mark.parametrize("shape", [3, (2, 3, 3)])
def test_torch_composition_is_the_restatement_in_fp64(shape):
    """What the layers evaluate beyond the kernel's feature limit (and the inverse under autograd) computes in the
    parameters' dtype throughout: in fp64 it equals the restatement to a few roundings."""
    from vcnf_amd.flows import Planar, Radial
    layers, z, _, _ = ref.inputs("mixed", shape, 3, 65)
    tight = dict(rtol=1e-14, atol=1e-14)
    for p in layers:
        if p["kind"] == "radial":
            f = Radial(shape, z_0=p["z_0"].clone())
            f.alpha.data, f.beta.data = p["alpha"].clone(), p["beta"].clone()
        else:
            f = Planar(shape, act=p["kind"], u=p["u"].clone(), w=p["w"].clone(), b=p["b"].clone())
        with torch.no_grad():
            out, log_det = f._torch_forward(z)
            want = ref.layer_forward(z, p)
            assert out.dtype == log_det.dtype == torch.float64
            assert_close(out, want[0], what=p["kind"] + " composition z", **tight)
            assert_close(log_det, want[1], what=p["kind"] + " composition log_det", **tight)
            if p["kind"] == "leaky_relu":
                back, log_det = f._torch_inverse(z)
                want = ref.planar_inverse(z, p)
                assert_close(back, want[0], what="composition inverse z", **tight)
                assert_close(log_det, want[1], what="composition inverse log_det", **tight)


# ---------------------------------------------------------------- the restatement, pinned
@pytest.mark.parametrize("d", [1, 2, 5])
@pytest.mark.parametrize("kind", ref.KINDS)
def test_restatement_log_det_is_the_jacobians(kind, d):
    g = torch.Generator().manual_seed(ref.seed_of("pin", kind, d))
    for _ in range(4):
        p = ref.make_layer(kind, (d,), g)
        z = torch.randn(6, d, generator=g, dtype=torch.float64)
        _, log_det, _ = ref.layer_forward(z, p)
        assert torch.isfinite(log_det).all()
        for i in range(len(z)):
            jac = torch.autograd.functional.jacobian(lambda x: ref.layer_forward(x[None], p)[0][0], z[i])
            assert_close(log_det[i], torch.linalg.slogdet(jac)[1], what="%s D=%d log_det vs Jacobian" % (kind, d), **PIN)


@pytest.mark.parametrize("d", [1, 2, 5, 17])
def test_restatement_inverse_undoes_forward(d):
    layers, z, _, _ = ref.inputs("leaky_relu", d, 5, 64)
    out, log_det, _ = ref.forward(z, layers)
    back, log_det_inv = ref.inverse(out, layers)
    assert torch.isfinite(out).all() and torch.isfinite(log_det).all()
    assert_close(back, z, what="inverse(forward(z))", **PIN)
    assert_close(log_det + log_det_inv, torch.zeros_like(log_det), what="log-dets sum to zero", **PIN)


def test_restatement_leaves_few_rows_out():
    """The rows near a kink are few on the shapes of the GPU tests."""
    for d in (1, 2, 3, 5, 16, 17, 64, 65, 130):
        for stack in ("leaky_relu", "radial", "mixed"):
            layers, z, _, _ = ref.inputs(stack, d, 33, 1000)
            out, log_det, trace = ref.forward(z, layers)
            assert torch.isfinite(out).all() and torch.isfinite(log_det).all()
            assert float(ref.kink_rows(trace, layers).double().mean()) <= 0.02, (stack, d)
