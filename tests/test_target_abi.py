"""Target densities without a GPU: the vcnf_target_log_prob_* symbols are exported and bound, their host-side argument
validation returns the documented status codes before anything is launched, the modules carry the reference's attribute
and buffer names, state_dict keys, dtypes and error strings, CPU tensors are refused, and the plain-torch restatement the
GPU tests compare against (target_ref.py) is itself pinned in fp64: normalisation, symmetries, the bound rejection
sampling assumes, the closed-form scores of include/vcnf_hip.h against autograd, and how few draws of the acceptance
test fall near a tie."""
import ctypes
import math

import pytest
import torch

import target_ref as ref
import vcnf_amd as nf
from helpers import assert_close
from vcnf_amd import _lib

FAKE = ctypes.c_void_p(0x1000)         # never dereferenced: validation fails first / batch == 0
ODD = ctypes.c_void_p(0x1002)          # not aligned to a float or a double
PIN = dict(rtol=1e-10, atol=1e-10)
TIE_SHARE = 0.002


def test_symbols_exported_and_bound():
    handle = ctypes.CDLL(_lib.lib_path())
    for name in ("vcnf_target_log_prob_f32", "vcnf_target_log_prob_f64"):
        assert hasattr(handle, name), "libvcnf_hip.so does not export " + name
        assert name in _lib.PROTOTYPES and getattr(nf.lib(), name).argtypes == _lib.PROTOTYPES[name][0]
    assert _lib.PROTOTYPES["vcnf_target_log_prob_f32"][0][7] is ctypes.c_float
    assert _lib.PROTOTYPES["vcnf_target_log_prob_f64"][0][7] is ctypes.c_double
    assert (_lib.TARGET_TWO_MOONS, _lib.TARGET_CIRCULAR_GMM, _lib.TARGET_RING_MIXTURE) == (0, 1, 2)
    assert callable(_lib.target_log_prob)


def _call(L, sfx, z=FAKE, table=FAKE, logp=FAKE, score=FAKE, b=4, n=3, family=1):
    return getattr(L, "vcnf_target_log_prob" + sfx)(z, table, logp, score, b, n, family, 0.5, None)


@pytest.mark.parametrize("sfx", ["_f32", "_f64"])
def test_validation_status_codes(sfx):
    L = nf.lib()
    for family in (0, 1, 2):
        assert _call(L, sfx, family=family, z=None) == 1                 # NULL required pointer
        assert _call(L, sfx, family=family, logp=None) == 1
        assert _call(L, sfx, family=family, b=-1) == 2
        for name in ("z", "table", "logp", "score"):                     # misaligned buffer
            assert _call(L, sfx, family=family, **{name: ODD}) == 3, name
        assert _call(L, sfx, family=family, b=0) == 0                    # empty batch: no launch
        assert _call(L, sfx, family=family, b=0, score=None) == 0
    for family in (1, 2):
        assert _call(L, sfx, family=family, table=None) == 1
        assert _call(L, sfx, family=family, n=0) == 2 and _call(L, sfx, family=family, n=-5) == 2
        assert _call(L, sfx, family=family, n=1 << 30, b=0) == 0         # no upper limit on the components
    assert _call(L, sfx, family=0, table=None, n=0, b=0) == 0            # TwoMoons ignores table and n_comp
    assert _call(L, sfx, family=0, table=None, n=-1, z=None) == 1
    for family in (3, -1, 1 << 20):
        assert _call(L, sfx, family=family) == 5 and _call(L, sfx, family=family, b=0) == 5


# ---------------------------------------------------------------- the modules
def test_target_base_class():
    D = nf.distributions
    assert D.target.Target is D.Target and D.target.TwoMoons is D.TwoMoons
    assert D.target.CircularGaussianMixture is D.CircularGaussianMixture and D.target.RingMixture is D.RingMixture
    t = D.Target()
    assert list(t.state_dict()) == ["prop_scale", "prop_shift"] and list(dict(t.named_buffers())) == ["prop_scale", "prop_shift"]
    assert float(t.prop_scale) == 6.0 and float(t.prop_shift) == -3.0
    assert t.prop_scale.dtype == t.prop_shift.dtype == torch.float32 and t.prop_scale.dim() == 0
    assert not list(t.parameters())
    with pytest.raises(NotImplementedError, match="The log probability is not implemented yet."):
        t.log_prob(torch.zeros(3, 2))
    t = D.Target(prop_scale=torch.tensor(4.0), prop_shift=torch.tensor(-2.0))
    assert float(t.prop_scale) == 4.0 and float(t.prop_shift) == -2.0
    assert t.double().prop_scale.dtype == torch.float64


def test_module_attributes_and_state_dicts():
    D = nf.distributions
    t = D.TwoMoons()
    assert isinstance(t, D.Target) and t.n_dims == 2 and t.max_log_prob == 0.0
    assert list(t.state_dict()) == ["prop_scale", "prop_shift"] and not list(t.parameters())

    assert D.CircularGaussianMixture().n_modes == 8
    for n in (2, 8, 33):
        t = D.CircularGaussianMixture(n)
        assert isinstance(t, D.Target) and t.n_dims == 2 and t.n_modes == n and not hasattr(t, "max_log_prob")
        assert list(t.state_dict()) == ["prop_scale", "prop_shift", "scale"] and not list(t.parameters())
        assert t.scale.dim() == 0 and t.scale.dtype == ref.scale_of("circular", n).dtype
        assert float(t.scale) == 2 / 3 * math.sin(math.pi / n) == float(ref.scale_of("circular", n))
        # the centres: fp64, a buffer that follows the module but is no part of the state dict
        table = dict(t.named_buffers())["table"]
        assert table.dtype == torch.float64 and tuple(table.shape) == (n, 2)
        want = torch.tensor([[2 * math.sin(2 * math.pi / n * i), 2 * math.cos(2 * math.pi / n * i)] for i in range(n)], dtype=torch.float64)
        assert_close(table, want, rtol=0.0, atol=4e-16, what="centres")         # one ulp of 2: numpy's sin against libm's
        t.double()
        assert t.scale.dtype == t.prop_scale.dtype == torch.float64 and float(t.scale) == 2 / 3 * math.sin(math.pi / n)

    assert D.RingMixture().n_rings == 2
    for n in (1, 2, 7):
        t = D.RingMixture(n)
        assert isinstance(t, D.Target) and t.n_dims == 2 and t.n_rings == n and t.max_log_prob == 0.0
        assert isinstance(t.scale, float) and t.scale == 1 / 4 / n == ref.scale_of("ring", n)
        assert list(t.state_dict()) == ["prop_scale", "prop_shift"] and not list(t.parameters())
        table = dict(t.named_buffers())["table"]
        assert table.dtype == torch.float64 and table.tolist() == [2 / n * (i + 1) for i in range(n)]
        assert t.double().prop_scale.dtype == torch.float64


def test_model_state_dict_has_the_reference_keys():
    from vcnf_amd.flows import Planar
    D = nf.distributions
    for target, extra in ((D.TwoMoons(), []), (D.CircularGaussianMixture(), ["p.scale"]), (D.RingMixture(), [])):
        model = nf.NormalizingFlow(D.DiagGaussian(2), [Planar(2) for _ in range(2)], target)
        assert model.p is target
        assert [k for k in model.state_dict() if k.startswith("p.")] == ["p.prop_scale", "p.prop_shift"] + extra
        other = nf.NormalizingFlow(D.DiagGaussian(2), [Planar(2) for _ in range(2)], type(target)())
        other.load_state_dict(model.state_dict())


def test_cpu_tensors_and_bad_inputs_are_refused():
    D = nf.distributions
    z = torch.zeros(3, 2)
    for t in (D.TwoMoons(), D.CircularGaussianMixture(), D.RingMixture()):
        for call in (t.log_prob, t.score):
            with pytest.raises(nf.VcnfError):
                call(z)
            with pytest.raises(nf.VcnfError):
                call(z.double())
    for t in (D.TwoMoons(), D.RingMixture()):
        with pytest.raises(nf.VcnfError):
            t.rejection_sampling(4)
        with pytest.raises(nf.VcnfError):
            t.sample(4)


def test_circular_mixture_samples_without_the_kernel():
    """Its sample is draws and a table lookup: [N, 2] in the dtype of prop_scale, every row near a centre."""
    t = nf.distributions.CircularGaussianMixture(8)
    torch.manual_seed(3)
    for dtype in (torch.float32, torch.float64):
        t = t.to(dtype)
        z = t.sample(4000)
        assert tuple(z.shape) == (4000, 2) and z.dtype == dtype and torch.isfinite(z).all()
        dist = torch.cdist(z.double(), dict(t.named_buffers())["table"].double()).min(1)[0]
        assert float(dist.max()) < 7 * float(t.scale)


# ---------------------------------------------------------------- the restatement, pinned
def _grid(lo, hi, n):
    """Midpoints of an n x n grid over [lo, hi]^2 as rows [n, 2] per grid row (one chunk per grid row), and a cell's area."""
    h = (hi - lo) / n
    mid = lo + h * (torch.arange(n, dtype=torch.float64) + 0.5)
    return mid, h * h


def _mass_in_box(n, lo, hi):
    """What a mixture of n isotropic Gaussians of the reference's scale on the circle of radius 2 has inside [lo, hi]^2,
    from the normal CDF: the yardstick of the grid sum."""
    s = 2 / 3 * math.sin(math.pi / n)
    cdf = lambda x: 0.5 * (1.0 + math.erf(x / math.sqrt(2.0)))
    side = lambda c: cdf((hi - c) / s) - cdf((lo - c) / s)
    return sum(side(2 * math.sin(2 * math.pi / n * i)) * side(2 * math.cos(2 * math.pi / n * i)) for i in range(n)) / n


@pytest.mark.parametrize("n", [2, 8])
def test_circular_mixture_integrates_to_one(n):
    """exp(log_prob) on a 2000^2 midpoint grid over [-5, 5]^2 sums to the mixture's mass in that box within 1e-6.  That
    mass is 1 to 1e-12 for 8 modes; the two modes of n = 2 are wide (scale 2/3, centres (0, +-2)) and leave 3.4e-6
    beyond |z1| = 5, 4.5 standard deviations out, so 1 itself is not what a correct density sums to there."""
    mid, area = _grid(-5.0, 5.0, 2000)
    total = 0.0
    for rows in mid.split(100):                     # 100 grid rows = 200 000 points per chunk
        z = torch.cartesian_prod(rows, mid)
        total += float(torch.exp(ref.log_prob("circular", n, z)).sum()) * area
    inside = _mass_in_box(n, -5.0, 5.0)
    assert 1.0 - 4e-6 <= inside <= 1.0 and (n == 2 or 1.0 - inside <= 1e-12)
    assert abs(total - inside) <= 1e-6, (total, inside)


def test_symmetries():
    z, _, _, _ = ref.inputs("two_moons", 0, 1000)
    flip = z * torch.tensor([-1.0, 1.0], dtype=torch.float64)
    assert torch.equal(ref.log_prob("two_moons", 0, z), ref.log_prob("two_moons", 0, flip))
    for n in (1, 2, 7):
        z, _, _, _ = ref.inputs("ring", n, 1000)
        for phi in (0.3, 1.0, 2.5):
            rot = torch.tensor([[math.cos(phi), -math.sin(phi)], [math.sin(phi), math.cos(phi)]], dtype=torch.float64)
            # log p moves with r by (t - r) / scale^2 <= 8.5 * 784 per unit, and r itself by a few ulps
            assert_close(ref.log_prob("ring", n, z @ rot.T), ref.log_prob("ring", n, z), rtol=1e-10, atol=1e-10, what="rotation")


@pytest.mark.parametrize("family,n", [("two_moons", 0), ("ring", 1), ("ring", 2), ("ring", 7)])
def test_density_stays_under_max_log_prob_on_the_proposal_box(family, n):
    mid, _ = _grid(ref.PROP_SHIFT, ref.PROP_SHIFT + ref.PROP_SCALE, 1000)
    lp = ref.log_prob(family, n, torch.cartesian_prod(mid, mid))
    assert torch.isfinite(lp).all() and float(lp.max()) <= ref.MAX_LOG_PROB + 1e-6, float(lp.max())


def _unit(z, r):
    """z / r with 0 at r == 0."""
    return torch.where(r > 0, z / torch.where(r > 0, r, torch.ones_like(r)), torch.zeros_like(z))


def closed_form_score(family, n, z):
    """The scores as include/vcnf_hip.h states them, in plain torch."""
    z0, z1 = z[:, 0], z[:, 1]
    r = torch.sqrt(z0 ** 2 + z1 ** 2)
    if family == "two_moons":
        a = z0.abs()
        e = torch.exp(-4 * a / 0.09)
        k = -(r - 2) / 0.04
        s0 = k * _unit(z0, r) + torch.sign(z0) * ((2 - a) / 0.09 - (4 / 0.09) * e / (1 + e))
        return torch.stack([s0, k * _unit(z1, r)], 1)
    if family == "circular":
        scale = float(ref.scale_of(family, n))
        i = torch.arange(n, dtype=torch.float64)
        c = torch.stack([2 * torch.sin(2 * math.pi * i / n), 2 * torch.cos(2 * math.pi * i / n)], 1)
        diff = c[None] - z[:, None]                                       # [B, n, 2]
        w = torch.softmax(-(diff ** 2).sum(2) / (2 * scale ** 2), 1)
        return (w[:, :, None] * diff).sum(1) / scale ** 2
    scale = ref.scale_of(family, n)
    t = 2 * (torch.arange(n, dtype=torch.float64) + 1) / n
    w = torch.softmax(-(r[:, None] - t[None]) ** 2 / (2 * scale ** 2), 1)
    k = (w * (t[None] - r[:, None])).sum(1) / scale ** 2
    return torch.stack([k * _unit(z0, r), k * _unit(z1, r)], 1)


@pytest.mark.parametrize("family,n", [("two_moons", 0), ("circular", 2), ("circular", 8), ("circular", 33),
                                      ("ring", 1), ("ring", 2), ("ring", 7)])
def test_closed_form_scores_are_autograds(family, n):
    z, _, _, _ = ref.inputs(family, n, 1000)
    assert float(torch.norm(z[0])) == 0.0                                 # the r == 0 row is in
    want = ref.score(family, n, z)
    got = closed_form_score(family, n, z)
    assert torch.isfinite(want).all()
    assert_close(got, want, what="%s n=%d closed-form score" % (family, n), **PIN)
    if family != "circular":
        assert want[0].tolist() == [0.0, 0.0] and got[0].tolist() == [0.0, 0.0]
    if family == "two_moons":
        assert float(want[6, 0]) == 0.0 and float(got[6, 0]) == 0.0       # z0 == -0.: the bracket is 0 there


@pytest.mark.parametrize("family,n", [("two_moons", 0), ("ring", 2)])
def test_few_draws_fall_near_a_tie(family, n):
    """Measured on the CPU over 200 000 draws: 0.014 % (TwoMoons) and 0.034 % (rings)."""
    _, _, eps, u = ref.inputs(family, n, 1000)
    assert len(u) == ref.DRAWS == 20000
    _, accept, near = ref.accept(family, n, eps, u)
    print("%s: accepted %.2f %%, near a tie %.3f %%" % (family, 100 * float(accept.double().mean()), 100 * float(near.double().mean())))
    assert 0.01 < float(accept.double().mean()) < 0.5
    assert float(near.double().mean()) <= TIE_SHARE
