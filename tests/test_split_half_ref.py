"""What the fp16 split-half arithmetic of the training path's backward GEMMs does to a small cotangent, on the CPU
(tests/split_half_ref.py; no GPU): forward_kld is a mean over the batch, so the cotangents that reach
csrc/linear_f16x3.hip (input gradients) and csrc/linear_wgrad.hip (weight gradients) are of order 1/B - 2^-17 at the
benchmark's training batch, below fp16's smallest normal 2^-14.

Pinned here, in ulp of the scale (2^-24 * sum |a b|), for the shapes of profiles/grad_range.md:

* the bare split is within 4 at cotangent scales 2^0, 2^-10, 2^-14 and beyond 4 from 2^-17 on for the input gradient
  (g [2577, 128] @ w [128, 128]) and from 2^-24 on for the weight gradient (dy^T x, B = 32 805, 128 x 128);
* with the power-of-two pre-scale of split_half.hpp::pre_scale (one exponent per row of the cotangent operand) the
  result at every scale 2^0 ... 2^-60 is the result at 2^0 times that power of two, bit for bit - and within 4; so is
  a cotangent with one entry of 1e6 among entries at 2^-17.
"""
import pytest
import torch

import split_half_ref as sh

BOUND = 4.0


def _dgrad_operands():
    gen = torch.Generator().manual_seed(0)
    return torch.randn(2577, 128, generator=gen), torch.randn(128, 128, generator=gen) / 128 ** 0.5


def _wgrad_operands():
    gen = torch.Generator().manual_seed(1)
    b = 32768 + 37
    return torch.randn(b, 128, generator=gen).t().contiguous(), torch.randn(b, 128, generator=gen)     # dy^T, x


OPERANDS = {"dgrad": _dgrad_operands, "wgrad": _wgrad_operands}
_CACHE = {}


def _case(name):
    """(cotangent at 2^0, other operand, fp64 product, ulp of the scale) - computed once per shape."""
    if name not in _CACHE:
        a, b = OPERANDS[name]()
        _CACHE[name] = (a, b, a.double() @ b.double(), sh.ulp_of_scale(a, b))
    return _CACHE[name]


def _max_ulp(name, k, prescale):
    a, b, ref, ulp = _case(name)
    got = sh.product(a * 2.0 ** -k, b, prescale=prescale)
    return float(((got - ref * 2.0 ** -k).abs() / (ulp * 2.0 ** -k)).max())


def test_split_is_the_kernels_split():
    v = torch.tensor([1.0, 1.0 + 2.0 ** -11, 1.0 + 2.0 ** -12, 3.0e-5, 2.0 ** -17 * 1.2345, 7.0e4, -7.0e4, 0.0])
    hi, lo = sh.split(v)
    t = v.clamp(-65504.0, 65504.0).double()
    assert hi.tolist()[:2] == [1.0, 1.0] and lo[1] == 1.0 and hi[5] == 65504.0 and hi[6] == -65504.0 and lo[5] == 0.0
    assert lo[2] == 0.5                                         # 1 + 2^-12 rounds to even (1.0); the rest is the lo half
    # normal range: hi + lo 2^-11 carries 22 bits; below fp16's smallest normal both halves sit on the 2^-24 / 2^-35 grids
    assert float((hi + lo / 2048.0 - t).abs()[:4].max()) <= 2.0 ** -22 * 1.0
    assert hi[4] == round(float(v[4]) * 2.0 ** 24) * 2.0 ** -24 and abs(float(hi[4] + lo[4] / 2048.0 - t[4])) <= 2.0 ** -36
    rows = torch.tensor([[0.0, 0.0], [float("inf"), 1.0], [float("nan"), 1.0], [1.0, 0.5], [0.3, -1.99], [2.0 ** -17, 0.0],
                         [1.0e6, 2.0 ** -17], [2.0 ** -120, 0.0], [3.0e38, 1.0]])
    assert sh.pre_exponent(rows).tolist() == [0, 0, 0, 14, 14, 31, -5, 100, -113]


@pytest.mark.parametrize("name,k,within", [
    ("dgrad", 0, True), ("dgrad", 10, True), ("dgrad", 14, True),
    ("dgrad", 17, False), ("dgrad", 20, False), ("dgrad", 24, False), ("dgrad", 30, False), ("dgrad", 36, False),
    ("wgrad", 0, True), ("wgrad", 10, True), ("wgrad", 14, True), ("wgrad", 17, True),
    ("wgrad", 24, False), ("wgrad", 30, False)])
def test_bare_split_loses_the_small_cotangent(name, k, within):
    worst = _max_ulp(name, k, prescale=False)
    print("\n%s 2^-%d bare split: max %.3g ulp of the scale" % (name, k, worst))
    assert (worst <= BOUND) == within, worst


@pytest.mark.parametrize("name", ["dgrad", "wgrad"])
def test_prescaled_split_is_scale_free(name):
    a, b, ref, ulp = _case(name)
    unit = sh.product(a, b, prescale=True)
    assert float(((unit - ref).abs() / ulp).max()) <= BOUND
    for k in (10, 14, 17, 20, 24, 30, 36, 48, 60):
        got = sh.product(a * 2.0 ** -k, b, prescale=True)
        assert torch.equal(got, unit * 2.0 ** -k), k
    # one entry of 1e6 among entries at 2^-17: its row has an exponent of its own, the other rows keep theirs
    big = a * 2.0 ** -17
    big[3, 5] = 1.0e6
    err = (sh.product(big, b, prescale=True) - big.double() @ b.double()).abs() / sh.ulp_of_scale(big, b)
    assert float(err.max()) <= BOUND, float(err.max())
