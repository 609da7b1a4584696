"""The fp16 split-half product of csrc/split_half.hpp restated in torch on the CPU (plain helper, no fixtures).

``split`` is the split as ``split8`` / ``split_plain`` do it (both give the same bits): clamp at +-65504,
hi = fp16(v), lo = fp16((v - hi) * 2^11), round to nearest even, fp16 subnormals KEPT.  ``product`` is the three-term
product hi*hi + (hi*lo + lo*hi) * 2^-11 with the accumulation done in fp64 (products of fp16 values are exact there;
what the matrix unit's fp32 accumulator adds on top is rounding of the usual kind and is not modelled).  ``pre_exponent``
is the power of two of ``split_half.hpp::pre_scale``, one per row of the first operand (the cotangent: a row of g in
g @ w, a column of dy - a row of dy^T - in dy^T @ x; a row meets only its own row of the result);
``product(..., prescale=True)`` applies it to those rows and removes it from the rows of the result, as the training
kernels do.

The device tests (tests/test_gpu_grad_range.py) use this as the statement of what the kernels compute.
"""
import torch

LO_SCALE = 2048.0


def split(v):
    """(hi, lo) of an fp32 tensor, both as fp64 tensors holding fp16 values."""
    t = v.float().clamp(-65504.0, 65504.0)
    hi = t.half()
    lo = ((t - hi.float()) * LO_SCALE).half()
    return hi.double(), lo.double()


def pre_exponent(a):
    """e of split_half.hpp::pre_scale per row of a [M, K] (int32 [M]): 14 - floor(log2 max|row|), kept in [-113, 100];
    0 for an all-zero row or one with a non-finite entry."""
    m = a.float().abs().amax(dim=1)
    e = (15 - torch.frexp(m)[1]).clamp(-113, 100)              # frexp: m = f * 2^x, f in [0.5, 1): floor(log2 m) = x - 1
    return torch.where((m > 0) & torch.isfinite(m), e, torch.zeros_like(e)).to(torch.int32)


def product(a, b, prescale=False):
    """a [M, K] @ b [K, N] (fp32 operands) in split-half arithmetic, fp64 result.  ``prescale``: row i of a travels as
    a[i] * 2^e[i]."""
    e = pre_exponent(a) if prescale else torch.zeros(a.shape[0], dtype=torch.int32)
    a = torch.ldexp(a.float(), e[:, None])                # exact: a power of two, no fp32 under- or overflow in range
    ah, al = split(a)
    bh, bl = split(b)
    return torch.ldexp(ah @ bh + (ah @ bl + al @ bh) / LO_SCALE, -e[:, None])


def ulp_of_scale(a, b):
    """2^-24 * sum_k |a b|: one fp32 rounding of the dot product's scale, the unit every bound here is stated in."""
    return 2.0 ** -24 * (a.double().abs() @ b.double().abs())
