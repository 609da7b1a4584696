"""The inputs, reference and yardstick of the spline edge tests (tests/spline_edge_ref.py) checked on the CPU with the
oracle alone: every interior knot has test points on both sides of it in the kernel's dtype, all points lie in the
interval, the end-point list has members on both sides of +-tb, the oracle's second rounding order (the stand-in for an
independent correct implementation) meets the tolerance the kernels are held to, the fp32 oracle is non-finite
(rounding-level negative discriminant) on at most 1 % of a case, and on tier A the row yardsticks are small enough for
the test to bite: in fp32 y <= 1e-5 and log|det| <= 5e-4 on every row of the fixed-interval cases up to K = 16.

Three kinds of fp32 tier A case cannot meet those two figures on every row, whatever the seed, and are held to what
the oracle gives on them plus a quarter (TIER_A_OWN; worst row of the forward / inverse case):
  tensor limits K = 5   y 1.44e-5 / 6.3e-6, log|det| 7.2e-4 / 1.62e-3     tensor limits K = 8   y 7.6e-6 / 2.06e-5,
  log|det| 1.46e-3 / 2.71e-3     K = 32 on [-3, 3] (identity-half kernel only)   y 4.9e-6, log|det| 2.8e-4 / 7.0e-4.
With tensor limits an interval is as narrow as 0.5 at |x| up to 3 (the issue's widths), so a bin is up to 12 x
narrower in floats of x than on [-3, 3]; K = 32 halves the bins of K = 16.  What these checks still see: the MEDIAN row
of every such case stays inside the general figures (asserted: y <= 1e-5, log|det| <= 5e-4; measured at most 2.1e-6
and 2.1e-4), so on half the rows a kernel error of 2e-3 in log|det| fails; on the worst row (yardstick 2.7e-3) the
tolerance is 2.2e-2, and only an error of that size - a wrong bin or a stale derivative, which move log|det| by
O(0.1 .. 1) - is seen there.
In fp64 8 x the yardstick stays below the 1e-10 the existing fp64 value tests allow (tests/test_gpu_spline_limits.py,
tests/test_gpu_f64.py)."""
import math

import pytest
import torch

import spline_edge_ref as E

F32, F64 = torch.float32, torch.float64
SQRT_HIDDEN = math.sqrt(128.0)

# (k, tails, limits, store): what tests/test_gpu_spline_edges.py draws, per dtype
SHAPES = {
    F32: [(k, t, "scalar", 1.0) for k in (4, 5, 8, 10, 16) for t in ("linear", "circular", None)]
    + [(32, "linear", "scalar", 1.0)] + [(k, None, "tensor", 1.0) for k in (5, 8)]
    + [(k, "linear", "scalar", SQRT_HIDDEN) for k in (5, 8, 10, 16)],
    F64: [(k, t, "scalar", 1.0) for k in (4, 5, 8, 10, 16) for t in ("linear", "circular", None)]
    + [(k, None, "tensor", 1.0) for k in (5, 8)],
}
# worst-row bounds (y, log|det|) of the fp32 tier A cases the general figures do not fit: measured x 1.25, see above
TIER_A_OWN = {("tensor", 5): (1.8e-5, 2.1e-3), ("tensor", 8): (2.6e-5, 3.4e-3), ("scalar", 32): (1e-5, 8.8e-4)}
CASES = [(dt, tier, k, t, lim, st, inv) for dt in (F32, F64) for (k, t, lim, st) in SHAPES[dt] for tier in "AB"
         for inv in (False, True)]
IDS = ["%s-%s-K%d-%s-%s-%s%s" % ("f32" if c[0] == F32 else "f64", c[1], c[2], c[3], c[4], "inv" if c[6] else "fwd",
                                   "-layer" if c[5] != 1.0 else "") for c in CASES]


@pytest.mark.parametrize("dtype,tier,k,tails,limits,store,inverse", CASES, ids=IDS)
def test_knot_case(dtype, tier, k, tails, limits, store, inverse):
    c = E.case(tier, k, tails, dtype, inverse, "knots", store, limits)
    n = 5 * (k + 1) + k
    assert c.x.shape == (E.R, n) and c.x.dtype == dtype and c.uw.dtype == dtype
    lims = c.limits if c.limits is not None else (-E.TB, E.TB, -E.TB, E.TB)
    lo, hi = (lims[2], lims[3]) if inverse else (lims[0], lims[1])
    lo_t, hi_t = torch.as_tensor(lo, dtype=dtype), torch.as_tensor(hi, dtype=dtype)
    assert bool(((c.x >= lo_t) & (c.x <= hi_t)).all()), "a point lies outside the interval"
    for i in range(1, k):                       # interior knots: the knot, two floats above, two below (own limits)
        for j, off in enumerate((0, 1, 2, -1, -2)):
            own = c.knots[:, 5 * i + j, i].to(dtype)
            assert torch.equal(c.x[:, 5 * i + j], E._step(own, off)), "knot %d offset %d" % (i, off)
            side = c.x[:, 5 * i + j] - own
            assert bool((side == 0).all() if off == 0 else (side * off > 0).all()), "knot %d is not bracketed" % i
    for i in range(k):                          # the midpoints lie strictly inside their bins
        j = 5 * (k + 1) + i
        assert bool(((c.x[:, j].double() > c.knots[:, j, i]) & (c.x[:, j].double() < c.knots[:, j, i + 1])).all())
    assert bool(torch.isfinite(c.y64).all() and torch.isfinite(c.lad64).all())
    _yardstick_holds(c)
    if tier == "A":
        print("tier A yardsticks: y %.3g, log|det| %.3g" % (float(c.yard_y.max()), float(c.yard_lad.max())))
        if dtype == F32:
            by, bl = TIER_A_OWN.get((limits, k), (1e-5, 5e-4))
            assert float(c.yard_y.max()) <= by and float(c.yard_lad.max()) <= bl
            assert float(c.yard_y.median()) <= 1e-5 and float(c.yard_lad.median()) <= 5e-4
        else:
            assert float(c.yard_y.max()) <= 1e-10 / E.SLACK and float(c.yard_lad.max()) <= 1e-10 / E.SLACK


def _yardstick_holds(c):
    """The oracle's second rounding order, in the case's dtype, is within the tolerance of the reference wherever it
    is finite (it is no kernel: its own rounding-level negative discriminants are counted, not compared)."""
    ok = (torch.isfinite(c.y_alt) | ~torch.isfinite(c.y64)) & torch.isfinite(c.lad_alt)
    assert float((~ok).double().mean()) <= 0.01
    if c.dtype == F32:
        print("fp32 oracle non-finite on %.3f %% of the case" % (100 * c.bad32))
        assert c.bad32 <= 0.01
    for what, alt, ref, yard in (("y", c.y_alt, c.y64, c.yard_y), ("log|det|", c.lad_alt, c.lad64, c.yard_lad)):
        fin = torch.isfinite(ref)
        err = (alt.double() - ref).abs()
        bad = ok & fin & (err > E.tolerance(ref, yard, c.dtype))
        assert not bool(bad.any()), "%s: the second rounding order misses the tolerance on %d elements" % (what, int(bad.sum()))


@pytest.mark.parametrize("inverse", [False, True], ids=["fwd", "inv"])
@pytest.mark.parametrize("tier", ["A", "B"])
@pytest.mark.parametrize("tails", ["linear", "circular"])
@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
def test_end_case(dtype, tails, tier, inverse):
    layer = dtype == F32 and tails == "linear"
    for k, store in [(k, 1.0) for k in (4, 5, 8, 10, 16)] + ([(32, 1.0)] + [(k, SQRT_HIDDEN) for k in (5, 8, 10, 16)] if layer else []):
        c = E.case(tier, k, tails, dtype, inverse, "ends", store)
        x = c.x[0]
        tb = torch.tensor(E.TB, dtype=dtype)
        assert bool((x == tb).any() and (x == -tb).any())
        for s in (1.0, -1.0):                   # float neighbours on both sides of each end, and farther out
            assert bool((x == E._step(s * tb, 1)).any() and (x == E._step(s * tb, -1)).any())
            assert bool((x * s > tb).sum() >= 4) and bool(((x * s < tb) & (x * s > 0)).any())
        assert int(torch.isnan(x).sum()) == 1 and int(torch.isinf(x).sum()) == 2
        inside = (c.x >= -tb) & (c.x <= tb)
        assert int(inside[0].sum()) == 8
        # outside: identity, zero log-det; NaN stays NaN
        assert torch.equal(c.y64[~inside].nan_to_num(nan=7.0), c.x[~inside].double().nan_to_num(nan=7.0))
        assert bool((c.lad64[~inside] == 0).all())
        assert bool(torch.isfinite(c.y64[inside]).all() and torch.isfinite(c.lad64[inside]).all())
        _yardstick_holds(c)


@pytest.mark.parametrize("inverse", [False, True], ids=["fwd", "inv"])
@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
@pytest.mark.parametrize("k", [4, 5, 8, 10, 16])
def test_gradient_case(k, dtype, inverse):
    """The gradient yardstick (cotangent on y only): the oracle's second rounding order is within the tolerance."""
    for shared in (False, True):
        if shared and (k == 5 or dtype == F64):
            continue
        g = E.grad_case(k, "linear", dtype, inverse, shared)
        assert bool((g.yard > 0).all())
        for a, ref in zip(g.alt, g.g64):
            assert bool(torch.isfinite(ref).all())
            ok = torch.isfinite(a)
            assert float((~ok).double().mean()) <= 0.01
            bad = ok & ((a - ref).abs() > E.tolerance(ref, g.yard, dtype))
            assert not bool(bad.any()), int(bad.sum())
