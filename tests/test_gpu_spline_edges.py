"""Every implementation of the rational-quadratic spline at the inputs where a bin search goes wrong: on the knots and
one and two floats beside them, on the interval ends and beyond them, with stiff logits.

Inputs (tests/spline_edge_ref.py, checked on the CPU by tests/test_spline_edge_ref.py): R = 32 rows of logits per case,
tier A 0.5 N(0, 1), tier B stiff (2 N(0, 1), and rows with +25 on one width and one height logit and -15 on the first
interior derivative logit).  Knot points: per row the K+1 knots of the searched side, computed in fp64 from the stored
logits and rounded to the kernel's dtype, each with its two float neighbours on both sides, and the K bin midpoints,
clamped into the interval (5 (K+1) + K points per row; with tensor limits each element's own interval).  End points
(linear and circular tails): +-tb, their float neighbours, +-tb (1 + 1e-6), +-0, +-1e-40, +-1e30, +-inf, NaN.

Reference: oracle.rqs.rq_spline / rq_spline_tails in fp64 on the exact stored inputs (the 1 / sqrt(hidden) scale
applied where the path applies it).

Tolerance: helpers.parity's constants per row instead of per fixture,
    fp32  |got - ref64| <= 2e-5 (1 + |ref64|) + 8 yard_row      fp64  |got - ref64| <= 3.7e-14 (1 + |ref64|) + 8 yard_row
yard_row = max(noise_row, sens_row): the oracle's own fp32 error on the row (fp64: the difference between two rounding
orders of the oracle) and what one rounding of the inputs (x and every logit by one unit roundoff) does to the row.
The spline is C1, so either neighbouring bin is right at a knot: NO element is left out and there is no exclusion
cap; outputs are finite wherever the reference is, and nf.check_discriminant() passes after each case.

Exact assertions: outside [-tb, tb] (+-1e30 and +-inf included) y is x bit for bit and log|det| is 0.0; a NaN input
gives a NaN y, log|det| 0.0 and changes nothing else in the launch; the image path equals the dense call and the
identity-half kernel the shared-table kernel bit for bit; the fp16x3 layer equals the fp32 layer bit for bit on samples
that hold a value the fp16 operands cannot carry (the redo contract).

Layer paths: the conditioner's final weight is zero and its bias holds the rows (width and height logits x sqrt(hidden),
which the layer divides out again), so every sample gets exactly these logits; a layer with d_t < 32 transformed features
takes d_t rows spread evenly over the 32, so both halves of tier B are present.  Each sample has ONE active transformed
feature carrying a test point; the other transformed features sit at tb + 1 and the identity features at -(tb + 1),
outside the interval, where they contribute exactly 0: the sample's log|det| is the active element's (batch = rows x
points), and the inactive columns must come back bit-identical.

Backward (vcnf_rqs_elementwise_bwd_f32 / _f64, vcnf_rqs_shared_bwd_f32): tier A knot points, a random cotangent on y
and a ZERO cotangent on log|det| - dy/dx and dy/dlogits are continuous across a knot (the gradient of log|det| jumps
there and stays with tests/test_gpu_grad.py and its cap); reference and yardstick as above by autograd over the oracle,
one yardstick per row over its elements and logit entries.

Each judged output prints a line ``EDGE-RATIO path tier output value``: the worst (|got - ref64| - atol) / yard_row
(allowed: 8); profiles/spline_edges.md records them.
"""
import math

import pytest
import torch

import vcnf_amd as nf
from vcnf_amd import _lib
from vcnf_amd.utils import splines

import spline_edge_ref as E

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64
DT = {"f32": F32, "f64": F64}
TB = E.TB
HIDDEN = 128
SQRT_HIDDEN = math.sqrt(float(HIDDEN))
ALWAYS_TILE32 = 1 << 40
TIERS = ("A", "B")
DIRECTIONS = (False, True)


@pytest.fixture(autouse=True)
def _restore_tile_threshold():
    prev = _lib.small_batch_rows() if torch.cuda.is_available() else None
    yield
    if prev is not None:
        _lib.small_batch_rows(prev)


# ---------------------------------------------------------------- judging
def _bits(t):
    t = t.detach().contiguous()
    return t.view(torch.int64 if t.dtype == F64 else torch.int32)


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


# A bound of its own (profiles/spline_edges.md), for ONE case: fp64 elementwise kernel, linear tails, tier B, K = 16,
# forward, knot points.  csrc/rqs_f64.hip forms its knots by the reference's running sum: K additions, each rounded,
# so a knot carries up to K u (hi - lo) of rounding (u = 2^-53), as the oracle's own knot does, and a floor-level bin
# w = 6e-3 wide beside a bin h ~ 6 high turns that into K u (hi - lo) h / w of y and K u (hi - lo) / w of the bin
# coordinate log|det| is evaluated at.  The fp64 yardstick does not see it: its noise term compares two runs of the
# oracle whose running sums round alike (0 on that row) and its sensitivity term moves x by one unit roundoff,
# 2 u |x| / w.  Measured: y 9.95 x the row yardstick (the midpoint of the floor-level bin of a spiked row; 8.7e-12
# absolute against K u (hi - lo) h / w = 1.1e-11), log|det| 10.0 x (the upper knot of that bin and its float
# neighbours).  Allowed: 19, below 2 x the measured ratios.  Every other K, direction and point set of that path keeps 8.
OWN_SLACK = {("elementwise-linear-f64", "B", 16, False, "knots"): 19.0}


def _within(path, c, out, got, ref, yard):
    got = got.detach().cpu()
    assert got.dtype == c.dtype, (path, got.dtype)
    worst = E.assert_within(got, ref, yard, c.dtype, "%s tier %s %s K=%d %s %s" % (
        path, c.tier, c.points, c.k, "inverse" if c.inverse else "forward", out),
        slack=OWN_SLACK.get((path, c.tier, c.k, c.inverse, c.points), E.SLACK), tag="EDGE-RATIO %s %s %s" % (path, c.tier, out))
    return worst


def _judge(path, c, y, lad, rows=None):
    """y, lad [len(rows), N] of the case's rows ``rows`` (an index; default all) against the reference; at end points
    the exact part too."""
    rows = torch.arange(E.R) if rows is None else rows
    y, lad = y.detach().cpu(), lad.detach().cpu()
    _within(path, c, "y", y, c.y64[rows], c.yard_y[rows])
    _within(path, c, "logdet", lad, c.lad64[rows], c.yard_lad[rows])
    if c.points == "ends":
        x = c.x[rows]
        outside = ~((x >= -TB) & (x <= TB))
        nan = torch.isnan(x)
        assert _same_bits(y[outside & ~nan], x[outside & ~nan]), path + ": y is not x bit for bit outside the interval"
        assert bool(torch.isnan(y[nan]).all()), path + ": NaN input, y is not NaN"
        assert bool((lad[outside] == 0.0).all()), path + ": log|det| is not 0.0 outside the interval"
        assert bool(torch.isfinite(y[~outside]).all() and torch.isfinite(lad[~outside]).all())
        if c.tails == "circular":       # one logit at both ends: log|det| = +-log(derivative) at -tb and at +tb
            a, b = lad[:, 0].double(), lad[:, 1].double()
            tol = 2 * E.tolerance(c.lad64[rows, 0], c.yard_lad[rows], c.dtype)
            assert bool(((a - b).abs() <= tol).all()), path + ": circular tails, the end derivatives differ"


def _nan_changes_nothing_else(path, run, c):
    """The launch with the NaN input against the same launch with 1e30 in its place (outside as well: identity, zero
    log-det): every output element but the NaN's own is the same bit for bit."""
    x2 = torch.where(torch.isnan(c.x), torch.full_like(c.x, 1e30), c.x)
    for (a, mask), (b, _) in zip(run(c.x)[2], run(x2)[2]):
        keep = torch.ones_like(a, dtype=torch.bool) if mask is None else ~mask.to(a.device)
        assert _same_bits(a[keep], b[keep]), path + ": a NaN input changed another element of the launch"


def _check(path, run, c, rows=None):
    y, lad, _ = run(c.x)
    _judge(path, c, y, lad, rows)
    if c.points == "ends":
        _nan_changes_nothing_else(path, run, c)
    nf.check_discriminant()


def _cfg(c, wh_scale=1.0):
    if c.tails is None:
        return _lib.make_cfg(c.k, None, wh_scale=wh_scale)
    return _lib.make_cfg(c.k, c.tails, tail_bound=TB, wh_scale=wh_scale)


def _logits(c, n):
    return [E.expand(t, n).contiguous().cuda() for t in (c.uw, c.uh, c.ud)]


# ---------------------------------------------------------------- 1. elementwise (rqs_point, templated and generic), fp32 / fp64
def _elementwise(c):
    def run(x):
        xd = x.cuda()
        args = [xd] + _logits(c, x.shape[1])
        with torch.no_grad():
            if c.tails is None:
                lim = [t.cuda() if torch.is_tensor(t) else t for t in c.limits]
                y, lad = splines.rational_quadratic_spline(*args, inverse=c.inverse, left=lim[0], right=lim[1],
                                                           bottom=lim[2], top=lim[3])
            else:
                y, lad = splines.unconstrained_rational_quadratic_spline(*args, inverse=c.inverse, tails=c.tails,
                                                                         tail_bound=TB)
        return y, lad, [(y, torch.isnan(x)), (lad, None)]
    return run


@pytest.mark.parametrize("inverse", DIRECTIONS, ids=["fwd", "inv"])
@pytest.mark.parametrize("tier", TIERS)
@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("tails", ["linear", "circular", None])
@pytest.mark.parametrize("k", [4, 8, 10, 16, 5])
def test_elementwise_knots(hip, k, tails, dtype, tier, inverse):
    c = E.case(tier, k, tails, DT[dtype], inverse, "knots")
    if tails is None:
        # x == left is knot 0 (column 0) and x == right knot K (column 5 K) of every row; the reference puts them in
        # bin 0 and in the LAST bin (y64 = bottom and top there), and _check holds the kernel to it
        assert torch.equal(c.x[:, 0], torch.zeros(E.R, dtype=c.dtype)) and torch.equal(c.x[:, 5 * k], torch.ones(E.R, dtype=c.dtype))
        assert bool((c.y64[:, 0].abs() <= 1e-12).all()) and bool(((c.y64[:, 5 * k] - 1.0).abs() <= 1e-5).all())
    _check("elementwise-%s-%s" % (tails, dtype), _elementwise(c), c)


@pytest.mark.parametrize("inverse", DIRECTIONS, ids=["fwd", "inv"])
@pytest.mark.parametrize("tier", TIERS)
@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("tails", ["linear", "circular"])
@pytest.mark.parametrize("k", [4, 8, 10, 16, 5])
def test_elementwise_ends(hip, k, tails, dtype, tier, inverse):
    c = E.case(tier, k, tails, DT[dtype], inverse, "ends")
    _check("elementwise-%s-%s" % (tails, dtype), _elementwise(c), c)


# ---------------------------------------------------------------- 2. tensor limits, one interval per element
@pytest.mark.parametrize("inverse", DIRECTIONS, ids=["fwd", "inv"])
@pytest.mark.parametrize("tier", TIERS)
@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("k", [5, 8])
def test_tensor_limits_knots(hip, k, dtype, tier, inverse):
    c = E.case(tier, k, None, DT[dtype], inverse, "knots", 1.0, "tensor")
    _check("tensor-limits-%s" % dtype, _elementwise(c), c)


# ---------------------------------------------------------------- 3. strided / image rows
IMG = (2, 2, 3)                 # C, H, W: H * W = 6


def _image(c):
    """Elements (row, point) laid out over [B, C, H, W] (padded with copies of element 0), logits in the conditioner's
    layout [B, C * P, H, W]; the dense call on the same elements must agree bit for bit."""
    cfg = _cfg(c)
    per = IMG[0] * IMG[1] * IMG[2]

    def run(x):
        n = x.shape[1]
        e = E.R * n
        b = (e + per - 1) // per
        pad = b * per - e
        rows = torch.cat([torch.arange(E.R).repeat_interleave(n), torch.zeros(pad, dtype=torch.long)])
        xe = torch.cat([x.reshape(-1), x.reshape(-1)[:1].expand(pad)])
        logits = torch.cat([c.uw, c.uh, c.ud], 1)[rows]                                  # [b * per, P]
        p = logits.shape[1]
        params = logits.reshape(b, *IMG, p).permute(0, 1, 4, 2, 3).reshape(b, IMG[0] * p, IMG[1], IMG[2]).contiguous()
        x4 = xe.reshape(b, *IMG).contiguous().cuda()
        y4, lad4 = _lib.rqs_elementwise_image(x4, params.cuda(), cfg, c.inverse)
        dense = [t[rows].reshape(b, *IMG, -1).contiguous().cuda() for t in (c.uw, c.uh, c.ud)]
        yd, ladd = _lib.rqs_elementwise(x4, *dense, cfg, c.inverse)
        assert _same_bits(y4, yd) and _same_bits(lad4, ladd), "image path differs from the dense call"
        y, lad = y4.reshape(-1)[:e].reshape(E.R, n), lad4.reshape(-1)[:e].reshape(E.R, n)
        return y, lad, [(y, torch.isnan(x)), (lad, None)]
    return run


@pytest.mark.parametrize("inverse", DIRECTIONS, ids=["fwd", "inv"])
@pytest.mark.parametrize("tier", TIERS)
@pytest.mark.parametrize("points", ["knots", "ends"])
@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_image_rows(hip, dtype, points, tier, inverse):
    c = E.case(tier, 8, "linear", DT[dtype], inverse, points)
    _check("image-%s" % dtype, _image(c), c)


# ---------------------------------------------------------------- 4. shared table, 5. identity half
def _shared(c):
    cfg = _cfg(c)
    logits = [t.cuda() for t in (c.uw, c.uh, c.ud)]

    def run(x):
        yt, ladt = _lib.rqs_elementwise_shared(x.t().contiguous().cuda(), *logits, cfg, c.inverse)      # batch = points
        y, lad = yt.t().contiguous(), ladt.t().contiguous()
        return y, lad, [(y, torch.isnan(x)), (lad, None)]
    return run


@pytest.mark.parametrize("inverse", DIRECTIONS, ids=["fwd", "inv"])
@pytest.mark.parametrize("tier", TIERS)
@pytest.mark.parametrize("tails", ["linear", None])
@pytest.mark.parametrize("k", [4, 8, 10, 16, 5])
def test_shared_table_knots(hip, k, tails, tier, inverse):
    c = E.case(tier, k, tails, F32, inverse, "knots")
    _check("shared-%s" % tails, _shared(c), c)


@pytest.mark.parametrize("inverse", DIRECTIONS, ids=["fwd", "inv"])
@pytest.mark.parametrize("tier", TIERS)
@pytest.mark.parametrize("k", [4, 8, 10, 16, 5])
def test_shared_table_ends(hip, k, tier, inverse):
    c = E.case(tier, k, "linear", F32, inverse, "ends")
    _check("shared-linear", _shared(c), c)


def _one_hot(x, d, tf, idf):
    """[rows * N, d]: sample (r, j) carries x[r, j] in column tf[r]; its other ``tf`` columns hold tb + 1, the ``idf``
    columns -(tb + 1).  Returns the batch and each sample's active column."""
    r, n = x.shape
    big = torch.empty(r * n, d, dtype=x.dtype)
    big[:, idf] = -(TB + 1.0)
    big[:, tf] = TB + 1.0
    col = torch.as_tensor(tf)[torch.arange(r * n) // n]
    big[torch.arange(r * n), col] = x.reshape(-1)
    return big, col


def _active(full, col, r):
    return full[torch.arange(full.shape[0], device=full.device), col.to(full.device)].reshape(r, -1)


def _inactive_unchanged(path, big, out, col):
    """Every column but the sample's active one comes back bit-identical."""
    mask = torch.ones_like(big, dtype=torch.bool)
    mask[torch.arange(big.shape[0]), col] = False
    assert _same_bits(out.cpu()[mask], big[mask]), path + ": an inactive column changed"


D_HALF = 40                     # the identity-half kernel gathers 32 of 40 columns


def _identity_half(c):
    """The 32 rows are the shared logits of 32 gathered columns; one active column per sample makes the partial
    log-det rows the active element's log|det|.  The gathered columns must equal the shared-table kernel bitwise."""
    cfg = _cfg(c)
    logits = tuple(t.cuda() for t in (c.uw, c.uh, c.ud))
    idf = [j for j in range(D_HALF) if j % 5 != 2]
    other = [j for j in range(D_HALF) if j % 5 == 2]
    idx = torch.tensor(idf, dtype=torch.int32).cuda()

    def run(x):
        big, col = _one_hot(x, D_HALF, idf, other)
        xd = big.cuda()
        out = xd.clone()
        rows = _lib.identity_half_rows(E.R, logits)
        partial = torch.zeros(rows, xd.shape[0], device="cuda")
        _lib.rqs_identity_half(xd, out, idx, E.R, logits, cfg, c.inverse, partial=partial)
        gathered = xd[:, idx.long()].contiguous()
        y_ref, _ = _lib.rqs_elementwise_shared(gathered, *logits, cfg, c.inverse)
        assert _same_bits(out[:, idx.long()], y_ref), "identity half differs from the shared-table kernel"
        _inactive_unchanged("identity-half", big, out, col)
        lad_rows = partial.sum(0)
        return _active(out, col, E.R), lad_rows.reshape(E.R, -1), [(out, torch.isnan(big)), (lad_rows, None)]
    return run


@pytest.mark.parametrize("inverse", DIRECTIONS, ids=["fwd", "inv"])
@pytest.mark.parametrize("tier", TIERS)
@pytest.mark.parametrize("k", [4, 8, 10, 16, 32])
def test_identity_half_knots(hip, k, tier, inverse):
    c = E.case(tier, k, "linear", F32, inverse, "knots")
    _check("identity-half", _identity_half(c), c)


@pytest.mark.parametrize("inverse", DIRECTIONS, ids=["fwd", "inv"])
@pytest.mark.parametrize("tier", TIERS)
@pytest.mark.parametrize("k", [4, 8, 10, 16, 32])
def test_identity_half_ends(hip, k, tier, inverse):
    c = E.case(tier, k, "linear", F32, inverse, "ends")
    _check("identity-half", _identity_half(c), c)


# ---------------------------------------------------------------- 6. packed coupling
D_COUPLING = 64


def _coupling(c):
    """vcnf_rqs_coupling_f32 on params [B, d_t (3K-1)] that repeat the 32 rows for every sample, wh_scale = 1/sqrt(128);
    no shared logits: the identity half is a copy."""
    cfg = _cfg(c, wh_scale=1.0 / SQRT_HIDDEN)
    tf = list(range(1, D_COUPLING, 2))
    idf = list(range(0, D_COUPLING, 2))
    tf_idx, id_idx = (torch.tensor(t, dtype=torch.int32).cuda() for t in (tf, idf))
    row = torch.cat([c.uw, c.uh, c.ud], 1).reshape(1, -1)

    def run(x):
        big, col = _one_hot(x, D_COUPLING, tf, idf)
        params = row.expand(big.shape[0], -1).contiguous().cuda()
        out, ld = _lib.rqs_coupling(big.cuda(), params, tf_idx, id_idx, None, cfg, c.inverse)
        _inactive_unchanged("coupling", big, out, col)
        return _active(out, col, E.R), ld.reshape(E.R, -1), [(out, torch.isnan(big)), (ld, None)]
    return run


@pytest.mark.parametrize("inverse", DIRECTIONS, ids=["fwd", "inv"])
@pytest.mark.parametrize("tier", TIERS)
@pytest.mark.parametrize("points", ["knots", "ends"])
@pytest.mark.parametrize("k", [8, 5])
def test_packed_coupling(hip, k, points, tier, inverse):
    c = E.case(tier, k, "linear", F32, inverse, points, SQRT_HIDDEN)
    _check("coupling", _coupling(c), c)


# ---------------------------------------------------------------- 7. fused layer, 8. run of layers, 9. final layer + splines
def _rows_for(d_t):
    """The d_t rows of a case a layer with d_t transformed features uses: spread evenly over the 32, so that tier B's
    2 N(0, 1) half (rows 0..15) and its spiked half (rows 16..31) are both present."""
    return (torch.arange(d_t) * E.R) // d_t


def _layer(d, ctx_dim, blocks, k, c, seed, zero_logits=False):
    """A coupling layer whose conditioner returns the case's rows _rows_for(d_t) for every sample: zero final weight,
    rows in the bias (feature-major [w | h | d] rows, the layout the coupling reads them in)."""
    torch.manual_seed(seed)
    m = nf.flows.CoupledRationalQuadraticSpline(d, blocks, HIDDEN, k, num_context_channels=ctx_dim or None,
                                                tail_bound=TB).cuda().eval()
    d_t = m.prqct.num_transform_features
    r = _rows_for(d_t)
    bias = torch.cat([c.uw[r], c.uh[r], c.ud[r]], 1).reshape(-1)
    fin = m.prqct.transform_net.final_layer
    assert fin.bias.shape == bias.shape
    with torch.no_grad():
        fin.weight.copy_(torch.zeros_like(fin.weight))
        fin.bias.copy_(torch.zeros_like(bias) if zero_logits else bias.cuda())
    return m


def _precision(m, flag):
    m.prqct.fused, m.prqct.fused_precision = True, flag
    return m


def _context(b, ctx_dim, seed):
    if not ctx_dim:
        return None
    return torch.randn(b, ctx_dim, generator=torch.Generator().manual_seed(seed)).cuda()


def _layer_run(c, call, d, tf, idf, ctx_dim, path):
    """``call(batch, context) -> (out [B, d], log|det| [B])`` on the one-hot batch of the case's rows _rows_for(d_t)."""
    def run(x):
        big, col = _one_hot(x[_rows_for(len(tf))], d, tf, idf)
        with torch.no_grad():
            out, ld = call(big.cuda(), _context(big.shape[0], ctx_dim, 5))
        _inactive_unchanged(path, big, out, col)
        return _active(out, col, len(tf)), ld.reshape(len(tf), -1), [(out, torch.isnan(big)), (ld, None)]
    return run


def _direction(m, inverse):
    """The spline itself is the density direction (the wrapper's ``inverse``), its inverse the sampling direction."""
    fn = m.forward if inverse else m.inverse
    return lambda z, ctx: fn(z, **({"context": ctx} if ctx is not None else {}))


# (d, context, residual blocks): the two one-kernel families, each with and without context
LAYERS = [(64, 16, 2), (64, 0, 2), (32, 0, 1), (32, 16, 1)]


@pytest.mark.parametrize("inverse", DIRECTIONS, ids=["fwd", "inv"])
@pytest.mark.parametrize("tier", TIERS)
@pytest.mark.parametrize("points", ["knots", "ends"])
@pytest.mark.parametrize("tile", ["default", "tile128"])
@pytest.mark.parametrize("precision", ["fp32", "fp16x3"])
@pytest.mark.parametrize("d,ctx_dim,blocks", LAYERS)
def test_fused_layer(hip, d, ctx_dim, blocks, precision, tile, points, tier, inverse):
    from vcnf_amd import fused as fz
    c = E.case(tier, 8, "linear", F32, inverse, points, SQRT_HIDDEN)
    m = _precision(_layer(d, ctx_dim, blocks, 8, c, 90 + d), precision)
    assert fz.eligible(m.prqct, _context(1, ctx_dim, 1))
    if tile == "tile128":
        _lib.small_batch_rows(0)
    tf, idf = m.prqct.transform_features.tolist(), m.prqct.identity_features.tolist()
    path = "fused-d%d-ctx%d-%s-%s" % (d, ctx_dim, precision, tile)
    run = _layer_run(c, _direction(m, inverse), d, tf, idf, ctx_dim, path)
    nf.range_redo_count()
    _check(path, run, c, rows=_rows_for(len(tf)))
    if points == "ends" and precision == "fp16x3":
        # samples holding a value the fp16 operands cannot carry: the exact fp32 layer's results, bit for bit
        full = run(c.x)[2]
        out, ld = full[0][0], full[1][0]
        _precision(m, "fp32")
        full = run(c.x)[2]
        out32, ld32 = full[0][0], full[1][0]
        x = c.x[_rows_for(len(tf))].reshape(-1)
        huge = (~torch.isfinite(x) | (x.abs() > 65504.0)).cuda()
        assert int(huge.sum()) == 5 * len(tf)
        assert _same_bits(out[huge], out32[huge]) and _same_bits(ld[huge], ld32[huge]), "flagged samples: not the fp32 layer's"
    nf.range_redo_count()
    nf.check_discriminant()


@pytest.mark.parametrize("inverse", DIRECTIONS, ids=["fwd", "inv"])
@pytest.mark.parametrize("tier", TIERS)
@pytest.mark.parametrize("points", ["knots", "ends"])
def test_run_of_fused_layers(hip, points, tier, inverse):
    """Two layers in one launch (vcnf_rqs_stack_fused_f32): the rows' layer, then an identity-like layer (zero logits,
    zero final weight) on its output, against the composed fp64 oracle."""
    from vcnf_amd import fused as fz
    d, ctx_dim, blocks = LAYERS[0]
    c = E.case(tier, 8, "linear", F32, inverse, points, SQRT_HIDDEN, "scalar", 0, True)
    first = _precision(_layer(d, ctx_dim, blocks, 8, c, 91), "fp16x3")
    second = _precision(_layer(d, ctx_dim, blocks, 8, c, 92, zero_logits=True), "fp16x3")
    # the density pass walks the flows last to first, the sampling pass first to last: the rows' layer comes first
    flows = [first, second] if inverse else [second, first]
    model = nf.NormalizingFlow(nf.distributions.DiagGaussian(d), flows).cuda().eval()
    _lib.small_batch_rows(ALWAYS_TILE32)
    tf, idf = first.prqct.transform_features.tolist(), first.prqct.identity_features.tolist()

    def call(z, ctx):
        order = list(model.flows) if inverse else list(reversed(model.flows))
        assert fz.plan_stack(order, 0, z, ctx) is not None, "the run of layers is not taken in one launch"
        out, lq = model._walk(z, torch.zeros(len(z), device="cuda"), ctx, not inverse)
        return out, (-lq if inverse else lq)
    nf.range_redo_count()
    _check("stack-fp16x3", _layer_run(c, call, d, tf, idf, ctx_dim, "stack"), c, rows=_rows_for(len(tf)))
    nf.range_redo_count()
    nf.check_discriminant()


@pytest.mark.parametrize("inverse", DIRECTIONS, ids=["fwd", "inv"])
@pytest.mark.parametrize("tier", TIERS)
@pytest.mark.parametrize("points", ["knots", "ends"])
@pytest.mark.parametrize("d,k,blocks,ctx_dim", [(40, 10, 2, 0), (10, 16, 2, 5)])
def test_final_layer_with_splines(hip, d, k, blocks, ctx_dim, points, tier, inverse):
    from vcnf_amd import fused as fz, fused_final
    c = E.case(tier, k, "linear", F32, inverse, points, SQRT_HIDDEN)
    m = _precision(_layer(d, ctx_dim, blocks, k, c, 93 + d), "fp16x3")
    probe = torch.zeros(1, d, device="cuda")
    ctx1 = _context(1, ctx_dim, 1)
    assert not fz.eligible(m.prqct, ctx1) and fused_final.eligible(m.prqct, probe, ctx1)
    tf, idf = m.prqct.transform_features.tolist(), m.prqct.identity_features.tolist()
    path = "final-K%d" % k
    _check(path, _layer_run(c, _direction(m, inverse), d, tf, idf, ctx_dim, path), c, rows=_rows_for(len(tf)))


# ---------------------------------------------------------------- backward: cotangent on y only
def _grad_within(path, g, names, got):
    c = g.case
    for nm, a, ref in zip(names, got, g.g64):
        a = a.detach().cpu()
        assert a.dtype == c.dtype and a.shape == ref.shape, (nm, a.dtype, tuple(a.shape), tuple(ref.shape))
        E.assert_within(a, ref, g.yard, c.dtype, "%s %s K=%d %s" % (path, nm, c.k, "inverse" if c.inverse else "forward"),
                        tag="EDGE-RATIO %s A grad" % path)


GRADS = ("g_x", "g_uw", "g_uh", "g_ud")


@pytest.mark.parametrize("inverse", DIRECTIONS, ids=["fwd", "inv"])
@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("k", [4, 8, 10, 16, 5])
def test_elementwise_vjp_at_knots(hip, k, dtype, inverse):
    g = E.grad_case(k, "linear", DT[dtype], inverse)
    c = g.case
    x = c.x.cuda()
    got = _lib.rqs_elementwise_bwd(x, *_logits(c, c.x.shape[1]), g.gy.cuda(), torch.zeros_like(x), _cfg(c), inverse)
    _grad_within("elementwise-bwd-%s" % dtype, g, GRADS, got)


@pytest.mark.parametrize("inverse", DIRECTIONS, ids=["fwd", "inv"])
@pytest.mark.parametrize("k", [4, 8, 10, 16])
def test_shared_vjp_at_knots(hip, k, inverse):
    g = E.grad_case(k, "linear", F32, inverse, True)
    c = g.case
    x = c.x.t().contiguous().cuda()                                                 # batch = points, period = rows
    gx, gw, gh, gd = _lib.rqs_shared_bwd(x, c.uw.cuda(), c.uh.cuda(), c.ud.cuda(), g.gy.t().contiguous().cuda(),
                                         torch.zeros(x.shape[0], device="cuda"), _cfg(c), inverse)
    _grad_within("shared-bwd", g, GRADS, (gx.t().contiguous(), gw, gh, gd))
