"""Two RQS coupling layers per tile visit of the 128-sample-tile kernel (csrc/fused_layer_v6_pair.hip).

Above the small-batch threshold the planner (vcnf_amd.fused.plan_stack) hands the split-half path runs of exactly two
layers where ``vcnf_rqs_pair_fused_supported`` says that both layers' tables fit the kernel's LDS; the kernel keeps the
tile in LDS between the two layers and adds the two log-dets onto the running log-density one after the other, as two
launches do.  Reference throughout: one launch per layer (``fuse_rqs_stacks = False``), never the pair path itself -
latents AND log-densities bitwise, both directions.

Range safety: the kernel has one range flag per 128-sample tile (it sets the tile's four 32-row entries of the flag
array, like the one-layer kernel: tests/test_gpu_fused_tail.py), so "its tile" below is the 128-row tile of the entry.
"""
import pytest
import torch

import vcnf_amd as nf
from vcnf_amd import _lib
from vcnf_amd import fused as fz

pytestmark = pytest.mark.gpu

TILE, WGS = 128, 256
ALWAYS_TILE32 = 1 << 40
# one row | one whole tile | one row more | a few tiles, the last ragged | workgroup 0 walks tiles 0 and 256, the last tile
# ragged: the smallest batch at which a persistent workgroup hands over from one tile to the next
BATCHES = (1, TILE, TILE + 1, TILE * 3 + 37, TILE * (WGS + 1) + 5)
# (d, ctx, residual blocks, the shape has the pair form)
SHAPES = [(64, 16, 2, True), (32, 0, 1, True), (64, 0, 3, True), (64, 16, 3, False)]


@pytest.fixture(autouse=True)
def _restore_tile_threshold():
    prev = _lib.small_batch_rows() if torch.cuda.is_available() else None
    yield
    if prev is not None:
        _lib.small_batch_rows(prev)


def _model(layers, d, ctx_dim, blocks, seed, precision="fp16x3"):
    torch.manual_seed(seed)
    flows = [nf.flows.CoupledRationalQuadraticSpline(d, blocks, 128, 8, reverse_mask=bool(i % 2),
                                                     num_context_channels=ctx_dim or None) for i in range(layers)]
    model = nf.NormalizingFlow(nf.distributions.DiagGaussian(d), flows).cuda().eval()
    with torch.no_grad():
        for n, p in model.named_parameters():
            if "unnormalized_" in n:
                p.normal_(0.0, 0.5)
    return _precision(model, precision)


def _precision(model, flag):
    for mod in model.modules():
        if isinstance(mod, nf.flows.PiecewiseRationalQuadraticCoupling):
            mod.fused, mod.fused_precision = True, flag
    return model


def _walk(model, order, z, lq, ctx, density, stacks):
    """The layers of ``order`` applied to z, adding onto the pre-filled lq: planned runs through fused.run_stack
    (``stacks``) or one launch per layer.  Returns z and the lengths of the planned runs."""
    kw = {"context": ctx} if ctx is not None else {}
    runs, i = [], 0
    while i < len(order):
        plan = fz.plan_stack(order, i, z, ctx) if stacks else None
        if plan is not None:
            end, run, sig = plan
            z = fz.run_stack(run, sig, z, ctx, not density, lq, 1.0 if density else -1.0)[0]
            runs.append(end - i)
            i = end
        else:
            z = order[i].inverse_into(z, lq, **kw) if density else order[i].forward_into(z, lq, **kw)
            i += 1
    return z, runs


@pytest.mark.parametrize("layers", [2, 3, 5])
@pytest.mark.parametrize("d,ctx_dim,blocks,pair", SHAPES)
def test_pair_matches_one_launch_per_layer_bitwise(hip, d, ctx_dim, blocks, pair, layers):
    model = _model(layers, d, ctx_dim, blocks, 900 + d + ctx_dim + blocks + layers)
    assert bool(_lib.lib().vcnf_rqs_pair_fused_supported(d // 2, d // 2, ctx_dim, 128, blocks)) == pair
    flows = list(model.flows)
    for B in BATCHES:
        g = torch.Generator(device="cuda").manual_seed(5 + B)
        x = torch.randn(B, d, device="cuda", generator=g) * 1.3
        eps = torch.randn(B, d, device="cuda", generator=g)
        ctx = torch.randn(B, ctx_dim, device="cuda", generator=g) if ctx_dim else None
        lq0 = torch.randn(B, device="cuda", generator=g) * 3.0          # a running log-density of its own in every row
        kw = {"context": ctx} if ctx_dim else {}

        # the planner: runs of two above the threshold where the pair form exists, the long runs below it
        _lib.small_batch_rows(ALWAYS_TILE32)
        with torch.no_grad():
            plan = fz.plan_stack(flows, 0, x, ctx)
        assert plan is not None and plan[0] == layers, "below the threshold: one run for the whole stack"
        _lib.small_batch_rows(0)
        with torch.no_grad():
            plan = fz.plan_stack(flows, 0, x, ctx)
            last = fz.plan_stack(flows, layers - 1, x, ctx)
        assert (plan is not None and plan[0] == 2 and len(plan[1]) == 2) if pair else plan is None
        assert last is None, "a single layer is no run"

        out = {}
        for stacks in (True, False):
            model.fuse_rqs_stacks = stacks
            with torch.no_grad():
                lp = model.log_prob(x, **kw)
                z, lq = model.sample_from(eps, **kw)
                lqd, lqs = lq0.clone(), lq0.clone()
                zd, runs_d = _walk(model, list(reversed(flows)), x, lqd, ctx, True, stacks)
                zs, runs_s = _walk(model, flows, eps, lqs, ctx, False, stacks)
            want = [2] * (layers // 2) if stacks and pair else []
            assert runs_d == want and runs_s == want, (B, runs_d, runs_s)
            out[stacks] = (lp, z, lq, zd, lqd, zs, lqs)
        model.fuse_rqs_stacks = True
        names = ("log_prob", "samples", "samples' log-density", "density latents", "density log_q", "sampling latents",
                 "sampling log_q")
        for name, a, b in zip(names, out[True], out[False]):
            diff = (a != b).nonzero()
            assert torch.equal(a, b), (B, name, "%d entries differ, first %s" % (diff.shape[0], diff[:4].tolist()))
        assert bool((out[True][4] != lq0).any()) and bool(torch.isfinite(out[True][0]).all())
    assert nf.range_redo_count() == 0
    nf.check_discriminant()


FAULTS = ["identity feature of the first layer", "transformed feature of the first layer", "NaN input", "Inf context"]


@pytest.mark.parametrize("sampling", [False, True], ids=["density", "sampling"])
def test_pair_is_range_safe(hip, sampling):
    """One entry the fp16 halves cannot carry, in turn: in an identity feature of the layer applied first; in a
    TRANSFORMED feature of that layer (outside the spline's interval: the linear tail passes it on unchanged, the first
    layer's conditioner never sees it, and it is an identity feature of the second layer - only layer 1 can flag it,
    checked here with the one-layer kernel: the first layer alone flags nothing, the two layers one tile); a NaN input;
    an Inf context entry.  Each flags its 128-row tile and no other: those rows are BITWISE the fp32 model's latents, their
    log-density within the 1e-4 of test_rqs_stack_is_range_safe_on_the_device (the fp32 launch sums the pair's
    log-dets before it adds them), every other row BITWISE the clean run's, the redo counter counts one tile."""
    d, ctx_dim = 64, 16
    model = _model(2, d, ctx_dim, 2, 77)
    _lib.small_batch_rows(0)
    B = TILE * 2 + 37
    g = torch.Generator(device="cuda").manual_seed(78)
    x = torch.randn(B, d, device="cuda", generator=g)
    ctx = torch.randn(B, ctx_dim, device="cuda", generator=g)
    lq0 = torch.randn(B, device="cuda", generator=g) * 3.0
    order = list(model.flows) if sampling else list(reversed(model.flows))
    first = order[0].prqct
    idf, tff = first.identity_features.tolist(), first.transform_features.tolist()
    assert set(tff) == set(order[1].prqct.identity_features.tolist())

    def run(xa, ca, stacks=True, layers=order):
        lq = lq0.clone()
        with torch.no_grad():
            z, runs = _walk(model, layers, xa, lq, ca, not sampling, stacks)
        assert runs == ([2] if stacks and len(layers) == 2 and model.flows[0].prqct.fused_precision == "fp16x3" else [])
        return z, lq

    nf.range_redo_count()
    z_clean, lq_clean = run(x, ctx)
    assert nf.range_redo_count() == 0
    eq = lambda a, b: torch.equal(torch.nan_to_num(a, nan=1.25e30), torch.nan_to_num(b, nan=1.25e30))
    for k, fault in enumerate(FAULTS):
        xb, cb = x.clone(), ctx.clone()
        row = (40, TILE + 100, TILE * 2 + 36, 3)[k]                     # tiles 0, 1, 2 (the ragged one, its last row), 0
        if k == 0:
            xb[row, idf[3]] = 3.0e5
        elif k == 1:
            xb[row, tff[5]] = 3.0e5
            run(xb, cb, stacks=False, layers=order[:1])
            assert nf.range_redo_count() == 0, "the first layer alone must not flag a transformed feature"
            run(xb, cb, stacks=False)
            assert nf.range_redo_count() == 1, "the second layer flags it as its identity feature"
        elif k == 2:
            xb[row, idf[0]] = float("nan")
        else:
            cb[row, 5] = float("inf")
        z, lq = run(xb, cb)
        assert nf.range_redo_count() == 1, fault
        _precision(model, "fp32")
        z32, lq32 = run(xb, cb)
        _precision(model, "fp16x3")
        torch.cuda.synchronize()
        redo = torch.arange(B, device="cuda") // TILE == row // TILE
        assert eq(z[redo], z32[redo]), (fault, "flagged tile: the exact fp32 kernel's latents, bitwise")
        a, b = torch.nan_to_num(lq[redo], nan=0.0, posinf=0.0, neginf=0.0), torch.nan_to_num(lq32[redo], nan=0.0, posinf=0.0, neginf=0.0)
        assert eq(torch.isfinite(lq[redo]), torch.isfinite(lq32[redo])) and bool(((a - b).abs() <= 1e-4).all()), \
            (fault, float((a - b).abs().max()))
        assert torch.equal(z[~redo], z_clean[~redo]) and torch.equal(lq[~redo], lq_clean[~redo]), (fault, "other rows: the clean run")
    nf.range_redo_count()
    _lib.bad_discriminant_counter("cuda").zero_()
