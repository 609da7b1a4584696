"""The tile tail of the 128-sample-tile fused RQS layer kernel (csrc/fused_layer_v6.hip) in accumulate mode.

In accumulate mode (``inverse_into`` / ``forward_into``) the kernel fetches the running log-density of a tile's rows into
LDS early in the tile and adds onto that copy in the tail; log-det, range flags and y leave through bounds-checked
stores.  A row mix-up in that fetch is invisible when the running log-density is one constant, so every test here
gives each row a value of its own.

References, never the kernel's own accumulate path: its store mode plus one fp32 add formed by torch (the same single
add the kernel does: BITWISE), the 32-sample-tile kernel (csrc/fused_layer_v6s.hip: z BITWISE, log-density within
4e-6 * (1 + |ref|), the two kernels add a sample's per-feature terms in a different order - bound of
tests/test_gpu_parity.py::test_small_batch_kernel_matches_large_batch_kernel), and the exact fp32 kernel for flagged
tiles (BITWISE).
"""
import pytest
import torch

import vcnf_amd as nf
from vcnf_amd import _lib

pytestmark = pytest.mark.gpu

TILE, WGS = 128, 256
ALWAYS_TILE32 = 1 << 40
TWO_TILES_RAGGED = TILE * WGS + 77                  # workgroup 0 walks tiles 0 and 256, the latter with 77 rows
# one partial tile | one row short of a tile | ragged second tile | fewer tiles than workgroups | a workgroup with two tiles
BATCHES = (1, 127, 129, TILE * 5 + 1, TWO_TILES_RAGGED)
MODELS = [(64, 16, 2), (32, 0, 1)]                  # (d, ctx, residual blocks)
SENTINEL = -12345.678


@pytest.fixture(autouse=True)
def _restore_tile_threshold():
    prev = _lib.small_batch_rows() if torch.cuda.is_available() else None
    yield
    if prev is not None:
        _lib.small_batch_rows(prev)


def _layer(d, ctx_dim, blocks, seed, reverse_mask=False):
    torch.manual_seed(seed)
    m = nf.flows.CoupledRationalQuadraticSpline(d, blocks, 128, 8, num_context_channels=ctx_dim or None,
                                                reverse_mask=reverse_mask).cuda().eval()
    with torch.no_grad():
        for n, p in m.named_parameters():
            if "unnormalized_" in n:
                p.normal_(0.0, 0.5)
    return m


def _precision(m, flag):
    for mod in m.modules():
        if isinstance(mod, nf.flows.PiecewiseRationalQuadraticCoupling):
            mod.fused, mod.fused_precision = True, flag
    return m


def _inputs(B, d, ctx_dim, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.randn(B, d, device="cuda", generator=g) * 1.5
    kw = {"context": torch.randn(B, ctx_dim, device="cuda", generator=g)} if ctx_dim else {}
    lq0 = torch.randn(B, device="cuda", generator=g) * 3.0      # a different running log-density in every row
    return x, kw, lq0


def _within(got, ref):
    return bool(((got - ref).abs() <= 4e-6 * (1.0 + ref.abs())).all())


@pytest.mark.parametrize("d,ctx_dim,blocks", MODELS)
def test_accumulate_equals_store_plus_one_add_bitwise(hip, d, ctx_dim, blocks):
    from vcnf_amd import fused as fz
    m = _precision(_layer(d, ctx_dim, blocks, 40 + d + blocks), "fp16x3")
    assert fz.eligible(m.prqct, torch.zeros(1, ctx_dim, device="cuda") if ctx_dim else None)
    for B in BATCHES:
        x, kw, lq0 = _inputs(B, d, ctx_dim, 7 + B)
        out = {}
        for rows in (0, ALWAYS_TILE32):
            _lib.small_batch_rows(rows)
            with torch.no_grad():
                zi, ldi = m.inverse(x, **kw)
                zf, ldf = m.forward(x, **kw)
                lqi, lqf = lq0.clone(), lq0.clone()
                zia = m.inverse_into(x, lqi, **kw)
                zfa = m.forward_into(x, lqf, **kw)
            out[rows] = (zi, ldi, zf, ldf, zia, lqi, zfa, lqf)
        zi, ldi, zf, ldf, zia, lqi, zfa, lqf = out[0]
        ref = out[ALWAYS_TILE32]
        bad = (lqi != lq0 + ldi).nonzero().flatten()
        assert torch.equal(lqi, lq0 + ldi), (B, "density: %d rows differ, first %s" % (bad.numel(), bad[:8].tolist()))
        bad = (lqf != lq0 - ldf).nonzero().flatten()
        assert torch.equal(lqf, lq0 - ldf), (B, "sampling: %d rows differ, first %s" % (bad.numel(), bad[:8].tolist()))
        assert torch.equal(zia, zi) and torch.equal(zfa, zf), (B, "z differs between store and accumulate mode")
        assert torch.equal(zia, ref[4]) and torch.equal(zfa, ref[6]), (B, "z differs from the 32-sample-tile kernel")
        for got, want in ((lqi, ref[5]), (lqf, ref[7])):
            print("B=%d: max |log-density difference| to the 32-sample-tile kernel %.3g" % (B, float((got - want).abs().max())))
            assert _within(got, want), B
    nf.check_discriminant()


@pytest.mark.parametrize("B", [129, TWO_TILES_RAGGED])
@pytest.mark.parametrize("d,ctx_dim,blocks", MODELS)
def test_nothing_past_the_batch_is_written(hip, d, ctx_dim, blocks, B):
    m = _precision(_layer(d, ctx_dim, blocks, 50 + d + blocks), "fp16x3")
    _lib.small_batch_rows(0)
    x, kw, lq0 = _inputs(B, d, ctx_dim, 11 + B)
    for into in (m.inverse_into, m.forward_into):
        buf = torch.full((B + 3 * TILE + 5,), SENTINEL, device="cuda")
        lq = buf[:B]
        lq.copy_(lq0)
        with torch.no_grad():
            into(x, lq, **kw)
        torch.cuda.synchronize()
        assert bool((buf[B:] == SENTINEL).all()), "the kernel wrote past the batch"
        assert bool((lq != lq0).any()) and bool(torch.isfinite(lq).all())


@pytest.mark.parametrize("sampling", [False, True], ids=["density", "sampling"])
def test_flagged_tiles_keep_their_rows_log_density(hip, sampling):
    """One value beyond +-65504 in the first tile of workgroup 0 (tile 0) and one in its last, ragged tile (tile 256):
    those tiles come from the exact fp32 kernel, which adds onto the untouched running log-density; every other row is
    the clean run's."""
    m = _precision(_layer(64, 16, 2, 62), "fp16x3")
    _lib.small_batch_rows(0)
    B = TWO_TILES_RAGGED
    x, kw, lq0 = _inputs(B, 64, 16, 23)
    idf = m.prqct.identity_features.tolist()
    xb = x.clone()
    xb[0 * TILE + 3, idf[0]] = 3.0e5
    xb[256 * TILE + 76, idf[1]] = -7.0e4
    run = lambda mod, a, lq: (mod.forward_into if sampling else mod.inverse_into)(a, lq, **kw)
    nf.range_redo_count()
    with torch.no_grad():
        lq_clean = lq0.clone()
        z_clean = run(m, x, lq_clean)
        assert nf.range_redo_count() == 0
        lq = lq0.clone()
        z = run(m, xb, lq)
        assert nf.range_redo_count() == 2
        lq32 = lq0.clone()
        z32 = run(_precision(m, "fp32"), xb, lq32)
        _precision(m, "fp16x3")
    torch.cuda.synchronize()
    redo = torch.isin(torch.arange(B, device="cuda") // TILE, torch.tensor([0, 256], device="cuda"))
    assert torch.equal(z[redo], z32[redo]) and torch.equal(lq[redo], lq32[redo]), "flagged tiles: exact fp32 path, bitwise"
    assert torch.equal(z[~redo], z_clean[~redo]) and torch.equal(lq[~redo], lq_clean[~redo]), "other rows: the clean run"
    nf.range_redo_count()
    _lib.bad_discriminant_counter("cuda").zero_()


def test_repeated_accumulation_over_three_layers(hip):
    """A stale copy of the running log-density carried from tile to tile or from launch to launch shows here: three
    layers add onto the same vector, each workgroup 0 tile after another one."""
    B = TWO_TILES_RAGGED
    flows = [_precision(_layer(64, 16, 2, 70 + i, reverse_mask=bool(i % 2)), "fp16x3") for i in range(3)]
    model = nf.NormalizingFlow(nf.distributions.DiagGaussian(64), flows).cuda().eval()
    x, kw, _ = _inputs(B, 64, 16, 31)
    out = {}
    for rows in (0, ALWAYS_TILE32):
        _lib.small_batch_rows(rows)
        with torch.no_grad():
            out[rows] = model.log_prob(x, kw["context"])
    err = (out[0] - out[ALWAYS_TILE32]).abs()
    print("max |log_prob difference| %.3g" % float(err.max()))
    assert _within(out[0], out[ALWAYS_TILE32]), float(err.max())
    nf.check_discriminant()
