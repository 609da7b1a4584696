"""The 128-sample-tile fused RQS layer kernel (csrc/fused_layer_v6.hip) over every way a workgroup can walk its tiles.

The kernel is persistent: 256 workgroups, workgroup w evaluates tiles w, w + 256, w + 512, ...; what one tile leaves
behind in LDS and in registers (bias tables, prefetched rows, the range flag, the wave groups' one-step offset) is what
the next one starts from.  The reference is never that kernel: the 32-sample-tile kernel (csrc/fused_layer_v6s.hip,
one tile per workgroup pass, same packed weights and the same matrix instructions in the same order) for clean inputs,
the exact fp32 kernel for tiles that hold a value the fp16 halves cannot carry.

Bounds: z BITWISE; log|det| within 4e-6 * (1 + |ref|) - the two kernels add a sample's per-feature terms in a
different order (bound of tests/test_gpu_parity.py::test_small_batch_kernel_matches_large_batch_kernel).
"""
import pytest
import torch

import vcnf_amd as nf
from vcnf_amd import _lib

pytestmark = pytest.mark.gpu

TILE, WGS = 128, 256
ALWAYS_TILE32 = 1 << 40
# one tile per workgroup | several tiles, ragged last one | fewer tiles than workgroups + a partial | one workgroup with two
BATCHES = (TILE * WGS, 3 * TILE * WGS + 77, TILE * 5 + 1, TILE * (WGS + 1))


@pytest.fixture(autouse=True)
def _restore_tile_threshold():
    prev = _lib.small_batch_rows() if torch.cuda.is_available() else None
    yield
    if prev is not None:
        _lib.small_batch_rows(prev)


def _layer(d, ctx_dim, blocks, seed):
    torch.manual_seed(seed)
    m = nf.flows.CoupledRationalQuadraticSpline(d, blocks, 128, 8, num_context_channels=ctx_dim or None).cuda().eval()
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


@pytest.mark.parametrize("blocks", [1, 2, 3])
@pytest.mark.parametrize("d,ctx_dim", [(64, 16), (64, 0), (32, 16), (32, 0)])
def test_tile128_kernel_matches_tile32_kernel_over_tile_walks(hip, d, ctx_dim, blocks):
    """Both directions, store and accumulate modes, every family member, at batch sizes that give a workgroup one tile
    only, several tiles with a ragged last one, no tile at all for most workgroups, and exactly one workgroup a second
    tile."""
    from vcnf_amd import fused as fz
    m = _precision(_layer(d, ctx_dim, blocks, 900 + d + ctx_dim + blocks), "fp16x3")
    assert fz.eligible(m.prqct, torch.zeros(1, ctx_dim, device="cuda") if ctx_dim else None)
    for B in BATCHES:
        x = torch.randn(B, d, device="cuda") * 1.5
        kw = {"context": torch.randn(B, ctx_dim, device="cuda")} if ctx_dim else {}
        out = {}
        for rows in (ALWAYS_TILE32, 0):
            _lib.small_batch_rows(rows)
            with torch.no_grad():
                zf, ldf = m.forward(x, **kw)
                zi, ldi = m.inverse(x, **kw)
                lq = torch.full((B,), -0.5, device="cuda")
                za = m.inverse_into(x, lq, **kw)
                lqf = torch.full((B,), 0.75, device="cuda")
                zfa = m.forward_into(x, lqf, **kw)
            out[rows] = (zf, ldf, zi, ldi, za, lq, zfa, lqf)
        ref, got = out[ALWAYS_TILE32], out[0]
        for i in (0, 2, 4, 6):
            bad = (ref[i] != got[i]).any(dim=1).nonzero().flatten()
            assert torch.equal(ref[i], got[i]), (B, i, "z differs in %d rows, first %s" % (bad.numel(), bad[:8].tolist()))
        for i in (1, 3, 5, 7):
            err = (ref[i] - got[i]).abs()
            print("B=%d output %d: max |log-det difference| %.3g" % (B, i, float(err.max())))
            assert bool((err <= 4e-6 * (1.0 + ref[i].abs())).all()), (B, i, float(err.max()))
    nf.check_discriminant()


@pytest.mark.parametrize("blocks", [1, 2, 3])
@pytest.mark.parametrize("sampling", [False, True], ids=["density", "sampling"])
def test_flagged_tiles_in_first_middle_and_last_place_of_a_workgroup(hip, blocks, sampling):
    """Values beyond +-65504, a non-finite context entry and NaN rows, placed in the first, a middle and the last tile
    of a workgroup's walk (tile t belongs to workgroup t % 256): all of a workgroup's tiles flagged (5, 261, 517), first
    two and the ragged last one of four (0, 256, 768), a middle one only (265), a last one only (522).  A flagged tile is
    not stored by the split-half kernel and comes from the exact fp32 kernel; every other row is BITWISE the clean run's;
    the redo counter counts the flagged tiles; store and accumulate modes."""
    m = _precision(_layer(64, 16, blocks, 60 + blocks), "fp16x3")
    _lib.small_batch_rows(0)
    B = 3 * TILE * WGS + 77                                  # 769 tiles: workgroup 0 walks four, the others three
    x, ctx = torch.randn(B, 64, device="cuda"), torch.randn(B, 16, device="cuda")
    call = (lambda mod, a, c: mod.forward(a, context=c)) if sampling else (lambda mod, a, c: mod.inverse(a, context=c))
    nf.range_redo_count()
    with torch.no_grad():
        z_clean, ld_clean = call(m, x, ctx)
    assert nf.range_redo_count() == 0
    idf = m.prqct.identity_features.tolist()
    xb, cb = x.clone(), ctx.clone()
    nan, inf = float("nan"), float("inf")
    placed = {5: (3, 3.0e5), 261: (77, nan), 517: (127, -7.0e4), 0: (0, 65505.0 * 4), 256: (64, nan), 768: (76, -3.0e5),
              265: (31, nan), 522: (100, 1.0e38)}
    for i, (t, (r, v)) in enumerate(placed.items()):
        xb[t * TILE + r, idf[i % len(idf)]] = v
    cb[517 * TILE + 2, 5] = inf                             # and a non-finite context entry in an already flagged tile
    cb[9 * TILE + 33, 0] = -inf                             # ... and in a tile of its own (first of workgroup 9)
    flagged = sorted(list(placed) + [9])
    with torch.no_grad():
        z, ld = call(m, xb, cb)
        assert nf.range_redo_count() == len(flagged)
        z32, ld32 = call(_precision(m, "fp32"), xb, cb)
        _precision(m, "fp16x3")
        logq = torch.full((B,), 0.25, device="cuda")
        z_acc = m.forward_into(xb, logq, context=cb) if sampling else m.inverse_into(xb, logq, context=cb)
    torch.cuda.synchronize()
    redo = torch.isin(torch.arange(B, device="cuda") // TILE, torch.tensor(flagged, device="cuda"))
    eq = lambda a, b: torch.equal(torch.nan_to_num(a, nan=1.25e30), torch.nan_to_num(b, nan=1.25e30))
    assert eq(z[redo], z32[redo]) and eq(ld[redo], ld32[redo]), "flagged tiles must carry the exact fp32 kernel's results"
    assert torch.equal(z[~redo], z_clean[~redo]) and torch.equal(ld[~redo], ld_clean[~redo])
    assert not torch.isfinite(z[261 * TILE + 77]).all() and not torch.isfinite(z[265 * TILE + 31]).all()
    assert eq(z_acc, z)
    assert eq(logq, 0.25 + (-1.0 if sampling else 1.0) * ld)
    nf.range_redo_count()
    _lib.bad_discriminant_counter("cuda").zero_()           # NaN rows trip the sampling direction's discriminant check
