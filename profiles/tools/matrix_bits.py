"""Result bits of the matrix units (csrc/conv1x1.hip, conv3x3_1x1.hip and the fused RQS layer kernels fused_layer_v6.hip,
fused_layer_v6_pair.hip, fused_layer_v6s.hip, fused_layer.hip) and of the composed RQS coupling around them, for comparing two builds or two
checkouts (VCNF_ROOT), modelled on stream_bits.py.

    python profiles/tools/matrix_bits.py --out DIR          # on a GPU: every output's raw bytes, one file each
    python profiles/tools/matrix_bits.py --compare DIR DIR  # anywhere: the two runs byte for byte

Inputs and weights come from fixed seeds on the host, so two builds (VCNF_LIB selects the library) given the same file
write comparable directories.  The shapes are the smallest that reach every launch decision; each is named where it is
used.  Needs vcnf_amd, torch and numpy only; the package is taken from the checkout this file lies in (or VCNF_ROOT).
"""
import argparse
import os
import sys

import torch

ROOT = os.environ.get("VCNF_ROOT") or os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from stream_bits import compare, offset_view   # noqa: E402  (the same comparison, the same misaligned view)

GEN = torch.Generator().manual_seed(20240712)
OUT = None
COUNT = 0


def rnd(*shape, scale=1.0):
    return (scale * torch.randn(*shape, generator=GEN, dtype=torch.float64)).float().cuda()


def save(tag, *tensors):
    global COUNT
    for i, t in enumerate(tensors):
        with open(os.path.join(OUT, "%s.%d.bin" % (tag, i)), "wb") as f:
            f.write(t.detach().cpu().contiguous().numpy().tobytes())
        COUNT += 1


# ---------------------------------------------------------------- conv1x1
def conv1x1(L):
    from vcnf_amd.nets.cnn import pack_conv1x1
    # (c_in, c_out, h, w, b, misaligned): one k-step and a partial row block on single pixels (inner % 4 != 0: rows staged
    # through registers); 6 k-steps, 130 images (more than one pass per workgroup, passes crossing images, rows staged
    # by buffer_load ... lds); 16 k-steps; inner % 4 == 0 on a view one float past a 16-byte boundary (registers again)
    cases = [(16, 7, 1, 1, 3, False), (96, 256, 2, 2, 130, False), (256, 256, 4, 4, 3, False), (16, 7, 2, 2, 3, True)]
    for c_in, c_out, h, w, b, off in cases:
        wgt, b_in, b_out = rnd(c_out, c_in, scale=c_in ** -0.5), rnd(c_in), rnd(c_out)
        pack = pack_conv1x1(wgt)
        x = rnd(b, c_in, h, w)
        if off:
            x = offset_view(x)
        tag = "conv1x1_%d_%d_%dx%d_b%d%s" % (c_in, c_out, h, w, b, "_off" if off else "")
        save(tag + "_full", L.conv1x1_fused(x, pack, c_out, in_bias=b_in, out_bias=b_out, in_slope=0.1, out_slope=0.2))
        save(tag + "_bare", L.conv1x1_fused(x, pack, c_out))


def _conv_weights(c_in, c_out):
    import torch.nn.functional as F
    from vcnf_amd.nets.cnn import pack_conv1x1
    w1 = rnd(256, c_in, 3, 3, scale=1.0 / (3.0 * c_in ** 0.5))
    w2 = rnd(256, 256, scale=1.0 / 16)
    k1 = 9 * c_in
    p1 = pack_conv1x1(F.pad(w1.reshape(256, k1), (0, (-k1) % 16)))
    p3 = None
    if c_out:
        w3 = rnd(c_out, 256, 3, 3, scale=1.0 / 48)
        p3 = pack_conv1x1(w3.permute(2, 3, 0, 1).reshape(9 * c_out, 256), row_blocks=(9 * c_out + 31) // 32)
    return p1, pack_conv1x1(w2), p3, rnd(256), rnd(256)


# ---------------------------------------------------------------- conv3x3_1x1 / convnet3
def conv3x3(L):
    # k-steps 1, 2 and 14 of the first layer; one image smaller than a pass, passes crossing images, > 1 pass per workgroup
    for c_in, h, w, b in ((1, 2, 2, 1), (3, 5, 7, 5), (24, 4, 4, 67)):
        p1, p2, _, b1, b2 = _conv_weights(c_in, 0)
        x = rnd(b, c_in, h, w)
        tag = "conv3x3_1x1_%d_%dx%d_b%d" % (c_in, h, w, b)
        save(tag + "_bias", L.conv3x3_1x1_fused(x, p1, p2, b1, b2, 0.1, 0.2))
        save(tag + "_nobias", L.conv3x3_1x1_fused(x, p1, p2, None, None, 0.0, 0.0))
    # c_out = 56: 16 row blocks of W3', every wave runs the row-block loop twice; c_out = 5: a partly filled second block
    for c_in, c_out, h, w in ((2, 56, 3, 3), (3, 5, 5, 7)):
        p1, p2, p3, b1, b2 = _conv_weights(c_in, c_out)
        b3 = rnd(c_out)
        for b in (5, 67):
            x = rnd(b, c_in, h, w)
            save("convnet3_%d_%d_%dx%d_b%d" % (c_in, c_out, h, w, b), L.convnet3_fused(x, p1, p2, p3, b1, b2, b3, c_out, 0.1, 0.2))


# ---------------------------------------------------------------- fused RQS layer
def _coupling(d, ctx, blocks, seed):
    import vcnf_amd as nf
    torch.manual_seed(seed)
    flow = nf.flows.CoupledRationalQuadraticSpline(d, blocks, 128, num_context_channels=ctx or None)
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for p in flow.parameters():                # the reference zero-initialises the last layer: move every parameter
            p.add_(0.05 * torch.randn(p.shape, generator=g))
    return flow.cuda().prqct


def fused_rqs(L):
    from vcnf_amd import fused
    prev = L.small_batch_rows()
    try:
        for d in (32, 64):
            for ctx in (0, 16):
                for blocks in (1, 2, 3):
                    cp = _coupling(d, ctx, blocks, 1000 * d + 10 * ctx + blocks)
                    for sampling in (False, True):
                        tag = "rqs_d%d_c%d_n%d_%s" % (d, ctx, blocks, "inv" if sampling else "fwd")
                        x33, x129 = rnd(33, d), rnd(129, d)
                        c33, c129 = (rnd(33, ctx), rnd(129, ctx)) if ctx else (None, None)
                        cp.fused_precision = 'fp16x3'
                        L.small_batch_rows(prev)             # 32-sample tiles (fused_layer_v6s.hip), one full tile + 1 row
                        save(tag + "_v6s_b33", *fused.run(cp, x33, c33, sampling))
                        L.small_batch_rows(0)                # 128-sample tiles (fused_layer_v6.hip), one full tile + 1 row
                        save(tag + "_v6_b129", *fused.run(cp, x129, c129, sampling))
                        L.small_batch_rows(prev)
                        cp.fused_precision = 'fp32'          # exact fp32 kernel (fused_layer.hip)
                        save(tag + "_f32_b129", *fused.run(cp, x129, c129, sampling))
        # a run of two layers in one launch, both matrix paths
        run = [_coupling(32, 16, 2, 77), _coupling(32, 16, 2, 78)]
        x, c = rnd(33, 32), rnd(33, 16)
        for prec in ('fp16x3', 'fp32'):
            for cp in run:
                cp.fused_precision = prec
            sig = fused._stack_sig(run[0], c)
            assert sig is not None and sig == fused._stack_sig(run[1], c)
            for sampling in (False, True):
                save("rqs_stack2_%s_%s" % (prec, "inv" if sampling else "fwd"), *fused.run_stack(run, sig, x, c, sampling, None, 1.0))
        # two layers above the small-batch threshold on the split-half path, one full 128-sample tile + 1 row: both layers
        # per tile visit (fused_layer_v6_pair.hip) where the shape has the pair form, else one launch per layer - what
        # fused.plan_stack decides
        L.small_batch_rows(0)
        for d, ctx, blocks, pair in ((32, 0, 1, True), (64, 0, 3, True), (64, 16, 2, True), (64, 16, 3, False)):
            run = [_coupling(d, ctx, blocks, 5000 + 1000 * d + 10 * ctx + blocks + s) for s in (0, 100)]
            for cp in run:
                cp.fused_precision = 'fp16x3'
            x, c = rnd(129, d), (rnd(129, ctx) if ctx else None)
            sig = fused._stack_sig(run[0], c)
            assert sig is not None and sig == fused._stack_sig(run[1], c) and fused._pair_form(sig) == pair
            for sampling in (False, True):
                if pair:
                    out = fused.run_stack(run, sig, x, c, sampling, None, 1.0)
                else:
                    y, ld = fused.run(run[0], x, c, sampling)
                    out = fused.run(run[1], y, c, sampling, log_q=ld)
                save("rqs_pair_d%d_c%d_n%d_%s" % (d, ctx, blocks, "inv" if sampling else "fwd"), *out)
    finally:
        L.small_batch_rows(prev)


# ---------------------------------------------------------------- composed RQS coupling (no fused kernel)
def _composed_coupling(path, seed):
    import vcnf_amd as nf
    from vcnf_amd.flows.neural_spline.coupling import PiecewiseRationalQuadraticCoupling
    torch.manual_seed(seed)
    mask = nf.utils.masks.create_alternating_binary_mask(4, even=True)
    if path == "image":
        net = lambda i, o: nf.nets.ConvResidualNet(in_channels=i, out_channels=o, hidden_channels=16, context_channels=None,
                                                   num_blocks=1, activation=torch.nn.functional.relu,
                                                   dropout_probability=0.0, use_batch_norm=False)
    else:
        net = lambda i, o: nf.nets.ResidualNet(in_features=i, out_features=o, context_features=None, hidden_features=16,
                                               num_blocks=1, activation=torch.nn.functional.relu, dropout_probability=0.0,
                                               use_batch_norm=False)
    cp = PiecewiseRationalQuadraticCoupling(
        mask=mask, transform_net_create_fn=net, num_bins=8, tail_bound=3.0, apply_unconditional_transform=True,
        tails=["linear", "circular", "circular", "linear"] if path == "per_feature" else "linear",
        img_shape=[2, 2] if path == "image" else None)
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for p in cp.parameters():                  # the reference zero-initialises the last layer: move every parameter
            p.add_(0.05 * torch.randn(p.shape, generator=g))
    return cp.cuda()


def composed_coupling(L):
    """The three compositions of PiecewiseRationalQuadraticCoupling._run around the conditioner call, B = 33: the
    training path (2-D inputs, autograd recording: SplitColumnsFn, rqs_packed, MergeColumnsFn), 4-D inputs, per-feature
    tails; both directions, without autograd and with it (then the parameter gradients too)."""
    for path, shape in (("train", (33, 4)), ("image", (33, 4, 2, 2)), ("per_feature", (33, 4))):
        cp = _composed_coupling(path, 4100 + len(path))
        x, w = rnd(*shape, scale=1.3), rnd(*shape)
        if path == "per_feature":                  # circular tails: inside the interval
            x = x.clamp(-2.9, 2.9)
        for dirn, fn in (("fwd", cp.forward), ("inv", cp.inverse)):
            if path != "train":                    # (without autograd the 2-D fp32 layer takes a fused or the three-step path)
                save("coupling_%s_%s" % (path, dirn), *fn(x))
            with torch.enable_grad():
                cp.zero_grad(set_to_none=True)
                xin = x.clone().requires_grad_(True)
                out, lad = fn(xin)
                ((out * w).sum() + lad.sum()).backward()
                if path == "train":
                    names = set()
                    todo = [out.grad_fn]
                    while todo:
                        node = todo.pop()
                        if node is not None and node not in names:
                            names.add(node)
                            todo += [n for n, _ in node.next_functions]
                    names = {type(n).__name__ for n in names}
                    assert {"SplitColumnsFnBackward", "RqsPackedFnBackward", "MergeColumnsFnBackward"} <= names, names
            save("coupling_%s_%s_grad" % (path, dirn), out, lad, xin.grad, *[p.grad for p in cp.parameters()])


def main():
    global OUT
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", metavar="DIR", help="run on the GPU and write every output's bytes into DIR")
    ap.add_argument("--compare", nargs=2, metavar="DIR", help="compare two such directories byte for byte")
    args = ap.parse_args()
    if args.compare:
        return compare(*args.compare)
    if not args.out:
        ap.error("--out DIR or --compare DIR DIR")
    import vcnf_amd as nf
    from vcnf_amd import _lib
    OUT = args.out
    os.makedirs(OUT, exist_ok=True)
    with torch.no_grad():
        for part in (conv1x1, conv3x3, fused_rqs, composed_coupling):
            part(_lib)
    torch.cuda.synchronize()
    assert nf.check_saturation() == 0
    print("%s: %d outputs from %s" % (OUT, COUNT, _lib._build.LIB if not os.environ.get("VCNF_LIB") else os.environ["VCNF_LIB"]))
    return 0


if __name__ == "__main__":
    sys.exit(main())
