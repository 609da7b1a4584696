"""Result bits of the fp64 spline unit (csrc/rqs_f64.hip, and csrc/made_sample.hip in both precisions) through their
vcnf_amd._lib wrappers, for comparing two builds (profiles/rqs64_unit.md section 3).

    python profiles/tools/spline64_bits.py --out DIR          # on a GPU: every output's raw bytes, one file each
    python profiles/tools/spline64_bits.py --compare DIR DIR  # anywhere: the two runs byte for byte

VCNF_LIB selects the build of the library under the same Python code.  Inputs come from fixed seeds on the host.  The
shapes are the smallest that reach every kernel instance: K = 8, 10, 16 (the templated instances) and K = 5 (the generic
one); tails none, linear and circular; both directions; n = 300 elements (more than one block of 256), as dense rows
and as an image [20, 5, 3] (inner = 3); one broadcast and one per-element limit on each axis; batch 70 for made_sample
on the two smallest MADE shapes of tests/made_sample_ref.py, (1, 8, 1) and (2, 8, 2): the packed operands are drawn here
in the kernel's own layout (vcnf_made_sample_pack_elems elements, order | count tables), not packed from a layer, so
that the tool needs neither tests/ nor the oracle; the bits do not depend on the weights being a masked network's.  The
inputs hold points outside the tail bound, both interval ends and, in rows of equal logits, interior knots as the host
computes them (with tails the middle one is 0, the interval's midpoint).  Needs vcnf_amd, torch and numpy only.
"""
import argparse
import os
import sys

import torch

ROOT = os.environ.get("VCNF_ROOT") or os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from stream_bits import compare          # the byte-for-byte comparison of two directories

F32, F64 = torch.float32, torch.float64
GEN = torch.Generator().manual_seed(20241021)
OUT = None
COUNT = 0
N, IMAGE = 300, (20, 5, 3)
BINS = (8, 10, 16, 5)
TAILS = (None, "linear", "circular")
BOUND = 3.0


def rnd(*shape, scale=1.0, dtype=F64):
    return (scale * torch.randn(*shape, generator=GEN, dtype=F64)).to(dtype)


def save(tag, *tensors):
    global COUNT
    for i, t in enumerate(tensors):
        path = os.path.join(OUT, "%s.%d" % (tag, i))
        if t is None:
            open(path + ".none", "wb").close()
        else:
            with open(path + ".bin", "wb") as f:
                f.write(t.detach().cpu().contiguous().numpy().tobytes())
        COUNT += 1


def knots(k, lo, hi, floor=1e-3):
    """The knots of a row of equal logits, in the kernel's order of operations."""
    run, out = 0.0, [lo]
    for _ in range(k):
        run += floor + (1.0 - floor * k) * (1.0 / k)
        out.append((hi - lo) * run + lo)
    out[-1] = hi
    return out


def points(k, tails, n):
    """n inputs and the rows (a list) whose logits are to be equal: random points - for a spline with tails a good share
    outside them - then both interval ends, every knot of an equal-logit row, and 0 (the midpoint with tails)."""
    lo, hi = (0.0, 1.0) if tails is None else (-BOUND, BOUND)
    u = torch.rand(n, generator=GEN, dtype=F64)
    x = lo + (hi - lo) * u if tails is None else 1.3 * (lo + (hi - lo) * u)
    special = knots(k, lo, hi) + [0.5 * (lo + hi)]
    rows = list(range(n - len(special), n))
    x[rows[0]:] = torch.tensor(special, dtype=F64)
    if tails is not None:
        x[0], x[1] = 1.5 * lo, 1.5 * hi
    return x, rows


def logits(k, nd, n, flat_rows):
    uw, uh, ud = rnd(n, k), rnd(n, k), rnd(n, nd)
    uw[flat_rows], uh[flat_rows] = 0.0, 0.0
    return uw, uh, ud


def elementwise(L):
    for k in BINS:
        for tails in TAILS:
            cfg = L.make_cfg(k, tails, tail_bound=BOUND)
            nd = L.n_derivatives(cfg)
            x, rows = points(k, tails, N)
            uw, uh, ud = logits(k, nd, N, rows)
            gy, glad = rnd(N), rnd(N)
            # the image layout of the same numbers: params [B, C * P, inner], logit p of element (b, c, s) at [b, c * P + p, s]
            b, c, inner = IMAGE
            params = torch.cat([uw, uh, ud], 1).reshape(b, c, inner, 2 * k + nd).permute(0, 1, 3, 2).reshape(b, -1, inner)
            ximg, gimg, glad_b = x.reshape(IMAGE), gy.reshape(IMAGE), rnd(b)
            dev = [t.cuda() for t in (x, uw, uh, ud, gy, glad, ximg, params.contiguous(), gimg, glad_b)]
            x, uw, uh, ud, gy, glad, ximg, params, gimg, glad_b = dev
            for inverse in (False, True):
                tag = "k%d_%s_%s" % (k, tails or "none", "inv" if inverse else "fwd")
                save("dense_" + tag, *L.rqs_elementwise(x, uw, uh, ud, cfg, inverse))
                save("dense_bwd_" + tag, *L.rqs_elementwise_bwd(x, uw, uh, ud, gy, glad, cfg, inverse))
                save("image_" + tag, *L.rqs_elementwise_image(ximg, params, cfg, inverse))
                save("packed_bwd_" + tag, *L.rqs_packed_bwd(ximg, params, gimg, glad_b, cfg, inverse))


def limits(L):
    # left and bottom per element, right and top one value for all; the inputs lie inside each element's interval and
    # on its ends
    for k in BINS:
        cfg = L.make_cfg(k, None)
        u = torch.rand(N, generator=GEN, dtype=F64)
        left, bottom = -1.0 - torch.rand(N, generator=GEN, dtype=F64), -2.0 - torch.rand(N, generator=GEN, dtype=F64)
        right, top = torch.tensor(1.25, dtype=F64), torch.tensor([2.5], dtype=F64)
        uw, uh, ud = logits(k, k + 1, N, [N - 2, N - 1])
        gy, glad = rnd(N), rnd(N)
        for inverse in (False, True):
            lo, hi = (bottom, top) if inverse else (left, right)
            x = lo + (hi - lo) * u
            x[0], x[1], x[N - 1] = lo[0], hi.reshape(-1)[0], 0.5 * (lo[N - 1] + hi.reshape(-1)[0])
            x[N - 2] = knots(k, float(lo[N - 2]), float(hi.reshape(-1)[0]))[2]        # an interior knot at every K
            lim = [t.cuda() for t in (left, right, bottom, top)]
            ops = [t.cuda() for t in (x, uw, uh, ud)]
            tag = "k%d_%s" % (k, "inv" if inverse else "fwd")
            save("limits_" + tag, *L.rqs_elementwise_limits(*ops, lim, cfg, inverse))
            out = L.rqs_elementwise_limits_bwd(*ops, lim, gy.cuda(), glad.cuda(), cfg, inverse)
            save("limits_bwd_" + tag, *out[:4], *out[4])
            out = L.rqs_elementwise_limits_bwd(*ops, lim, gy.cuda(), glad.cuda(), cfg, inverse, want=(True, False, False, True))
            save("limits_bwd_two_" + tag, *out[:4], *out[4])


def made(L):
    # packed operands of the kernel's own layout (include/vcnf_hip.h) with random weights: (features, hidden, blocks)
    # of the structures d1 and d2, hidden units split evenly over the degrees
    batch = 70
    for d, h, nb in ((1, 8, 1), (2, 8, 2)):
        tables = torch.tensor(list(range(d)) + [h * (i + 1) // d for i in range(d)], dtype=torch.int32).cuda()
        for k in BINS[:3]:
            for tails in TAILS:
                cfg = L.make_cfg(k, tails, tail_bound=1.5)
                p = 2 * k + L.n_derivatives(cfg)
                elems = h * d + h + nb * (2 * h * h + 2 * h) + d * p * h + d * p
                wpack = rnd(elems, scale=0.5)
                x = 1.5 * torch.randn(batch, d, generator=GEN, dtype=F64)
                if tails is None:
                    x = torch.sigmoid(x)
                else:
                    x[0, 0], x[1, 0], x[2, 0] = -1.5, 1.5, 0.0
                for dt in (F32, F64):
                    tag = "made_d%d_k%d_%s_%s" % (d, k, tails or "none", "f64" if dt == F64 else "f32")
                    save(tag, *L.made_sample(x.to(dt).cuda(), wpack.to(dt).cuda(), tables, None, None, h, nb, p, cfg))
                    save(tag + "_acc", *L.made_sample(x.to(dt).cuda(), wpack.to(dt).cuda(), tables, None, None, h, nb, p, cfg,
                                                      logdet=rnd(batch, dtype=dt).cuda(), sign=-1.0))


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
    from vcnf_amd import _lib
    OUT = args.out
    os.makedirs(OUT, exist_ok=True)
    with torch.no_grad():
        for part in (elementwise, limits, made):
            part(_lib)
    torch.cuda.synchronize()
    print("%s: %d outputs from %s, bad discriminants %s" % (OUT, COUNT, _lib.lib_path(),
                                                           int(_lib.bad_discriminant_counter("cuda").item())))
    return 0


if __name__ == "__main__":
    sys.exit(main())
