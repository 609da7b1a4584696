"""Result bits of the stream kernels (csrc/affine_kernels.hip, class_cond_gaussian.hip, gaussian_mixture.hip,
heavy_tail.hip) through their vcnf_amd._lib wrappers, forward and backward, fp32 and fp64, for comparing two builds.

    python profiles/tools/stream_bits.py --out DIR          # on a GPU: every output's raw bytes, one file each
    python profiles/tools/stream_bits.py --compare DIR DIR  # anywhere: the two runs byte for byte

Inputs come from fixed seeds on the host, so two checkouts given the same file write comparable directories.  Bytes,
not values, are compared: some outputs are NaN by design (labels outside the table).  The shapes are the smallest
that reach every launch decision of the host functions; each is named where it is used.  Needs vcnf_amd, torch and
numpy only; the package is taken from the checkout this file lies in (or from VCNF_ROOT).
"""
import argparse
import os
import sys

import torch

ROOT = os.environ.get("VCNF_ROOT") or os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

F32, F64 = torch.float32, torch.float64
GEN = torch.Generator().manual_seed(20240611)
OUT = None
COUNT = 0


def rnd(*shape, dtype=F32, scale=1.0):
    return (scale * torch.randn(*shape, generator=GEN, dtype=torch.float64)).to(dtype).cuda()


def pos(*shape, dtype=F32, lo=0.5, hi=3.0):
    return (lo + (hi - lo) * torch.rand(*shape, generator=GEN, dtype=torch.float64)).to(dtype).cuda()


def save(tag, *tensors):
    """tag.<i>.bin per output; a None output (a gradient nobody wanted) leaves tag.<i>.none"""
    global COUNT
    for i, t in enumerate(tensors):
        path = os.path.join(OUT, "%s.%d" % (tag, i))
        if t is None:
            open(path + ".none", "wb").close()
        else:
            with open(path + ".bin", "wb") as f:
                f.write(t.detach().cpu().contiguous().numpy().tobytes())
        COUNT += 1


def tname(dtype):
    return "f64" if dtype == F64 else "f32"


def offset_view(t):
    """The same values in a buffer that starts one element past a 16-byte boundary."""
    big = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    big[1:].copy_(t.reshape(-1))
    return big[1:].view(t.shape)


# ---------------------------------------------------------------- diagonal Gaussian
def diag_gaussian(L):
    # fp32: D = 64 the four-columns-per-lane kernel; 6 / 130 one / three columns per lane; 300 the generic kernel;
    # D = 64 one element off alignment leaves the 16-byte kernel; B = 16389 x 130 is past 4096 workgroups, where the
    # second row in flight exists.  fp64 always takes the generic kernel.
    cases = [(3, 64, F32, False), (3, 6, F32, False), (3, 130, F32, False), (3, 300, F32, False), (3, 64, F32, True),
             (16389, 130, F32, False), (3, 5, F64, False)]
    for b, d, dt, off in cases:
        tag = "diag_b%d_d%d_%s%s" % (b, d, tname(dt), "_off" if off else "")
        x, loc, ls = rnd(b, d, dtype=dt), rnd(d, dtype=dt), rnd(d, dtype=dt, scale=0.3)
        if off:
            x = offset_view(x)
        for temp in (None, 0.7):
            t = "%s_t%s" % (tag, "1" if temp is None else "07")
            save(t + "_lp", L.diag_gaussian_log_prob(x, loc, ls, temp))
            save(t + "_lp_acc", L.diag_gaussian_log_prob(x, loc, ls, temp, logp=rnd(b, dtype=dt), sign=-1.0))
            save(t + "_sample", *L.diag_gaussian_sample(x, loc, ls, temp))


# ---------------------------------------------------------------- affine / maf / masked / const / permute / split / merge
def affine_family(L):
    b, c, t_off, d_t = 5, 6, 2, 3
    perm = torch.tensor([4, 0, 5, 2, 1, 3], dtype=torch.int32).cuda()
    for dt in (F32, F64):
        for inner in (1, 3):
            shape = (b, c) if inner == 1 else (b, c, inner)
            tail = () if inner == 1 else (inner,)
            z = rnd(*shape, dtype=dt)
            tag = "i%d_%s" % (inner, tname(dt))
            for inv in (False, True):
                d = "inv" if inv else "fwd"
                for sm in (L.SCALE_EXP, L.SCALE_SIGMOID, L.SCALE_SIGMOID_INV, L.SCALE_NONE):
                    param = rnd(b, (1 if sm == L.SCALE_NONE else 2) * d_t, *tail, dtype=dt, scale=0.5)
                    save("affine_%s_m%d_%s" % (tag, sm, d), *L.affine_coupling(z, param, t_off, d_t, sm, inv))
                    save("affine_%s_m%d_%s_acc" % (tag, sm, d),
                         *L.affine_coupling(z, param, t_off, d_t, sm, inv, logdet=rnd(b, dtype=dt), sign=-1.0))
                s, t = rnd(c, dtype=dt, scale=0.5), rnd(c, dtype=dt)
                save("const_%s_%s" % (tag, d), L.affine_const(z, s, t, inv))
            save("permute_%s" % tag, L.permute(z, perm))
        z = rnd(b, c, dtype=dt)
        tag = tname(dt)
        for inv in (False, True):
            d = "inv" if inv else "fwd"
            save("maf_%s_%s" % (tag, d), *L.maf_affine(z, rnd(b, 2 * c, dtype=dt), inv))
            s, t = rnd(b, c, dtype=dt, scale=0.5), rnd(b, c, dtype=dt)
            mask = (torch.arange(c) % 2).to(dt).cuda()
            save("masked_%s_%s" % (tag, d), *L.masked_affine(z, s, t, mask, inv))
            save("masked_%s_%s_acc" % (tag, d), *L.masked_affine(z, s, t, mask, inv, logdet=rnd(b, dtype=dt), sign=-1.0))
            save("masked_%s_%s_nos" % (tag, d), *L.masked_affine(z, None, t, mask, inv))
        pa, pb = L.split_columns(z, perm, 2)
        save("split_%s" % tag, pa, pb)
        save("merge_%s" % tag, L.merge_columns(pa, pb, perm))


# ---------------------------------------------------------------- class-conditional Gaussian
def class_cond(L):
    # (C, P): (3, 4) packs inside a channel, (8, 1) flat rows, (3, 5) scalar accesses.  With a row index over R = 4
    # rows that holds one label outside the table (its sample's outputs are NaN), and without one at R = 1.
    b = 7
    labels = torch.tensor([0, 3, 1, 9, 2, 1, 0], dtype=torch.int32).cuda()
    for dt in (F32, F64):
        for c, p in ((3, 4), (8, 1), (3, 5)):
            for idx, r in ((labels, 4), (None, 1)):
                tag = "cc_c%d_p%d_%s_%s" % (c, p, "idx" if idx is not None else "r1", tname(dt))
                z, loc, ls = rnd(b, c, p, dtype=dt), rnd(r, c, dtype=dt), rnd(r, c, dtype=dt, scale=0.3)
                g, gz = rnd(b, dtype=dt), rnd(b, c, p, dtype=dt)
                for temp in (None, 0.7):
                    t = "%s_t%s" % (tag, "1" if temp is None else "07")
                    save(t + "_lp", L.cc_gaussian_log_prob(z, loc, ls, idx, p, temp))
                    save(t + "_lp_acc", L.cc_gaussian_log_prob(z, loc, ls, idx, p, temp, logp=rnd(b, dtype=dt), sign=-1.0))
                    save(t + "_sample", *L.cc_gaussian_sample(z, loc, ls, idx, p, temp))
                    save(t + "_lp_bwd", *L.cc_gaussian_log_prob_bwd(z, loc, ls, idx, p, temp, g))
                    save(t + "_sample_bwd", *L.cc_gaussian_sample_bwd(z, ls, idx, p, temp, gz, g))
            save("cc_reduce_c%d_p%d_%s" % (c, p, tname(dt)), L.cc_gaussian_reduce_rows(rnd(b, c, dtype=dt), labels, 4))


# ---------------------------------------------------------------- Gaussian mixture
def mixture(L):
    # (M, D): (3, 8) packs; (5, 3) V = 1; (2, 1040) fp32: rows beyond the register packs; (8192, 1) fp64: no LDS room
    # for the per-mode constants.  B = 1 and 70 (more than one wave of samples in the VJP).
    cases = [(3, 8, F32), (3, 8, F64), (5, 3, F32), (5, 3, F64), (2, 1040, F32), (8192, 1, F64)]
    for m, d, dt in cases:
        loc, ls = rnd(m, d, dtype=dt, scale=2.0), rnd(m, d, dtype=dt, scale=0.3)
        log_w = torch.log_softmax(rnd(m, dtype=dt), 0)
        for b in (1, 70):
            tag = "gmm_m%d_d%d_b%d_%s" % (m, d, b, tname(dt))
            z, g = rnd(b, d, dtype=dt, scale=2.0), rnd(b, dtype=dt)
            mode = (torch.arange(b) % m).to(torch.int32)
            if b > 1:
                mode[3] = m                                   # one mode outside the table: NaN row
            lp = L.gmm_log_prob(z, loc, ls, log_w)
            save(tag + "_lp", lp)
            save(tag + "_lp_acc", L.gmm_log_prob(z, loc, ls, log_w, logp=rnd(b, dtype=dt), sign=-1.0))
            save(tag + "_sample", *L.gmm_sample(z, mode.cuda(), loc, ls, log_w))
            save(tag + "_bwd", *L.gmm_log_prob_bwd(z, loc, ls, log_w, lp, g))
            save(tag + "_bwd_dz", *L.gmm_log_prob_bwd(z, loc, ls, log_w, lp, g, tables=False))
        save(tag + "_bwd_gz", *L.gmm_log_prob_bwd(z, loc, ls, log_w, lp, g, gz_in=rnd(b, d, dtype=dt)))


# ---------------------------------------------------------------- heavy-tailed bases
def heavy_tail(L):
    # D = 8 packs, 3 scalar accesses; D = 520 fp32: 130 packs > 128, the VJP kernel in which a lane owns a pack of
    # columns.  B = 1 and 70.
    cases = [(8, F32), (8, F64), (3, F32), (3, F64), (520, F32)]
    for fam in (L.TAIL_STUDENT_T, L.TAIL_GEN_GAUSSIAN):
        for d, dt in cases:
            loc, ls, cst = rnd(d, dtype=dt), rnd(d, dtype=dt, scale=0.3), rnd(d, dtype=dt)
            shape = pos(d, dtype=dt, lo=1.5, hi=30.0) if fam == L.TAIL_STUDENT_T else pos(d, dtype=dt, lo=0.6, hi=2.5)
            for b in (1, 70):
                tag = "tail_f%d_d%d_b%d_%s" % (fam, d, b, tname(dt))
                z, gamma, g, gz = rnd(b, d, dtype=dt), pos(b, d, dtype=dt, lo=0.1), rnd(b, dtype=dt), rnd(b, d, dtype=dt)
                save(tag + "_lp", L.tail_log_prob(z, loc, ls, shape, cst, fam))
                save(tag + "_lp_acc", L.tail_log_prob(z, loc, ls, shape, cst, fam, logp=rnd(b, dtype=dt), sign=-1.0))
                save(tag + "_sample", *L.tail_sample(z, gamma, loc, ls, shape, cst, fam))
                save(tag + "_lp_bwd", *L.tail_log_prob_bwd(z, loc, ls, shape, fam, g))
                save(tag + "_lp_bwd_gz", *L.tail_log_prob_bwd(z, loc, ls, shape, fam, g, gz_in=gz))
                save(tag + "_lp_bwd_dz", *L.tail_log_prob_bwd(z, loc, ls, shape, fam, g, rows=False))
                save(tag + "_sample_bwd", *L.tail_sample_bwd(z, gamma, loc, ls, shape, fam, g_z=gz, g_lp=g))
                save(tag + "_sample_bwd_norows", *L.tail_sample_bwd(z, gamma, loc, ls, shape, fam, g_z=gz, g_lp=g, rows=False))
                save(tag + "_sample_bwd_noeps", *L.tail_sample_bwd(z, gamma, loc, ls, shape, fam, g_z=gz, g_lp=g, want_eps=False))
                save(tag + "_sample_bwd_gz", *L.tail_sample_bwd(z, gamma, loc, ls, shape, fam, g_z=gz))


def compare(a, b):
    fa, fb = sorted(os.listdir(a)), sorted(os.listdir(b))
    if fa != fb:
        print("different sets of outputs: only in %s %s, only in %s %s" % (a, sorted(set(fa) - set(fb)), b, sorted(set(fb) - set(fa))))
        return 1
    bad = [f for f in fa if open(os.path.join(a, f), "rb").read() != open(os.path.join(b, f), "rb").read()]
    nbytes = sum(os.path.getsize(os.path.join(a, f)) for f in fa)
    print("%d outputs, %d bytes: %d differ%s" % (len(fa), nbytes, len(bad), "".join("\n  " + f for f in bad)))
    return 1 if bad else 0


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
        for part in (diag_gaussian, affine_family, class_cond, mixture, heavy_tail):
            part(_lib)
    torch.cuda.synchronize()
    print("%s: %d outputs from %s" % (OUT, COUNT, os.path.dirname(_lib.__file__)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
