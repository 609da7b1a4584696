"""Host cost of a HIT on the derived-buffer caches, per call, on CPU tensors (packing works on them, as in
tests/test_fused_pack.py; no GPU needed): fused.packed_weights with the key given (as fused.run calls it) and without,
fused_affine.packed_weights, Permute._idx32 and the coupling's _index32.

    python profiles/tools/hit_path.py [CHECKOUT]

Minimum over 7 rounds of 20000 calls, in ns."""
import os
import sys
import timeit

ROOT = os.path.abspath(sys.argv[1]) if len(sys.argv) > 1 else os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import torch            # noqa: E402
import vcnf_amd as nf   # noqa: E402
from vcnf_amd import fused, fused_affine  # noqa: E402


def main():
    torch.manual_seed(0)
    cp = nf.flows.CoupledRationalQuadraticSpline(64, 2, 128, 8, num_context_channels=16).prqct
    blk = nf.flows.AffineCouplingBlock(nf.nets.MLP([16, 64, 64, 32]))
    swap, shuffle = nf.flows.Permute(32, mode="swap"), nf.flows.Permute(32, mode="shuffle")
    cpu = torch.device("cpu")
    key = fused._param_key(cp)
    rows = (("fused._param_key", lambda: fused._param_key(cp)),
            ("fused.packed_weights(cp, prec, key)", lambda: fused.packed_weights(cp, fused.PREC_F16X3, key)),
            ("fused.packed_weights(cp)", lambda: fused.packed_weights(cp)),
            ("coupling._index32('tf')", lambda: cp._index32('tf')),
            ("fused_affine.packed_weights(block)", lambda: fused_affine.packed_weights(blk)),
            ("Permute('swap')._idx32", lambda: swap._idx32(False, cpu)),
            ("Permute('shuffle')._idx32", lambda: shuffle._idx32(False, cpu)))
    print(os.path.dirname(nf.__file__))
    for name, fn in rows:
        fn()
        print("%-40s %8.0f ns" % (name, min(timeit.repeat(fn, number=20000, repeat=7)) / 20000 * 1e9), flush=True)


if __name__ == "__main__":
    main()
