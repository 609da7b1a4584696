"""Phase stamps of the large-batch fused RQS layer kernel (csrc/fused_layer_v6.hip, 128-sample tiles), config C3's layer.

Needs a library whose v6 translation unit (two residual blocks) was compiled with -DVCNF_TIME=1:
    VCNF_OBJ_DIR=scratch/obj python -m vcnf_amd.build
    hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -fno-slp-vectorize -DVCNF_V6_NBLK=2 -DVCNF_TIME=1 \
        -c vcnf_amd/csrc/fused_layer_v6.hip -o scratch/v6_time.o
    hipcc --offload-arch=gfx950 -shared -fPIC -o scratch/libvcnf_time.so $(ls scratch/obj/*.o | grep -v fused_layer_v6_b2.o) scratch/v6_time.o
    VCNF_LIB=$PWD/scratch/libvcnf_time.so python profiles/tools/v6_phase_timing.py [batch] [into] [pair]
"into": the accumulating calls of a flow (inverse_into / forward_into: log-det added onto a running log-density, one
value per row) instead of the store-mode ones.
"pair": two layers per tile visit (csrc/fused_layer_v6_pair.hip, compiled with -DVCNF_TIME=1 as well and linked in place
of fused_layer_v6_pair_b2.o); a tile's slots then hold the steps of BOTH layers, slots 0, 1 and 12 run once per tile.
Waves 0 (group A) and 4 (group B) of workgroup 0 sum the shader cycles of every step over the tiles the workgroup walks;
the timing build keeps them in a buffer of its own (vcnf_v6_phase_stamps), the layer's results are untouched.  Printed:
cycles per tile.  A wave's slots add up to its whole tile; the four waits that shift group B one step behind group A
and re-align the groups are what the other group's step costs beside an idle half of the CU.
"""
import ctypes
import os
import sys
sys.path[:0] = [os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))]
import torch
import vcnf_amd as nf
from vcnf_amd import _lib

NAMES = ["tail of the previous tile (store) + loop top", "x rows, context -> LDS", "identity half + first-layer fragments",
         "M0: first layer", "V1: publish", "M: block layers (sum)", "V: publish, block first layer (sum)",
         "V: gate + residual + publish (sum)", "last-layer operand fragments + bias", "first window DMA + wait",
         "round M (sum)", "round V (sum)", "log|det| exchange, range flag", "after the last tile", "(unused)",
         "barriers between steps (sum)", "WAIT group B: A runs M0", "WAIT group A: B's last trunk V",
         "WAIT group B: A's first round M", "WAIT group A: B's last round V"]
SLOTS = 24
torch.manual_seed(0)
B = int(sys.argv[1]) if len(sys.argv) > 1 else 1 << 20
INTO, PAIR = "into" in sys.argv[2:], "pair" in sys.argv[2:]
lay = nf.flows.CoupledRationalQuadraticSpline(64, 2, 128, 8, num_context_channels=16).cuda().eval()
lay2 = nf.flows.CoupledRationalQuadraticSpline(64, 2, 128, 8, num_context_channels=16, reverse_mask=True).cuda().eval()
handle = _lib.lib()
STAMPS = "vcnf_v6_pair_phase_stamps" if PAIR else "vcnf_v6_phase_stamps"
if not hasattr(handle, STAMPS):
    sys.exit("this library was not built with -DVCNF_TIME=1 (see the docstring)")
stamps = getattr(handle, STAMPS)
stamps.argtypes, stamps.restype = [ctypes.c_void_p], ctypes.c_int


def pair_call(dirn, xb, cb, lq):
    from vcnf_amd import fused as fz
    order = [lay2, lay] if dirn == "inverse" else [lay, lay2]
    end, run, sig = fz.plan_stack(order, 0, xb, cb)
    assert end == 2
    fz.run_stack(run, sig, xb, cb, dirn == "forward", lq if INTO else None, 1.0 if dirn == "inverse" else -1.0)


with torch.no_grad():
    xb, cb = torch.randn(B, 64, device="cuda"), torch.randn(B, 16, device="cuda")
    lq = torch.randn(B, device="cuda")
    for dirn in ("inverse", "forward"):
        for _ in range(3):
            if PAIR:
                pair_call(dirn, xb, cb, lq)
            else:
                getattr(lay, dirn + "_into")(xb, lq, context=cb) if INTO else getattr(lay, dirn)(xb, context=cb)
        torch.cuda.synchronize()
        out = (ctypes.c_float * (2 * SLOTS))()
        assert stamps(ctypes.cast(out, ctypes.c_void_p)) == 0
        for w in (0, 1):
            v = [float(f) for f in out[w * SLOTS:(w + 1) * SLOTS]]
            tiles = max(v[22], 1.0)
            print("%s%s, wave %d (group %s): %d tiles, %.0f shader cycles in all, %.2f us, in-kernel clock %.0f MHz" % (
                "density" if dirn == "inverse" else "sampling", " (accumulate)" if INTO else "", 4 * w, "AB"[w], tiles, v[20], v[21] / 100.0,
                100.0 * v[20] / max(v[21], 1.0)))
            for i, n in enumerate(NAMES):
                if i != 14:
                    print("    %2d %-48s %9.0f cycles per tile" % (i, n, v[i] / tiles))
            print("       %-48s %9.0f" % ("sum", sum(v[:20]) / tiles))
