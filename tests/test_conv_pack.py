"""nets/cnn.py::pack_conv1x1 against the packed layout's definition, written as explicit loops in numpy (CPU, no GPU):
entry [rb, ks, h, lane, i] is the hi (h = 0) or lo (h = 1) fp16 half of w[32 rb + lane % 32, 16 ks + 8 (lane / 32) + i],
zero for rows at or beyond c_out; hi = fp16(w), lo = fp16((w - hi) * 2048).  Bit-exact through the float32 view.  The
shapes: fewer rows than one block, the 1x1 layer's own 256 rows, the tap matrices of 5 and 56 output channels (2 and
16 row blocks, the last one partly filled)."""
import numpy as np
import pytest
import torch

from vcnf_amd.nets.cnn import pack_conv1x1


def reference_pack(w, row_blocks):
    c_out, c_in = w.shape
    out = np.zeros((row_blocks, c_in // 16, 2, 64, 8), dtype=np.float16)
    for rb in range(row_blocks):
        for ks in range(c_in // 16):
            for lane in range(64):
                row = 32 * rb + lane % 32
                if row >= c_out:
                    continue
                for i in range(8):
                    v = w[row, 16 * ks + 8 * (lane // 32) + i]
                    hi = np.float16(v)
                    out[rb, ks, 0, lane, i] = hi
                    out[rb, ks, 1, lane, i] = np.float16((v - np.float32(hi)) * np.float32(2048.0))
    return out.reshape(-1).view(np.float32)


@pytest.mark.parametrize("c_out,c_in,row_blocks", [(7, 16, 8), (256, 96, 8), (45, 256, 2), (504, 256, 16)])
def test_pack_conv1x1_layout(c_out, c_in, row_blocks):
    g = torch.Generator().manual_seed(1000 * c_out + c_in)
    w = torch.randn(c_out, c_in, generator=g) * torch.logspace(-3, 1, c_in)      # halves of every magnitude
    got = pack_conv1x1(w, row_blocks=row_blocks)
    assert got.dtype == torch.float32 and got.dim() == 1 and got.is_contiguous()
    want = reference_pack(w.numpy(), row_blocks)
    assert got.numel() == want.size == row_blocks * (c_in // 16) * 2 * 64 * 4
    assert np.array_equal(got.numpy().view(np.uint32), want.view(np.uint32))
