"""The table of grid caps (tests/grid_caps.py) against the source: CPU only.

Every cap is found in the .hip file that defines it; every case gets past its cap by the restated launch rules with a
ragged third trip; no tensor of a case is larger than 12 M elements; and the .hip files with a loop strided by gridDim.x
are exactly the files the table covers plus its commented exclusion list, so a new looping unit cannot arrive without a
case."""
import re

import pytest

import grid_caps as gc


@pytest.mark.parametrize("name", sorted(gc.CONSTANTS))
def test_constant_is_in_the_source(name):
    assert gc.constant(name) >= 1


def test_a_missing_constant_is_an_error(monkeypatch):
    monkeypatch.setitem(gc.CONSTANTS, "gone", ("affine_kernels.hip", gc._constexpr("kNoSuchCap"), 1))
    with pytest.raises(LookupError):
        gc.constant("gone")
    monkeypatch.setitem(gc.CONSTANTS, "twice", ("rqs_kernels.hip", r"elem_blocks\(\w+, kBlock, ([^)]+)\)", 1))
    with pytest.raises(LookupError):                       # 256 * 16 four times and 256 * 8 once: count and values differ
        gc.constant("twice")


def test_the_caps_the_tests_were_written_for():
    """The values at the time the cases were sized.  A changed cap is not an error of the kernel: the cases follow it,
    this assertion is the reminder to look at their sizes and times again."""
    want = {"affine.cap": 4096, "cc.cap": 4096, "target.cap": 2048, "stoch.cap": 2048, "tail.fwd_cap": 2048,
            "gmm.fwd_cap": 2048, "pr.fwd_cap": 4096, "pr.bwd_cap": 1024, "mvn.fwd_cap": 512, "mvn.bwd_cap": 256,
            "stoch.bwd_cap": 1024, "rqs.elem_cap": 4096, "rqs.bwd_cap": 4096, "rqs64.cap": 8192,
            "rqs.shared_bwd_threads": 262144, "tail.bwd_hi": 2048, "gmm.bwd_hi": 4096,
            "conv1.cap": 256, "conv1.pix": 64, "conv31.cap": 256, "conv31.pix": 64, "mix.cap": 4096, "mix.pix": 128,
            "mix.block": 256, "faffine.cap": 2048, "faffine.block": 256, "trunk.cap": 2048}
    assert {k: gc.constant(k) for k in want} == want


def test_restated_launch_rules():
    assert [gc.pick_lanes(n) for n in (0, 1, 2, 3, 4, 5, 33, 64, 65, 1000)] == [1, 1, 2, 4, 4, 8, 64, 64, 64, 64]
    assert gc.grid_for(0, 1, 256, 4096) == 1 and gc.grid_for(257, 1, 256, 4096) == 2
    assert gc.grid_for(10 ** 9, 64, 256, 4096) == 4096 and gc.grid_for(9, 64, 256, 4096) == 3
    assert [gc.pick_pack(d, False) for d in (1, 2, 3, 4, 6, 8, 130)] == [1, 2, 1, 4, 2, 4, 2]
    assert [gc.pick_pack(d, True) for d in (1, 2, 3, 4, 130)] == [1, 2, 1, 2, 2]
    assert [gc.pr_checkpoint_every(d) for d in (2, 32, 33, 130, 256)] == [4, 4, 5, 17, 32]
    # the python restatements next to the source they restate
    src = gc.source("stream_common.hpp")
    assert "while (G < 64 && G < n) G <<= 1;" in src and "const long long per_block = block / G;" in src
    assert "return D > 32 ? (D + 7) / 8 : 4;" in gc.source("planar_radial.hip")


@pytest.mark.parametrize("name", sorted(gc.CASES))
def test_case_crosses_its_cap(name):
    c = gc.CASES[name]
    assert c.tiles >= 2 * c.cap + 1, c.describe()
    assert c.trips >= 3
    # the workgroups run out in the middle of the last trip, and the last workgroup's rows in the middle of a workgroup
    last = c.tiles - (c.trips - 1) * c.cap
    assert 1 <= last < c.cap, c.describe()
    items = c.B * c.items_per_row
    assert items % c.per_block != 0 or c.per_block == 1, c.describe()
    if c.per_block > 1:
        assert items % c.per_block == c.remainder or c.items_per_row > 1
    assert c.kind in ("narrow", "wide", "tile"), c.describe()
    if c.kind == "narrow":
        assert c.B * c.items_per_row > 2 * c.cap * c.rule.worst
    elif c.kind == "wide":
        assert c.rule.lanes == 64, c.describe()
    else:                                                   # a fixed tile per workgroup and trip: 2 x cap + 1 tiles exactly
        assert c.rule.worst == c.per_block and c.tiles == 2 * c.cap + 1, c.describe()
    assert c.elements <= gc.MAX_ELEMENTS, c.describe()
    # the windows of the row-independence checks lie inside the batch and fit into a first trip and a ragged rest
    for lo, hi in c.windows():
        assert 0 <= lo < hi <= c.B
    (tail_lo, tail_hi), (lo, hi) = c.windows()
    assert tail_hi == c.B and lo < c.rows_per_trip < hi and hi - lo == gc.STRADDLE
    assert c.trip_rows(0)[0] == 0 and c.trip_rows(c.trips - 1)[1] == c.B


def test_wide_and_narrow_cases_exist_for_the_lane_group_units():
    for stem in ("affine.coupling", "affine.masked", "affine.maf", "affine.diag_gaussian", "cc.fwd", "tail.fwd", "gmm.fwd", "pr.fwd", "pr.bwd"):
        for t in ("f32", "f64"):
            assert "%s.narrow.%s" % (stem, t) in gc.CASES and "%s.wide.%s" % (stem, t) in gc.CASES, stem
    for t in ("f32", "f64"):
        k, d = gc.CASES["pr.bwd.ckpt." + t].shape["K"], gc.CASES["pr.bwd.ckpt." + t].shape["D"]
        assert (k - 1) // gc.pr_checkpoint_every(d) >= 1            # a checkpoint row exists
    # the matrix kernels: both staging variants of conv1x1, each with an even and an odd count of k-steps (the DMA
    # request loop treats odd counts specially) and a partial row block; the ROWS instance of channel_mix and the image one
    conv1 = [gc.CASES["conv1x1.%s.f32" % n] for n in ("dma", "dma_odd", "regs", "regs_rows")]
    for dma in (True, False):
        mine = [c for c in conv1 if c.shape["dma"] == dma]
        assert all((c.items_per_row % 4 == 0) == dma for c in mine)             # what the launcher decides on (aligned x)
        assert {c.shape["c_in"] // 16 for c in mine} == {1, 3} and any(c.shape["c_out"] % 32 for c in mine)
    assert {gc.CASES["mix.%s.f32" % n].shape["rows"] for n in ("rows", "rows8", "image")} == {True, False}
    assert all(gc.CASES["mix.%s.f32" % n].items_per_row == 1 for n in ("rows", "rows8"))
    assert gc.CASES["faffine.layer_odd.f32"].shape["D"] % 4 and not gc.CASES["faffine.layer.f32"].shape["D"] % 4


def test_matrix_kernel_batches():
    """The batches of the "tile" cases as they were sized (a changed cap moves them: look at the times again)."""
    want = {"conv1x1.dma": 8201, "conv1x1.dma_odd": 8201, "conv1x1.regs": 10934, "conv1x1.regs_rows": 32801,
            "conv3x3_1x1": 5467, "convnet3": 5467, "mix.rows": 1048641, "mix.rows8": 1048641, "mix.image": 349547,
            "faffine.layer": 262177, "faffine.layer_odd": 262177, "faffine.stack": 262177}
    assert {k: gc.CASES[k + ".f32"].B for k in want} == want
    assert sorted(k[:-4] for k, c in gc.CASES.items() if c.kind == "tile") == sorted(want)
    # the launch loops the rules restate
    assert "for (long long tile = blockIdx.x; tile < ntiles; tile += gridDim.x)" in gc.source("conv1x1.hip")
    assert "for (long long tile = blockIdx.x; tile < ntiles; tile += gridDim.x)" in gc.source("conv3x3_1x1.hip")
    assert "t = (long long)blockIdx.x * (kMixBlock / 64) + wave; t < ntiles; t += stride" in gc.source("channel_mix.hip")
    assert gc.source("fused_affine.hip").count("wt = blockIdx.x + (long long)gridDim.x * wave; wt < nwt; wt += wstride") == 2
    assert "#define VCNF_FA_NCB 1" in gc.source("fused_affine.hip")


def test_looping_files_are_the_covered_and_the_excluded():
    files = gc.looping_files()
    assert files, "no .hip file found under " + gc.CSRC
    assert not set(gc.COVERED) & set(gc.EXCLUDED)
    assert sorted(gc.COVERED + tuple(gc.EXCLUDED)) == files, (
        "every .hip file with a gridDim.x-strided loop needs cases in tests/grid_caps.py (COVERED) or an entry in its "
        "exclusion list with a reason: %s" % sorted(set(files) ^ set(gc.COVERED + tuple(gc.EXCLUDED))))
    assert all(len(reason) > 20 for reason in gc.EXCLUDED.values())
    # the kernels of the covered files that are named as left out exist under those names
    for path, kernels in gc.NOT_COVERED.items():
        assert path in gc.COVERED
        for k in kernels:
            assert re.search(r"void %s\(" % k, gc.source(path)), "%s: no kernel %s" % (path, k)


def test_table_prints():
    lines = gc.table().splitlines()
    assert len(lines) == len(gc.CASES) and all("x cap" in line for line in lines)
