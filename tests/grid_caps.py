"""The grid caps of the stream kernels, read from the source, and the batch shapes that get past them.

Every stream unit of vcnf_amd/csrc caps its grid and lets a workgroup loop over further rows or tiles ("trips").  This
module (a plain helper, not a conftest) holds
  * CONSTANTS: every cap, found with a regular expression in the .hip file that defines it (``constant`` raises when a
    pattern no longer matches: a renamed or re-typed cap must be restated here);
  * the launchers' rules restated in Python: ``pick_lanes``, ``grid_for``, ``pick_pack`` and, per kernel, the lanes per
    row and the rows a workgroup takes per trip (the rule_* functions);
  * CASES: per kernel a shape whose batch is B = 2 * rows_per_trip + r with rows_per_trip = cap x rows per workgroup,
    so that every workgroup makes two full trips and the third one is ragged: r = per_block / 2 + 1 rows (5 where a
    workgroup takes one row), which ends inside a workgroup and, where lanes are grouped, inside a wave.
    "narrow" cases have 2 - 5 features and a batch sized for one lane per row (B > 2 * cap * block: past the cap
    whatever lane count the launcher picks); "wide" cases have rows for which the restated rule gives 64 lanes;
    "tile" cases belong to the matrix kernels (conv1x1, conv3x3_1x1, channel_mix, fused_affine), whose workgroups take
    a fixed tile of pixels or rows per trip whatever the shape: B holds 2 x cap + 1 tiles, the last one ragged.
test_grid_caps_table.py checks the table on the CPU, test_gpu_grid_caps.py runs the cases."""
import glob
import os
import re
from collections import namedtuple

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "vcnf_amd", "csrc")
MAX_ELEMENTS = 12 * 1000 * 1000          # per tensor of a case
STRADDLE = 257                           # rows of the window across the boundary between trip 1 and trip 2


def source(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _value(expr):
    """A cap as the source writes it: integers, LL suffixes, *, /, <<, parentheses."""
    expr = re.sub(r"(?<=\d)LL\b", "", expr.strip())
    if not re.fullmatch(r"[\d\s*/()<]+", expr):
        raise ValueError("not a constant expression: %r" % expr)
    return int(eval(expr.replace("/", "//"), {"__builtins__": {}}))


def _constexpr(name):
    return r"constexpr\s+(?:int|long long)\s+%s\s*=\s*([^;]+);" % name


_LOCAL_CAP = r"const long long cap = ([^;]+);"          # the matrix kernels' launchers

# name -> (file, pattern with one group, occurrences expected).  Every occurrence must give the same value.
CONSTANTS = {
    "affine.block": ("affine_kernels.hip", _constexpr("kBlock"), 1),
    "affine.cap": ("affine_kernels.hip", _constexpr("kMaxBlocks"), 1),
    "cc.block": ("class_cond_gaussian.hip", _constexpr("kBlock"), 1),
    "cc.cap": ("class_cond_gaussian.hip", _constexpr("kMaxBlocks"), 1),
    "gmm.fwd_block": ("gaussian_mixture.hip", _constexpr("kFwdBlock"), 1),
    "gmm.bwd_block": ("gaussian_mixture.hip", _constexpr("kBwdBlock"), 1),
    "gmm.reg_packs": ("gaussian_mixture.hip", _constexpr("kRegPacks"), 1),
    "gmm.fwd_cap": ("gaussian_mixture.hip", _constexpr("kMaxFwdBlocks"), 1),
    "gmm.bwd_ws": ("gaussian_mixture.hip", r"long long cap = (\(1LL << \d+\)) / elems;", 1),
    "gmm.bwd_lo": ("gaussian_mixture.hip", r"cap = cap < (\d+) \? \1 : cap > \d+ \? \d+ : cap;", 1),
    "gmm.bwd_hi": ("gaussian_mixture.hip", r"cap = cap < \d+ \? \d+ : cap > (\d+) \? \1 : cap;", 1),
    "gmm.bwd_rows": ("gaussian_mixture.hip", r"long long n = \(batch \+ \d+\) / (\d+);", 1),
    "tail.block": ("heavy_tail.hip", _constexpr("kBlock"), 1),
    "tail.reg_packs": ("heavy_tail.hip", _constexpr("kRegPacks"), 1),
    "tail.fwd_cap": ("heavy_tail.hip", _constexpr("kMaxFwdBlocks"), 1),
    "tail.bwd_ws": ("heavy_tail.hip", r"long long cap = (\(1LL << \d+\)) / \(3LL \* D\);", 1),
    "tail.bwd_lo": ("heavy_tail.hip", r"cap = cap < (\d+) \? \1 : cap > \d+ \? \d+ : cap;", 1),
    "tail.bwd_hi": ("heavy_tail.hip", r"cap = cap < \d+ \? \d+ : cap > (\d+) \? \1 : cap;", 1),
    "tail.bwd_rows": ("heavy_tail.hip", r"const long long n = \(batch \+ \d+\) / (\d+);", 1),
    "mvn.block": ("mvn_lds.hpp", _constexpr("kBlock"), 1),
    "mvn.tile_f32": ("mvn_lds.hpp", r"tile_rows\(\) \{ return sizeof\(T\) == 4 \? (\d+) : \d+; \}", 1),
    "mvn.tile_f64": ("mvn_lds.hpp", r"tile_rows\(\) \{ return sizeof\(T\) == 4 \? \d+ : (\d+); \}", 1),
    "mvn.fwd_cap": ("mvn_base.hip", _constexpr("kMaxFwdBlocks"), 1),
    "mvn.bwd_ws": ("mvn_base.hip", _constexpr("kMaxWorkspace"), 1),
    "mvn.bwd_cap": ("mvn_base.hip", _constexpr("kMaxGroups"), 1),
    "mvn.bwd_rows": ("mvn_base.hip", r"const long long n = \(batch \+ \d+\) / (\d+);", 1),
    "pr.block": ("planar_radial.hip", _constexpr("kBlock"), 1),
    "pr.lane_el": ("planar_radial.hip", _constexpr("kLaneEl"), 1),
    "pr.fwd_cap": ("planar_radial.hip", _constexpr("kMaxFwdBlocks"), 1),
    "pr.bwd_ws": ("planar_radial.hip", _constexpr("kMaxWsElems"), 1),
    "pr.bwd_cap": ("planar_radial.hip", _constexpr("kMaxBwdGroups"), 1),
    "target.block": ("target_density.hip", _constexpr("kBlock"), 1),
    "target.cap": ("target_density.hip", _constexpr("kMaxBlocks"), 1),
    "stoch.block": ("stochastic.hip", _constexpr("kBlock"), 1),
    "stoch.cap": ("stochastic.hip", _constexpr("kMaxBlocks"), 1),
    "stoch.bwd_cap": ("stochastic.hip", _constexpr("kMaxBwdGroups"), 1),
    "mstack.cap": ("masked_affine_stack.hip", r"if \(blocks > ([^)]+)\) blocks = \1;", 2),
    "mstack.rows": ("masked_affine_stack.hip", r"long long blocks = \(batch \+ \d+\) / (\d+);", 2),
    "resblock.cap": ("resblock_ops.hip", r"if \(blocks > ([^)]+)\) blocks = \1;", 1),
    "resblock.block": ("resblock_ops.hip", r"long long blocks = \(work \+ \d+\) / (\d+);", 1),
    "rqs.block": ("rqs_kernels.hip", _constexpr("kBlock"), 1),
    "rqs.elem_cap": ("rqs_kernels.hip", r"elem_blocks\(n, kBlock, ([^)]+)\)", 4),
    "rqs.bwd_block": ("rqs_backward.hip", _constexpr("kBwdBlock"), 1),
    "rqs.bwd_cap": ("rqs_backward.hip", r"elem_blocks\((?:a\.)?n, kBwdBlock, ([^)]+)\)", 2),
    "rqs.bwd_lds": ("rqs_backward.hip", r"\(size_t\)kBwdBlock \* P \* sizeof\(float\) <= (48 \* 1024);", 1),
    "rqs.shared_bwd_threads": ("rqs_backward.hip", r"long long g = (\(256LL \* 1024\)) / period;", 1),
    "rqs64.cap": ("rqs_f64.hip", r"grid64\(int64_t n\) \{ return dim3\(elem_blocks\(n, 256, ([^)]+)\)\); \}", 1),
    # the matrix kernels: a local ``cap`` in the launcher
    "conv1.pix": ("conv1x1.hip", _constexpr("kC1Pix"), 1),
    "conv1.cap": ("conv1x1.hip", _LOCAL_CAP, 1),
    "conv31.pix": ("conv3x3_1x1.hip", _constexpr("kC31Pix"), 1),
    "conv31.cap": ("conv3x3_1x1.hip", _LOCAL_CAP, 1),
    "mix.block": ("channel_mix.hip", _constexpr("kMixBlock"), 1),
    "mix.cap": ("channel_mix.hip", _LOCAL_CAP, 1),
    "mix.pix": ("channel_mix.hip", r"const long long blocks = \(a\.npix \+ \d+\) / (\d+);", 1),
    "faffine.block": ("fused_affine.hip", _constexpr("kFABlock"), 1),
    "faffine.cap": ("fused_affine.hip", _LOCAL_CAP, 2),
    "trunk.cap": ("resnet_trunk.hip", _LOCAL_CAP, 1),
}


def constant(name):
    """The value of CONSTANTS[name] in the source.  Raises when the pattern is not found as often as expected or its
    occurrences disagree."""
    path, pattern, count = CONSTANTS[name]
    found = re.findall(pattern, source(path))
    if len(found) != count:
        raise LookupError("%s: %d matches of %r in %s, expected %d" % (name, len(found), pattern, path, count))
    values = {_value(x) for x in found}
    if len(values) != 1:
        raise LookupError("%s: the occurrences in %s disagree: %s" % (name, path, sorted(values)))
    return values.pop()


def looping_files():
    """The .hip files with a loop strided by gridDim.x."""
    return sorted(os.path.basename(p) for p in glob.glob(os.path.join(CSRC, "*.hip")) if "gridDim.x" in source(os.path.basename(p)))


# files whose looping kernels have cases here
COVERED = ("affine_kernels.hip", "channel_mix.hip", "class_cond_gaussian.hip", "conv1x1.hip", "conv3x3_1x1.hip",
           "fused_affine.hip", "gaussian_mixture.hip", "heavy_tail.hip", "masked_affine_stack.hip", "mvn_base.hip",
           "planar_radial.hip", "resblock_ops.hip", "rqs_backward.hip", "rqs_f64.hip", "rqs_kernels.hip",
           "stochastic.hip", "target_density.hip")
# looping files without a case, and why.  A new looping file has to be entered in COVERED, with cases, or here, with a reason.
_RQS_LAYER = ("fused RQS layer kernel: its tile walk is covered by tests/test_gpu_fused_handover.py, which runs the "
              "128-sample-tile kernel (fused_layer_v6.hip, 256 workgroups) over 769 tiles - three full trips and a "
              "ragged fourth - bitwise against the 32-sample-tile kernel (fused_layer_v6s.hip) walking the same rows, "
              "and flagged tiles in the first, a middle and the last place of a workgroup's walk against the exact "
              "fp32 kernel (fused_layer.hip)")
EXCLUDED = {
    "fused_layer.hip": _RQS_LAYER,
    "fused_layer_v6.hip": _RQS_LAYER,
    "fused_layer_v6s.hip": _RQS_LAYER,
    "resnet_trunk.hip": ("a workgroup takes two 16-row tiles per wave (128 rows) once B >= 65 536, so two trips of the "
                         "2048 workgroups and a ragged third need B = 524 353 rows, whose [B, 128] output is 67 M elements "
                         "against MAX_ELEMENTS = 12 M here (one tile per wave below 65 536 rows is at most 1024 workgroups: "
                         "no second trip either).  test_gpu_parity.py::test_resnet_trunk_kernel_vs_torch runs the "
                         "two-tile instance at B = 65 557: 513 workgroups, a ragged last one, every one on its first trip "
                         "- a later trip of this kernel is not run by any test"),
}


# ---------------------------------------------------------------- the launchers' rules, restated
def pick_lanes(n):
    g = 1
    while g < 64 and g < n:
        g <<= 1
    return g


def grid_for(groups, g, block, max_blocks):
    per_block = block // g
    return max(1, min(max_blocks, (groups + per_block - 1) // per_block))


def pick_pack(d, f64):
    """Elements per 16-byte pack for rows of d elements in buffers that torch allocated (aligned)."""
    v = 2 if f64 else 4
    while v > 1 and d % v:
        v >>= 1
    return v


Rule = namedtuple("Rule", "per_block cap lanes worst floor", defaults=(0,))
# per_block: items a workgroup takes per trip; cap: workgroups; lanes: lanes per item; worst: per_block with one lane
# per item (what a narrow case is sized for); floor: rows per workgroup below which the launcher starts fewer workgroups
# than the cap (the VJPs' bwd_groups).  An item is a row unless the case says otherwise (items_per_row).


def _rows(g, block, cap, flight=1, floor=0):
    return Rule(flight * (block // g), cap, g, flight * block, floor)


def rule_affine_rows(d, f64=False):
    """affine coupling (d = channels * inner), masked affine, MAF: pick_lanes(d) lanes per row."""
    return _rows(pick_lanes(d), constant("affine.block"), constant("affine.cap"))


def rule_affine_flat():
    """affine const, permute, split / merge: one element per thread."""
    return _rows(1, constant("affine.block"), constant("affine.cap"))


def rule_diag_gaussian(d, f64):
    """fp32 rows of at most four columns per lane keep two rows in flight per lane group and trip."""
    block, cap = constant("affine.block"), constant("affine.cap")
    if not f64 and d % 4 == 0 and d <= 256:
        return _rows(pick_lanes(d // 4), block, cap, flight=2)
    g = pick_lanes(d)
    if not f64 and (d + g - 1) // g <= 4:
        return _rows(g, block, cap, flight=2)
    return _rows(g, block, cap)


def rule_cc_fwd(c, p, f64):
    v = 2 if f64 else 4
    packs = c * p // v if (p % v == 0 or (p == 1 and c % v == 0)) else c * p
    return _rows(pick_lanes(packs), constant("cc.block"), constant("cc.cap"))


def rule_cc_bwd(c, p, f64):
    """Items are (sample, channel) segments, or packs of channels for flat rows: (rule, items per row)."""
    v = 2 if f64 else 4
    block, cap = constant("cc.block"), constant("cc.cap")
    if p % v == 0:
        return _rows(pick_lanes(p // v), block, cap), c
    if p == 1:
        return _rows(1, block, cap), (c // v if c % v == 0 else c)
    return _rows(pick_lanes(p), block, cap), c


def rule_gmm_fwd(d, f64):
    return _rows(pick_lanes(d // pick_pack(d, f64)), constant("gmm.fwd_block"), constant("gmm.fwd_cap"))


def rule_gmm_bwd(d, m, f64):
    cap = constant("gmm.bwd_ws") // (m * (2 * d + 1))
    cap = max(constant("gmm.bwd_lo"), min(constant("gmm.bwd_hi"), cap))
    return _rows(pick_lanes(d // pick_pack(d, f64)), constant("gmm.bwd_block"), cap, floor=constant("gmm.bwd_rows"))


def _tail_lanes(d, f64):
    nv, reg = d // pick_pack(d, f64), constant("tail.reg_packs")
    return pick_lanes((nv + reg - 1) // reg) if nv <= reg * 64 else 64


def rule_tail_fwd(d, f64):
    return _rows(_tail_lanes(d, f64), constant("tail.block"), constant("tail.fwd_cap"))


def rule_tail_bwd(d, f64):
    """The rows kernel (rows of at most kRegPacks * 64 packs)."""
    assert d // pick_pack(d, f64) <= constant("tail.reg_packs") * 64
    cap = constant("tail.bwd_ws") // (3 * d)
    cap = max(constant("tail.bwd_lo"), min(constant("tail.bwd_hi"), cap))
    return _rows(_tail_lanes(d, f64), constant("tail.block"), cap, floor=constant("tail.bwd_rows"))


def _mvn_tile(f64):
    return constant("mvn.tile_f64" if f64 else "mvn.tile_f32")


def rule_mvn_fwd(d, f64):
    ts = _mvn_tile(f64)
    return Rule(ts, constant("mvn.fwd_cap"), constant("mvn.block") // ts, ts)


def rule_mvn_bwd(d, f64):
    ts = _mvn_tile(f64)
    cap = min(constant("mvn.bwd_cap"), constant("mvn.bwd_ws") // (d * d + d + 1))
    return Rule(ts, cap, constant("mvn.block") // ts, ts, constant("mvn.bwd_rows"))


def _pr_lanes(d):
    el = constant("pr.lane_el")
    return pick_lanes((d + el - 1) // el)


def rule_pr_fwd(d, k=1, f64=False):
    return _rows(_pr_lanes(d), constant("pr.block"), constant("pr.fwd_cap"))


def rule_pr_bwd(d, k, f64=False):
    cap = max(1, min(constant("pr.bwd_cap"), constant("pr.bwd_ws") // (k * (2 * d + 2))))
    return _rows(_pr_lanes(d), constant("pr.block"), cap)


def pr_checkpoint_every(d):
    return (d + 7) // 8 if d > 32 else 4


def rule_masked_stack():
    """A run of masked affine layers with their MLPs: 16 lanes per sample, 16 samples per workgroup and trip."""
    rows = constant("mstack.rows")
    return Rule(rows, constant("mstack.cap"), 256 // rows, rows)


def rule_resblock():
    """The residual block's elementwise maps: one element, or one pack of four, per thread."""
    return _rows(1, constant("resblock.block"), constant("resblock.cap"))


def rule_target():
    return _rows(1, constant("target.block"), constant("target.cap"))


def rule_stoch_fwd():
    return _rows(1, constant("stoch.block"), constant("stoch.cap"))


def rule_stoch_bwd():
    return _rows(1, constant("stoch.block"), constant("stoch.bwd_cap"))


def rule_rqs_elem(f64=False):
    return _rows(1, 256 if f64 else constant("rqs.block"), constant("rqs64.cap") if f64 else constant("rqs.elem_cap"))


def rule_rqs_bwd(f64=False):
    """The elementwise VJPs: a workgroup takes a block of kBwdBlock elements per trip (fp64: one element per thread)."""
    return _rows(1, 256 if f64 else constant("rqs.bwd_block"), constant("rqs64.cap") if f64 else constant("rqs.bwd_cap"))


def rqs_bwd_packed(inner, k, nd):
    """bwd_launch's choice for the operands of vcnf_rqs_packed_bwd_f32 (logits and gradients in one layout): the variant
    that stages a workgroup's block of rows in LDS, with the barriers between one trip's block and the next."""
    return inner == 1 and constant("rqs.bwd_block") * (2 * k + nd) * 4 <= constant("rqs.bwd_lds")


def rule_rqs_shared_bwd(period):
    """Thread (group sg, position f) walks the samples sg, sg + groups, ...: a group takes one row per trip."""
    return Rule(1, max(1, constant("rqs.shared_bwd_threads") // period), 1, 1)


def _tiles(per_block, cap, lanes):
    """A workgroup takes ``per_block`` consecutive items per trip whatever the shape: kind "tile"."""
    return Rule(per_block, cap, lanes, per_block)


def rule_conv_tile(unit):
    """conv1x1.hip ("conv1") and conv3x3_1x1.hip ("conv31"): an item is a pixel of the batch (items_per_row = H W); an
    8-wave workgroup takes one pass of 64 consecutive pixels per trip, tile = blockIdx + trip * gridDim."""
    return _tiles(constant(unit + ".pix"), constant(unit + ".cap"), 8)


def rule_channel_mix():
    """channel_mix.hip: an item is a pixel (a row of a [B, C] matrix); wave w of workgroup g takes the pass
    4 g + w + trip * 4 gridDim of 2 tiles x 16 pixels, so a workgroup takes 4 waves x 2 x 16 = 128 consecutive pixels
    per trip - the divisor of the launcher's ``blocks`` line."""
    waves = constant("mix.block") // 64
    per_block = waves * 2 * 16
    assert per_block == constant("mix.pix"), "channel_mix.hip: the grid is no longer sized for 2 tiles of 16 pixels per wave"
    return _tiles(per_block, constant("mix.cap"), 2)


def rule_fused_affine():
    """fused_affine.hip (layer and stack kernels; one 16-row column block per wave, VCNF_FA_NCB = 1): an item is a batch
    row.  The four waves of workgroup g do NOT take neighbouring wave-tiles: with G = gridDim they take the 16-row
    wave-tiles g + G (w + 4 trip), w = 0 .. 3, i.e. g, g + G, g + 2 G, g + 3 G on the first trip.  A trip of the whole
    grid still covers 4 G consecutive wave-tiles = 64 G consecutive rows, so per_block = 64 rows and rows_per_trip =
    64 cap hold, while "the rows of workgroup g" are four runs of 16 rows G wave-tiles apart.  The remainder of 33 rows
    makes three wave-tiles of the third trip, the last one with a single row."""
    waves = constant("faffine.block") // 64
    return _tiles(waves * 16, constant("faffine.cap"), 4)


# ---------------------------------------------------------------- cases
class Case(namedtuple("Case", "name rule kind items_per_row row_elements shape")):
    """One shape past a cap.  ``items_per_row``: items of the kernel's loop per batch row (1 for the row kernels);
    ``row_elements``: elements per batch row of the case's widest tensor."""

    @property
    def per_block(self):
        return self.rule.per_block

    @property
    def cap(self):
        return self.rule.cap

    @property
    def items_per_trip(self):
        return self.rule.cap * self.rule.per_block

    @property
    def remainder(self):
        return 5 if self.rule.per_block == 1 else self.rule.per_block // 2 + 1

    @property
    def items(self):
        """Items of the call: two full trips of the sizing workgroup and the remainder."""
        sized = self.rule.worst if self.kind == "narrow" else self.rule.per_block
        return max(2 * self.rule.cap * sized, self.rule.cap * self.rule.floor) + self.remainder

    @property
    def B(self):
        """Rows that hold ``items``; where a row is several items, one row more if the last workgroup came out full."""
        b = -(-self.items // self.items_per_row)
        while self.rule.per_block > 1 and b * self.items_per_row % self.rule.per_block == 0:
            b += 1
        return b

    @property
    def rows_per_trip(self):
        """Whole rows of the first trip (the boundary between trip 1 and trip 2 lies in or after row rows_per_trip)."""
        return self.items_per_trip // self.items_per_row

    @property
    def tiles(self):
        """Workgroup-trips the call needs."""
        return -(-self.B * self.items_per_row // self.rule.per_block)

    @property
    def trips(self):
        return -(-self.tiles // self.rule.cap)

    @property
    def elements(self):
        return self.B * self.row_elements

    def windows(self):
        """(first row, end row) of the row sets run again as batches of their own: the last full trip with the ragged
        tail (as a batch of its own a first trip and r rows of a second), and STRADDLE rows across the boundary between
        trip 1 and trip 2."""
        tail = max(0, self.B - self.rows_per_trip - -(-self.remainder // self.items_per_row))
        lo = self.rows_per_trip - STRADDLE // 2
        return ((tail, self.B), (lo, lo + STRADDLE))

    def trip_rows(self, trip):
        """(first row, end row) of the rows wholly inside trip 0, 1, ...; the last trip runs to B."""
        lo = -(-trip * self.items_per_trip // self.items_per_row)
        hi = (trip + 1) * self.items_per_trip // self.items_per_row
        return lo, min(hi, self.B)

    def describe(self):
        return "%-34s %-6s cap %5d  per_block %4d  rows/trip %8d  B %8d  tiles %7d (%.2f x cap)  max tensor %5.2f M" % (
            self.name, self.kind, self.cap, self.per_block, self.rows_per_trip, self.B, self.tiles,
            self.tiles / self.cap, self.elements / 1e6)


def _case(name, rule, kind, row_elements, items_per_row=1, **shape):
    return Case(name, rule, kind, items_per_row, row_elements, shape)


def _build():
    cases = []
    for f64 in (False, True):
        t = "f64" if f64 else "f32"
        add = lambda name, *a, **kw: cases.append(_case("%s.%s" % (name, t), *a, f64=f64, **kw))
        # affine family: rows of D, D = 130 gives 64 lanes
        for kind, d in (("narrow", 3), ("wide", 130)):
            t_off, d_t = d // 3, d - d // 3 - (1 if d > 3 else 0)    # the transformed columns; two parameters each
            add("affine.coupling." + kind, rule_affine_rows(d), kind, max(d, 2 * d_t), D=d, t_off=t_off, d_t=d_t)
            add("affine.masked." + kind, rule_affine_rows(d), kind, d, D=d)
        # MAF reads two parameters per element, the fp32 Gaussian keeps two rows in flight: D = 2 keeps them in bounds
        for kind, d in (("narrow", 2), ("wide", 130)):
            add("affine.maf." + kind, rule_affine_rows(d), kind, 2 * d, D=d)
            add("affine.diag_gaussian." + kind, rule_diag_gaussian(d, f64), kind, d, D=d)
        for op in ("const", "permute", "split", "merge"):
            add("affine.%s.narrow" % op, rule_affine_flat(), "narrow", 3, items_per_row=3, D=3)
        # class-conditional Gaussian: rows of C * P
        for kind, c, p in (("narrow", 3, 1), ("wide", 10, 16)):
            add("cc.fwd." + kind, rule_cc_fwd(c, p, f64), kind, c * p, C=c, P=p)
        for kind, c, p in (("narrow", 3, 1), ("narrow_pixels", 2, 2), ("wide", 2, 136)):
            rule, per_row = rule_cc_bwd(c, p, f64)
            add("cc.bwd." + kind, rule, "narrow" if kind != "wide" else "wide", c * p, items_per_row=per_row, C=c, P=p)
        # Gaussian mixture
        add("gmm.fwd.narrow", rule_gmm_fwd(2, f64), "narrow", 2, D=2, M=3)
        add("gmm.fwd.wide", rule_gmm_fwd(130, f64), "wide", 130, D=130, M=3)
        add("gmm.bwd.narrow", rule_gmm_bwd(2, 3, f64), "narrow", 2, D=2, M=3)
        # heavy tail
        add("tail.fwd.narrow", rule_tail_fwd(3, f64), "narrow", 3, D=3)
        add("tail.fwd.wide", rule_tail_fwd(130, f64), "wide", 130, D=130)
        add("tail.bwd.narrow", rule_tail_bwd(3, f64), "narrow", 3, D=3)
        add("tail.bwd.wide", rule_tail_bwd(130, f64), "wide", 130, D=130)
        # full-covariance bases: a tile of samples per workgroup and trip
        for d in (3, 17):
            add("mvn.fwd.D%d" % d, rule_mvn_fwd(d, f64), "narrow", d, D=d)
            add("mvn.bwd.D%d" % d, rule_mvn_bwd(d, f64), "narrow", d, D=d)
        # Planar / Radial: K = 5 at D = 2 has a checkpoint row (every = 4), D = 130 has 64 lanes
        for kind, d, k in (("narrow", 2, 3), ("ckpt", 2, 5), ("wide", 130, 5)):
            widest = max(d, k, (k - 1) // pr_checkpoint_every(d) * d)      # the row, its trace [K], its checkpoints
            add("pr.fwd." + kind, rule_pr_fwd(d, k), "narrow" if d == 2 else "wide", widest, D=d, K=k)
            add("pr.bwd." + kind, rule_pr_bwd(d, k), "narrow" if d == 2 else "wide", widest, D=d, K=k)
        # 2-D targets and the stochastic layers (K = 2 layers: noise [K, B, 2])
        add("target.narrow", rule_target(), "narrow", 2, D=2)
        add("stoch.hmc_fwd.narrow", rule_stoch_fwd(), "narrow", 4, D=2, K=2, steps=2)
        add("stoch.hmc_bwd.narrow", rule_stoch_bwd(), "narrow", 4, D=2, K=2, steps=2)
        add("stoch.mh.narrow", rule_stoch_fwd(), "narrow", 4, D=2, steps=2)
        # elementwise splines with batch-shared logit rows (period 32, or one row for all, with or without
        # tensor limits): one element per thread
        add("rqs.strided.narrow", rule_rqs_elem(f64), "narrow", 32, items_per_row=32, period=32, bins=8)
        # elementwise spline VJPs: one logit gradient row per element, so two bins (the fewest linear tails take) keep the
        # tensors in bounds
        add("rqs.bwd.dense", rule_rqs_bwd(f64), "narrow", 2, bins=2, tails="linear")
        # the reference drivers' models: K x [masked affine with MLPs, ActNorm] in one launch, D = 15, H = 30
        add("mstack.narrow", rule_masked_stack(), "narrow", 15, D=15, H=30)
    # packed rows of 3 elements per sample: the per-sample cotangent of log|det| changes inside a workgroup's block
    cases.append(_case("rqs.bwd.packed.f32", rule_rqs_bwd(), "narrow", 15, items_per_row=3, f64=False, bins=2, tails="linear", C=3))
    cases.append(_case("rqs.bwd.limits.f32", rule_rqs_bwd(), "narrow", 3, f64=False, bins=2, tails=None))
    # residual-block maps (fp32 only): a row is an element, or a pack of four
    cases.append(_case("resblock.scalar.f32", rule_resblock(), "narrow", 1, f64=False, pack=1))
    cases.append(_case("resblock.vec.f32", rule_resblock(), "narrow", 4, f64=False, pack=4))
    f32 = lambda name, *a, **kw: cases.append(_case(name + ".f32", *a, f64=False, **kw))
    f32("rqs.shared.narrow", rule_rqs_elem(), "narrow", 32, items_per_row=32, period=32, bins=8)
    f32("rqs.shared_bwd.narrow", rule_rqs_shared_bwd(32), "narrow", 32, period=32, bins=8)
    # ---- the matrix kernels (fp32 only): the smallest shapes that still reach the cap, 2 x cap + 1 tiles each
    def image(name, rule, c_widest, h, w, **shape):
        f32(name, rule, "tile", c_widest * h * w, items_per_row=h * w, H=h, W=w, **shape)
    # conv1x1: KS = c_in / 16 k-steps.  2 x 2 images in torch's aligned buffers take the DMA staging (inner % 4 == 0),
    # 1 x 3 and 1 x 1 images the register staging; 33 output channels leave the second row block partial
    image("conv1x1.dma", rule_conv_tile("conv1"), 16, 2, 2, c_in=16, c_out=7, dma=True)
    image("conv1x1.dma_odd", rule_conv_tile("conv1"), 48, 2, 2, c_in=48, c_out=33, dma=True)
    image("conv1x1.regs", rule_conv_tile("conv1"), 16, 1, 3, c_in=16, c_out=7, dma=False)
    image("conv1x1.regs_rows", rule_conv_tile("conv1"), 48, 1, 1, c_in=48, c_out=33, dma=False)
    # conv3x3 + conv1x1 (256 hidden / output channels): every pixel of a 2 x 3 image is on a border, a pass of 64
    # pixels holds ten images and two parts; convnet3 adds the nine taps (its widest tensor is z [B, 9 c_out, H, W])
    image("conv3x3_1x1", rule_conv_tile("conv31"), 256, 2, 3, c_in=2)
    image("convnet3", rule_conv_tile("conv31"), 9 * 5, 2, 3, c_in=3, c_out=5)
    # channel mixing: [B, C] matrices (the ROWS instances, 16-byte stores) and an image whose pixel count is odd
    f32("mix.rows", rule_channel_mix(), "tile", 4, C=4, rows=True)
    f32("mix.rows8", rule_channel_mix(), "tile", 8, C=8, rows=True)
    image("mix.image", rule_channel_mix(), 4, 1, 3, C=4, rows=False)
    # fused affine coupling: one layer (D = 33: scalar strip copies, 16 + 1 output rows) and C1's stack of four
    f32("faffine.layer", rule_fused_affine(), "tile", 4, D=4, hidden=32, mode="channel", scale_map="exp")
    f32("faffine.layer_odd", rule_fused_affine(), "tile", 33, D=33, hidden=32, mode="channel_inv", scale_map="sigmoid_inv")
    f32("faffine.stack", rule_fused_affine(), "tile", 2, D=2, widths=(1, 32, 32, 2), layers=4)
    return {c.name: c for c in cases}


CASES = _build()

# Kernels of the covered files whose cases are NOT here, and why: the coupling and conditioner-input kernels belong to
# the fused path, whose full-size tests run them at 1 M rows.
NOT_COVERED = {
    "rqs_kernels.hip": ("rqs_coupling_kernel", "rqs_coupling_pf_kernel", "rqs_conditioner_input_kernel"),
}
# Entry points without a case although their kernel has one.  vcnf_rqs_packed_bwd_f64 launches the strided instance of
# rqs_elementwise_bwd_f64_kernel (no LDS stage; the dense instance runs past the cap): its smallest row is 3 logits per
# element (one bin, circular tails; linear tails need two bins and 5 logits), and 3 x (2 x 8192 x 256 + r) elements are
# 12.58 M, over MAX_ELEMENTS.  vcnf_rqs_elementwise_limits_bwd_f64 (the tensor-limit instance of that kernel; no tails, so
# 3 derivative logits at 2 bins) is over it in the same way.
NOT_COVERED_ENTRY_POINTS = ("vcnf_rqs_packed_bwd_f64", "vcnf_rqs_elementwise_limits_bwd_f64")


def table():
    return "\n".join(c.describe() for c in CASES.values())


if __name__ == "__main__":
    print(table())
