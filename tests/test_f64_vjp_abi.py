"""vcnf_rqs_elementwise_bwd_f64 (the VJP of the fp64 spline): declared, exported, bound, and its host-side argument
validation returns the documented status codes.  No GPU needed: nothing is launched (every call below fails
validation or has n == 0, and the fake pointer is never dereferenced)."""
import ctypes

import vcnf_amd
from vcnf_amd import _lib

from test_abi import declared_symbols

NAME = "vcnf_rqs_elementwise_bwd_f64"


def test_symbol_declared_exported_and_bound():
    assert NAME in declared_symbols()
    assert hasattr(ctypes.CDLL(_lib.lib_path()), NAME)
    args, ret = _lib.PROTOTYPES[NAME]
    assert len(args) == 17 and args[14] is ctypes.POINTER(_lib.RqsCfg64) and ret is ctypes.c_int


def _call(cfg, n=4, ld=(8, 8, 7), null_at=None):
    fake = ctypes.c_void_p(0x1000)
    ptrs = [fake] * 10                # x, uw, uh, ud, g_y, g_logabsdet, g_x, g_uw, g_uh, g_ud
    if null_at is not None:
        ptrs[null_at] = None
    x, uw, uh, ud, gy, gl, gx, gw, gh, gd = ptrs
    return vcnf_amd.lib().vcnf_rqs_elementwise_bwd_f64(x, uw, uh, ud, *ld, gy, gl, gx, gw, gh, gd, n,
                                                       ctypes.byref(cfg) if cfg is not None else None, 0, None)


def _cfg(k=8, tails="linear", **kw):
    return _lib.make_cfg(k, tails, tail_bound=3.0, **kw).f64


def test_validation_status_codes():
    # status codes of include/vcnf_hip.h: 1 NULL, 2 SHAPE, 4 VALUE, 5 UNSUPPORTED
    assert _call(None) == 1
    # K out of range, linear tails with one bin
    assert _call(_cfg(0)) == 2
    assert _call(_cfg(65)) == 2
    assert _call(_cfg(1, "linear")) == 2
    # negative n / leading dimensions
    assert _call(_cfg(), n=-1) == 2
    for i in range(3):
        ld = [8, 8, 7]
        ld[i] = -1
        assert _call(_cfg(), ld=tuple(ld)) == 2
    # unknown tails
    bad = _cfg()
    bad.tails = 7
    assert _call(bad) == 5
    # min_bin_width * K > 1, min_bin_height * K > 1
    assert _call(_cfg(min_bin_width=0.2)) == 4
    assert _call(_cfg(min_bin_height=0.2)) == 4
    # n == 0: nothing to do, even with NULL data pointers
    assert _call(_cfg(), n=0) == 0
    assert _call(_cfg(), n=0, null_at=0) == 0
    # any NULL data pointer when n > 0
    for i in range(10):
        assert _call(_cfg(), null_at=i) == 1, i
    # the other tails modes and bin counts pass validation up to the pointers
    assert _call(_cfg(1, "circular"), null_at=9) == 1
    assert _call(_cfg(64, None), ld=(64, 64, 65), null_at=9) == 1
