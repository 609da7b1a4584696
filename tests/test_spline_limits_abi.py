"""vcnf_rqs_elementwise_limits_{f32,f64} and their VJPs vcnf_rqs_elementwise_limits_bwd_{f32,f64} (the functional spline
with tensor interval limits): declared, exported, bound, and their host-side argument validation returns the documented
status codes.  No GPU needed: nothing is launched (every call below fails validation or has n == 0, and the fake
pointer is never dereferenced)."""
import ctypes

import pytest

import vcnf_amd
from vcnf_amd import _lib

from test_abi import declared_symbols

FWD = ("vcnf_rqs_elementwise_limits_f32", "vcnf_rqs_elementwise_limits_f64")
BWD = ("vcnf_rqs_elementwise_limits_bwd_f32", "vcnf_rqs_elementwise_limits_bwd_f64")
NAMES = FWD + BWD
# data pointers whose NULL is an error when n > 0: forward x, uw, uh, ud, left, right, bottom, top, y, logabsdet;
# VJP x, uw, uh, ud, left, right, bottom, top, g_y, g_logabsdet, g_x, g_uw, g_uh, g_ud (the four limit gradients
# are optional)
N_DATA = {"fwd": 10, "bwd": 14}


def _cfg_type(name):
    return _lib.RqsCfg64 if name.endswith("_f64") else _lib.RqsCfg


@pytest.mark.parametrize("name", NAMES)
def test_symbol_declared_exported_and_bound(name):
    assert name in declared_symbols()
    assert hasattr(ctypes.CDLL(_lib.lib_path()), name)
    args, ret = _lib.PROTOTYPES[name]
    n_args, i_bcast, i_cfg = (19, 11, 15) if name in FWD else (26, 11, 23)
    assert len(args) == n_args and ret is ctypes.c_int
    assert args[i_bcast] is ctypes.POINTER(_lib.RqsLimitBcast)
    assert args[i_cfg] is ctypes.POINTER(_cfg_type(name))


def test_bcast_struct_layout():
    assert ctypes.sizeof(_lib.RqsLimitBcast) == 64     # int64 period[4], inner[4]
    assert ctypes.sizeof(_lib.RqsCfg) == 40            # the existing config struct is unchanged


def _bc(period=(8, 8, 1, 4), inner=(1, 1, 1, 2)):
    return _lib.RqsLimitBcast((ctypes.c_int64 * 4)(*period), (ctypes.c_int64 * 4)(*inner))


def _call(name, cfg, n=8, ld=(8, 8, 9), bcast="default", null_at=None, limit_grads=True):
    fake = ctypes.c_void_p(0x1000)
    fwd = name in FWD
    ptrs = [fake] * N_DATA["fwd" if fwd else "bwd"]
    if null_at is not None:
        ptrs[null_at] = None
    bc = _bc() if bcast == "default" else bcast
    bcp = ctypes.byref(bc) if bc is not None else None
    cfgp = ctypes.byref(cfg) if cfg is not None else None
    fn = getattr(vcnf_amd.lib(), name)
    if fwd:
        x, uw, uh, ud, l, r, b, t, y, lad = ptrs
        return fn(x, uw, uh, ud, *ld, l, r, b, t, bcp, y, lad, n, cfgp, 0, None, None)
    x, uw, uh, ud, l, r, b, t, gy, gl, gx, gw, gh, gd = ptrs
    glim = [fake if limit_grads else None] * 4
    return fn(x, uw, uh, ud, *ld, l, r, b, t, bcp, gy, gl, gx, gw, gh, gd, *glim, n, cfgp, 0, None)


def _cfg(name, k=8, tails=None, **kw):
    c = _lib.make_cfg(k, tails, tail_bound=3.0, **kw)
    return c.f64 if name.endswith("_f64") else c


@pytest.mark.parametrize("name", NAMES)
def test_validation_status_codes(name):
    # status codes of include/vcnf_hip.h: 1 NULL, 2 SHAPE, 4 VALUE, 5 UNSUPPORTED
    assert _call(name, None) == 1
    # K out of range
    assert _call(name, _cfg(name, 0)) == 2
    assert _call(name, _cfg(name, 65)) == 2
    # negative n / leading dimensions
    assert _call(name, _cfg(name), n=-1) == 2
    for i in range(3):
        ld = [8, 8, 9]
        ld[i] = -1
        assert _call(name, _cfg(name), ld=tuple(ld)) == 2
    # period or inner below 1, for each of the four limits
    for j in range(4):
        for field in ("period", "inner"):
            period, inner = [8, 8, 1, 4], [1, 1, 1, 2]
            (period if field == "period" else inner)[j] = 0
            assert _call(name, _cfg(name), bcast=_bc(period, inner)) == 2, (j, field)
            (period if field == "period" else inner)[j] = -3
            assert _call(name, _cfg(name), bcast=_bc(period, inner)) == 2, (j, field)
    # no broadcast description
    assert _call(name, _cfg(name), bcast=None) == 1
    # min_bin_width * K > 1, min_bin_height * K > 1
    assert _call(name, _cfg(name, min_bin_width=0.2)) == 4
    assert _call(name, _cfg(name, min_bin_height=0.2)) == 4
    # the functional spline has no tails: every other tails code is unsupported
    assert _call(name, _cfg(name, tails="linear")) == 5
    assert _call(name, _cfg(name, tails="circular")) == 5
    bad = _cfg(name)
    bad.tails = 7
    assert _call(name, bad) == 5
    # n == 0: nothing to do, even with NULL data pointers
    assert _call(name, _cfg(name), n=0) == 0
    for i in range(N_DATA["fwd" if name in FWD else "bwd"]):
        assert _call(name, _cfg(name), n=0, null_at=i) == 0, i
    # any NULL data pointer when n > 0
    for i in range(N_DATA["fwd" if name in FWD else "bwd"]):
        assert _call(name, _cfg(name), null_at=i) == 1, i
    # the largest bin count passes validation up to the pointers
    assert _call(name, _cfg(name, 64), ld=(64, 64, 65), null_at=0) == 1


@pytest.mark.parametrize("name", BWD)
def test_limit_gradients_are_optional(name):
    # NULL limit gradients are "not wanted", not an error: validation still stops at the first NULL data pointer
    assert _call(name, _cfg(name), null_at=13, limit_grads=False) == 1
    assert _call(name, _cfg(name), n=0, limit_grads=False) == 0
