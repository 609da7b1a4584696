"""The fp64 entry points of image-shaped spline couplings and of the masked affine autoregressive flow
(vcnf_rqs_elementwise_strided_f64, vcnf_rqs_packed_bwd_f64, vcnf_maf_affine_f64): declared, exported, bound, and their
host-side argument validation returns the documented status codes.  No GPU needed: nothing is launched (every call below
fails validation or has n == 0, and the fake pointers are never dereferenced)."""
import ctypes

import vcnf_amd
from vcnf_amd import _lib

from test_abi import declared_symbols

STRIDED, PACKED, MAF = "vcnf_rqs_elementwise_strided_f64", "vcnf_rqs_packed_bwd_f64", "vcnf_maf_affine_f64"
FAKE = 0x1000


def test_symbols_declared_exported_and_bound():
    declared = declared_symbols()
    so = ctypes.CDLL(_lib.lib_path())
    for name in (STRIDED, PACKED, MAF):
        assert name in declared and hasattr(so, name), name
    cfg64 = ctypes.POINTER(_lib.RqsCfg64)
    args, ret = _lib.PROTOTYPES[STRIDED]
    assert len(args) == 17 and args[13] is cfg64 and ret is ctypes.c_int
    # same arity and argument kinds as the fp32 twin, the configuration aside
    assert args[:13] == _lib.PROTOTYPES["vcnf_rqs_elementwise_strided_f32"][0][:13]
    args, ret = _lib.PROTOTYPES[PACKED]
    assert len(args) == 12 and args[9] is cfg64 and ret is ctypes.c_int
    args, ret = _lib.PROTOTYPES[MAF]
    assert len(args) == 10 and args[8] is ctypes.c_double and ret is ctypes.c_int


def _cfg(k=8, tails="linear", **kw):
    return _lib.make_cfg(k, tails, tail_bound=3.0, **kw).f64


def _strided(cfg, n=4, rows=(23, 23, 23), inner=5, ks=5, period=0, null_at=None):
    ptrs = [ctypes.c_void_p(FAKE)] * 6           # x, uw, uh, ud, y, logabsdet
    if null_at is not None:
        ptrs[null_at] = None
    x, uw, uh, ud, y, lad = ptrs
    return vcnf_amd.lib().vcnf_rqs_elementwise_strided_f64(x, uw, uh, ud, *rows, inner, ks, period, y, lad, n,
                                                           ctypes.byref(cfg) if cfg is not None else None, 0, None,
                                                           None)


def _packed(cfg, n=4, inner=5, lad_div=10, null_at=None):
    ptrs = [ctypes.c_void_p(FAKE)] * 6           # x, params, g_y, g_logabsdet, g_x, g_params
    if null_at is not None:
        ptrs[null_at] = None
    x, p, gy, gl, gx, gp = ptrs
    return vcnf_amd.lib().vcnf_rqs_packed_bwd_f64(x, p, inner, lad_div, gy, gl, gx, gp, n,
                                                  ctypes.byref(cfg) if cfg is not None else None, 0, None)


def _maf(batch=4, features=7, params=FAKE, ld_mode=_lib.LD_STORE, null_at=None):
    ptrs = [ctypes.c_void_p(FAKE), ctypes.c_void_p(params), ctypes.c_void_p(FAKE), ctypes.c_void_p(FAKE)]
    if null_at is not None:
        ptrs[null_at] = None
    return vcnf_amd.lib().vcnf_maf_affine_f64(*ptrs, batch, features, 0, ld_mode, 1.0, None)


def test_strided_validation_status_codes():
    # status codes of include/vcnf_hip.h: 1 NULL, 2 SHAPE, 4 VALUE, 5 UNSUPPORTED
    assert _strided(None) == 1
    assert _strided(_cfg(0)) == 2 and _strided(_cfg(65)) == 2
    bad = _cfg()
    bad.tails = 7
    assert _strided(bad) == 5
    assert _strided(_cfg(min_bin_width=0.2)) == 4 and _strided(_cfg(min_bin_height=0.2)) == 4
    assert _strided(_cfg(), n=-1) == 2
    for i in range(3):
        rows = [23, 23, 23]
        rows[i] = -1
        assert _strided(_cfg(), rows=tuple(rows)) == 2
    assert _strided(_cfg(), inner=0) == 2
    assert _strided(_cfg(), ks=0) == 2
    assert _strided(_cfg(), period=-1) == 2
    assert _strided(_cfg(), n=0) == 0 and _strided(_cfg(), n=0, null_at=0) == 0
    for i in range(6):
        assert _strided(_cfg(), null_at=i) == 1, i
    assert _strided(_cfg(64, None), rows=(193, 193, 193), null_at=5) == 1
    assert _strided(_cfg(2, "circular"), null_at=5) == 1


def test_packed_bwd_validation_status_codes():
    assert _packed(None) == 1
    assert _packed(_cfg(0)) == 2 and _packed(_cfg(65)) == 2
    assert _packed(_cfg(1, "linear")) == 2
    bad = _cfg()
    bad.tails = 7
    assert _packed(bad) == 5
    assert _packed(_cfg(min_bin_width=0.2)) == 4 and _packed(_cfg(min_bin_height=0.2)) == 4
    assert _packed(_cfg(), n=-1) == 2
    assert _packed(_cfg(), inner=0) == 2
    assert _packed(_cfg(), lad_div=0) == 2
    assert _packed(_cfg(), n=0) == 0 and _packed(_cfg(), n=0, null_at=1) == 0
    for i in range(6):
        assert _packed(_cfg(), null_at=i) == 1, i
    assert _packed(_cfg(64, None), null_at=5) == 1
    assert _packed(_cfg(1, "circular"), null_at=5) == 1


def test_maf_validation_status_codes():
    # 3 ALIGN: params are read as double2, so they must be 16-byte aligned
    assert _maf(batch=-1) == 2 and _maf(features=0) == 2
    assert _maf(ld_mode=7) == 5
    assert _maf(batch=0) == 0 and _maf(batch=0, null_at=0) == 0
    for i in range(4):
        assert _maf(null_at=i) == 1, i
    assert _maf(params=FAKE + 8) == 3
    assert _maf(params=FAKE + 4) == 3
    # the fp32 twin accepts 8-byte aligned params (float2): the fp64 check is its own
    assert vcnf_amd.lib().vcnf_maf_affine_f32(ctypes.c_void_p(FAKE), ctypes.c_void_p(FAKE + 8), None,
                                              ctypes.c_void_p(FAKE), 4, 7, 0, _lib.LD_STORE, 1.0, None) == 1
