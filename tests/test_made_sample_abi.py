"""The one-launch sampling kernel of the autoregressive flows (csrc/made_sample.hip) without a GPU: its entry points are
declared in the header, read by vcnf_amd/_abi.py, exported and bound; the host-side validation returns the documented
status codes before anything is launched; ``vcnf_made_sample_supported`` answers from the LDS budget; the layers carry
the ``fuse_sampling`` switch and CPU tensors keep the loop."""
import ctypes

import pytest
import torch

import made_sample_ref as R
import vcnf_amd as nf
from vcnf_amd import _abi, _lib, build, made_sample

FAKE = ctypes.c_void_p(0x1000)         # never dereferenced: validation fails first / batch == 0
ODD = ctypes.c_void_p(0x1002)          # not aligned to a float or a double
NAMES = ["vcnf_made_sample_f32", "vcnf_made_sample_f64", "vcnf_made_sample_supported", "vcnf_made_sample_lanes",
         "vcnf_made_sample_pack_elems"]


def test_entry_points_in_the_header_with_prototypes():
    with open(build.HEADER) as f:
        text = f.read()
    abi = _abi.read(build.HEADER)
    for name in NAMES:
        assert name + "(" in text, name
        assert name in abi.functions and name in _lib.PROTOTYPES, name
    for sfx, real, cfg in (("f32", "float", "vcnf_rqs_cfg"), ("f64", "double", "vcnf_rqs_cfg_f64")):
        ret, args = abi.decls["vcnf_made_sample_" + sfx]
        assert ret == "int" and len(args) == 18
        assert args[:8] == ["const %s*" % real, real + "*", real + "*"] + ["const %s*" % real] * 3 + ["int64_t", "const int32_t*"]
        assert args[8:] == ["int64_t"] + ["int32_t"] * 4 + ["const %s*" % cfg, "int", real, "int32_t*", "void*"]
    assert abi.decls["vcnf_made_sample_supported"] == ("int", ["int32_t"] * 5)
    assert "made_sample.hip" in build.SOURCES and "rqs_math64.hpp" in build.HEADERS


def test_symbols_exported_and_bound():
    handle = ctypes.CDLL(_lib.lib_path())
    for name in NAMES:
        assert hasattr(handle, name), "libvcnf_hip.so does not export " + name
        assert getattr(nf.lib(), name).argtypes == _lib.PROTOTYPES[name][0]
    assert callable(_lib.made_sample) and callable(_lib.made_sample_supported)


def test_supported_answers_from_the_lds_budget():
    L = nf.lib()
    assert L.vcnf_made_sample_supported(16, 128, 2, 23, 4) == 1
    assert L.vcnf_made_sample_supported(16, 1 << 20, 2, 23, 4) == 0            # an absurd hidden width
    assert not _lib.made_sample_supported(16, 1 << 20, 2, 23, 4)
    for bad in ((0, 8, 1, 2, 4), (1, 0, 1, 2, 4), (1, 8, -1, 2, 4), (1, 8, 1, 1, 4), (1, 8, 1, 2, 2), (2000, 8, 1, 2, 4),
                (4, 8, 17, 2, 4), (4, 8, 1, 3 * 65, 4)):
        assert L.vcnf_made_sample_supported(*bad) == 0, bad
    # splines (both precisions invert with the fp64 spline): the bin counts with an instance (8, 10, 16), every tails
    # mode; the affine map always
    for k, ok in ((8, 1), (10, 1), (16, 1), (4, 0), (12, 0)):
        for p in (3 * k - 1, 3 * k, 3 * k + 1):
            assert L.vcnf_made_sample_supported(6, 32, 1, p, 8) == ok and L.vcnf_made_sample_supported(6, 32, 1, p, 4) == ok
    assert L.vcnf_made_sample_supported(6, 32, 1, 2, 8) == 1 and L.vcnf_made_sample_supported(6, 32, 1, 2, 4) == 1
    # a sample keeps (1 + 2 nb) H + D values and P doubles; 256 / lanes samples fit 48 KiB, or with 64 lanes 64 KiB
    for d, h, nb, p, es in ((1, 8, 1, 2, 4), (16, 128, 2, 23, 4), (16, 128, 2, 23, 8), (64, 256, 2, 23, 4), (64, 256, 2, 23, 8),
                            (7, 4, 2, 2, 8), (16, 512, 2, 23, 4), (16, 768, 2, 23, 4)):
        lanes = L.vcnf_made_sample_lanes(d, h, nb, p, es)
        need = (1 + 2 * nb) * h + d + p * (8 // es)
        assert lanes in (8, 16, 32, 64) and (256 // lanes) * need * es <= (48 << 10 if lanes < 64 else 64 << 10), (d, h, lanes)
        assert lanes == 8 or (256 // (lanes // 2)) * need * es > 48 << 10            # the smallest group that fits
    assert L.vcnf_made_sample_lanes(16, 128, 2, 23, 4) == 16 and L.vcnf_made_sample_lanes(16, 128, 2, 23, 8) == 32
    assert L.vcnf_made_sample_lanes(16, 4096, 2, 23, 4) == 0 and L.vcnf_made_sample_supported(16, 4096, 2, 23, 4) == 0
    assert L.vcnf_made_sample_pack_elems(16, 128, 2, 23) == 128 * 16 + 128 + 2 * (2 * 128 * 128 + 256) + 16 * 23 * 129
    assert L.vcnf_made_sample_pack_elems(0, 8, 1, 2) == 0


def _call(L, sfx, x=FAKE, y=FAKE, ld=FAKE, add=None, gate=None, w=FAKE, elems=None, tab=FAKE, b=4, d=6, h=32, nb=1, p=2, cfg=None,
          ld_mode=0, bad=None):
    if elems is None:
        elems = L.vcnf_made_sample_pack_elems(d, h, nb, p)
    return getattr(L, "vcnf_made_sample" + sfx)(x, y, ld, add, gate, w, elems, tab, b, d, h, nb, p, cfg, ld_mode, 1.0, bad, None)


@pytest.mark.parametrize("sfx", ["_f32", "_f64"])
def test_validation_status_codes(sfx):
    L = nf.lib()
    cfg = _lib.make_cfg(8, "linear", tail_bound=3.0)
    cfg = cfg.f64 if sfx == "_f64" else cfg
    assert _call(L, sfx, b=0) == 0                                      # empty batch: no launch
    assert _call(L, sfx, b=0, p=23, cfg=cfg) == 0
    assert _call(L, sfx, b=-1) == 2 and _call(L, sfx, d=0) == 2 and _call(L, sfx, h=1 << 20, elems=1) == 2
    assert _call(L, sfx, elems=5) == 2                                  # wpack of another shape
    assert _call(L, sfx, p=23) == 2 and _call(L, sfx, p=2, cfg=cfg) == 2 and _call(L, sfx, p=24, cfg=cfg) == 2
    assert _call(L, sfx, ld_mode=2) == 5
    for arg in ("x", "y", "ld", "w", "tab"):
        assert _call(L, sfx, **{arg: None}) == 1, arg
        assert _call(L, sfx, **{arg: ODD}) == 3, arg
    assert _call(L, sfx, gate=FAKE) == 1 and _call(L, sfx, add=FAKE) == 1            # one context operand without the other
    assert _call(L, sfx, add=FAKE, nb=0, b=0) == 0
    bad_cfg = _lib.make_cfg(8, "linear", tail_bound=3.0, min_bin_width=0.2)
    assert _call(L, sfx, p=23, cfg=bad_cfg.f64 if sfx == "_f64" else bad_cfg) == 4   # min_bin_width * K > 1
    twelve = _lib.make_cfg(12, "linear", tail_bound=3.0)
    assert _call(L, sfx, p=35, cfg=twelve.f64 if sfx == "_f64" else twelve, b=0) == 5                # no instance for 12 bins


def test_layers_carry_the_switch_and_cpu_tensors_keep_the_loop():
    for kind in ("affine", "spline"):
        lay = R.make_layer(kind, "uneven", seed=2)
        assert lay.fuse_sampling is True and callable(lay.inverse_into)
        x, _ = R.inputs_for(lay, 5)
        assert made_sample.plan(lay, x, None, R.dims(lay)[3]) is None              # a CPU tensor
        with torch.no_grad(), pytest.raises(nf.VcnfError):                         # ... and the loop's kernels have no CPU path
            lay.inverse(x)
    assert callable(nf.flows.AutoregressiveRationalQuadraticSpline(6, 1, 32).forward_into)
