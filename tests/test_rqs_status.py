"""Status codes of the spline entry points for invalid configurations and sizes, one fault and two faults at a time
(two faults pin the order of the checks).  No GPU needed: every call either fails validation or has an empty batch, so
nothing is launched; the pointers are never dereferenced.

Every case is called with an empty batch (n = 0; n = -1 for the cases with a size fault), so a configuration that
wrongly passes validation shows as status 0 and never as a launch on these pointers.  The spline units check the
configuration before they return for an empty batch; the fused entry points test the bin minima behind that return,
so those two cases are 0 there.

EXPECTED was recorded, called in this way, from the library built at the commit before the entry points' validation
moved to csrc/rqs_host.hpp (rqs_check_cfg).  The literals are that build's answers, and the test passes on that build
as it does on the present one: the move kept every status."""
import ctypes

import pytest

import vcnf_amd
from vcnf_amd import _lib

FAKE = ctypes.c_void_p(0x1000)        # 16-byte aligned, never dereferenced

# (name, changes to the base configuration - None: cfg is NULL, size fault).  The base configuration is valid for
# the entry point: 8 bins, linear tails with bound 3 (no tails for the tensor-limit entry points), default minima.
CASES = (
    ("cfg NULL", None, False),
    ("0 bins", dict(num_bins=0), False),
    ("65 bins", dict(num_bins=65), False),
    ("1025 bins", dict(num_bins=1025), False),
    ("linear tails, 1 bin", dict(num_bins=1, tails=1), False),
    ("tails -1", dict(tails=-1), False),
    ("tails 3", dict(tails=3), False),
    ("min_bin_width * K > 1", dict(min_bin_width=0.2), False),
    ("min_bin_height * K > 1", dict(min_bin_height=0.2), False),
    ("n = -1", dict(), True),
    ("cfg NULL, n = -1", None, True),
    ("n = -1, tails 3", dict(tails=3), True),
    ("n = -1, min_bin_width * K > 1", dict(min_bin_width=0.2), True),
    ("65 bins, tails 3", dict(num_bins=65, tails=3), False),
    ("linear tails, 1 bin, min_bin_width * K > 1", dict(num_bins=1, tails=1, min_bin_width=1.5), False),
)


def _cfg(no_tails, changes, f64):
    if changes is None:
        return None
    cfg = _lib.make_cfg(8, None if no_tails else "linear", tail_bound=3.0)
    for c in (cfg, cfg.f64):
        for k, v in changes.items():
            setattr(c, k, v)
    return ctypes.byref(cfg.f64 if f64 else cfg)


def _bcast():
    return ctypes.byref(_lib.RqsLimitBcast((ctypes.c_int64 * 4)(1, 1, 1, 1), (ctypes.c_int64 * 4)(1, 1, 1, 1)))


def _elementwise(sfx):
    return lambda L, c, n: getattr(L, "vcnf_rqs_elementwise" + sfx)(FAKE, FAKE, FAKE, FAKE, 8, 8, 7, FAKE, FAKE, n, c, 0,
                                                                   None, None)


def _strided(sfx):
    return lambda L, c, n: getattr(L, "vcnf_rqs_elementwise_strided" + sfx)(FAKE, FAKE, FAKE, FAKE, 8, 8, 7, 1, 1, 0, FAKE,
                                                                           FAKE, n, c, 0, None, None)


def _limits(sfx):
    return lambda L, c, n: getattr(L, "vcnf_rqs_elementwise_limits" + sfx)(FAKE, FAKE, FAKE, FAKE, 8, 8, 9, FAKE, FAKE, FAKE,
                                                                          FAKE, _bcast(), FAKE, FAKE, n, c, 0, None, None)


def _bwd(sfx):
    return lambda L, c, n: getattr(L, "vcnf_rqs_elementwise_bwd" + sfx)(FAKE, FAKE, FAKE, FAKE, 8, 8, 7, FAKE, FAKE, FAKE,
                                                                       FAKE, FAKE, FAKE, n, c, 0, None)


def _limits_bwd(sfx):
    return lambda L, c, n: getattr(L, "vcnf_rqs_elementwise_limits_bwd" + sfx)(
        FAKE, FAKE, FAKE, FAKE, 8, 8, 9, FAKE, FAKE, FAKE, FAKE, _bcast(), FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE,
        FAKE, FAKE, n, c, 0, None)


def _packed_bwd(sfx):
    return lambda L, c, n: getattr(L, "vcnf_rqs_packed_bwd" + sfx)(FAKE, FAKE, 1, 1, FAKE, FAKE, FAKE, FAKE, n, c, 0, None)


def _layer_fused(L, c, n):
    floats = L.vcnf_rqs_layer_fused_pack_floats(32, 32, 16, 2)
    return L.vcnf_rqs_layer_fused_f32(FAKE, FAKE, FAKE, FAKE, n, FAKE, 32, FAKE, 32, 16, 128, 2, 0, FAKE, floats, None, None,
                                      None, c, 0, 0, 1.0, None, None, None, None)


def _stack_fused(L, c, n):
    floats = L.vcnf_rqs_layer_fused_pack_floats(32, 32, 16, 2)
    layers = (_lib.RqsStackLayer * 1)(_lib.RqsStackLayer(0x1000, 0x1000, 0x1000, None, None, None))
    return L.vcnf_rqs_stack_fused_f32(FAKE, FAKE, FAKE, FAKE, n, layers, 1, 32, 32, 16, 128, 2, 0, floats, c, 0, 0, 1.0, None,
                                      None, None, None)


def _final_fused(name):
    def call(L, c, n):
        floats = L.vcnf_rqs_final_fused_pack_floats(512, 128, 8)
        return getattr(L, name)(FAKE, FAKE, FAKE, FAKE, n, 1024, FAKE, 512, 128, FAKE, floats, c, 0, None, None)
    return call


# entry point -> (call(L, cfg, n), no tails in the base configuration, fp64 configuration)
ENTRY = {
    "vcnf_rqs_coupling_f32": (lambda L, c, n: L.vcnf_rqs_coupling_f32(
        FAKE, FAKE, FAKE, 1, FAKE, 1, None, None, None, FAKE, FAKE, n, c, 0, 0, 1.0, None, None), False, False),
    "vcnf_rqs_elementwise_f32": (_elementwise("_f32"), False, False),
    "vcnf_rqs_elementwise_limits_f32": (_limits("_f32"), True, False),
    "vcnf_rqs_elementwise_strided_f32": (_strided("_f32"), False, False),
    "vcnf_rqs_shared_f32": (lambda L, c, n: L.vcnf_rqs_shared_f32(
        FAKE, FAKE, FAKE, FAKE, 4, FAKE, FAKE, FAKE, n, c, 0, None, None), False, False),
    "vcnf_rqs_identity_half_f32": (lambda L, c, n: L.vcnf_rqs_identity_half_f32(
        FAKE, FAKE, FAKE, FAKE, n, 8, FAKE, 4, FAKE, FAKE, FAKE, c, 0, 0, None, None), False, False),
    "vcnf_rqs_conditioner_input_f32": (lambda L, c, n: L.vcnf_rqs_conditioner_input_f32(
        FAKE, n, 8, FAKE, 4, None, 0, None, None, None, c, 0, FAKE, None), False, False),
    "vcnf_rqs_elementwise_bwd_f32": (_bwd("_f32"), False, False),
    "vcnf_rqs_elementwise_limits_bwd_f32": (_limits_bwd("_f32"), True, False),
    "vcnf_rqs_packed_bwd_f32": (_packed_bwd("_f32"), False, False),
    "vcnf_rqs_shared_bwd_f32": (lambda L, c, n: L.vcnf_rqs_shared_bwd_f32(
        FAKE, FAKE, FAKE, FAKE, n, 4, 1, FAKE, FAKE, FAKE, FAKE, L.vcnf_rqs_shared_bwd_groups(n, 4), c, 0, None), False, False),
    "vcnf_rqs_elementwise_f64": (_elementwise("_f64"), False, True),
    "vcnf_rqs_elementwise_strided_f64": (_strided("_f64"), False, True),
    "vcnf_rqs_elementwise_bwd_f64": (_bwd("_f64"), False, True),
    "vcnf_rqs_elementwise_limits_f64": (_limits("_f64"), True, True),
    "vcnf_rqs_elementwise_limits_bwd_f64": (_limits_bwd("_f64"), True, True),
    "vcnf_rqs_packed_bwd_f64": (_packed_bwd("_f64"), False, True),
    "vcnf_rqs_layer_fused_f32": (_layer_fused, False, False),
    "vcnf_rqs_stack_fused_f32": (_stack_fused, False, False),
    "vcnf_rqs_final_fused_f32": (_final_fused("vcnf_rqs_final_fused_f32"), False, False),
    "vcnf_rqs_final_fused_presplit_f32": (_final_fused("vcnf_rqs_final_fused_presplit_f32"), False, False),
}

# one status per case, in the order of CASES; 0: the case reaches the return for an empty batch
EXPECTED = {
    "vcnf_rqs_coupling_f32": (1, 2, 0, 2, 2, 5, 5, 4, 4, 2, 1, 5, 4, 5, 2),
    "vcnf_rqs_elementwise_f32": (1, 2, 0, 2, 2, 5, 5, 4, 4, 2, 1, 5, 4, 5, 2),
    "vcnf_rqs_elementwise_limits_f32": (1, 2, 2, 2, 5, 5, 5, 4, 4, 2, 1, 5, 4, 2, 5),
    "vcnf_rqs_elementwise_strided_f32": (1, 2, 0, 2, 2, 5, 5, 4, 4, 2, 1, 5, 4, 5, 2),
    "vcnf_rqs_shared_f32": (1, 2, 0, 2, 2, 5, 5, 4, 4, 2, 1, 5, 4, 5, 2),
    "vcnf_rqs_identity_half_f32": (1, 2, 5, 2, 2, 5, 5, 4, 4, 2, 1, 5, 4, 5, 2),
    "vcnf_rqs_conditioner_input_f32": (1, 2, 0, 2, 2, 5, 5, 4, 4, 2, 1, 5, 4, 5, 2),
    "vcnf_rqs_elementwise_bwd_f32": (1, 2, 2, 2, 2, 5, 5, 4, 4, 2, 1, 5, 4, 2, 2),
    "vcnf_rqs_elementwise_limits_bwd_f32": (1, 2, 2, 2, 5, 5, 5, 4, 4, 2, 1, 5, 4, 2, 5),
    "vcnf_rqs_packed_bwd_f32": (1, 2, 2, 2, 2, 5, 5, 4, 4, 2, 1, 5, 4, 2, 2),
    "vcnf_rqs_shared_bwd_f32": (1, 2, 2, 2, 2, 5, 5, 4, 4, 2, 1, 5, 4, 2, 2),
    "vcnf_rqs_elementwise_f64": (1, 2, 2, 2, 0, 5, 5, 4, 4, 2, 1, 2, 2, 2, 4),
    "vcnf_rqs_elementwise_strided_f64": (1, 2, 2, 2, 0, 5, 5, 4, 4, 2, 1, 2, 2, 2, 4),
    "vcnf_rqs_elementwise_bwd_f64": (1, 2, 2, 2, 2, 5, 5, 4, 4, 2, 1, 5, 4, 2, 2),
    "vcnf_rqs_elementwise_limits_f64": (1, 2, 2, 2, 5, 5, 5, 4, 4, 2, 1, 5, 4, 2, 5),
    "vcnf_rqs_elementwise_limits_bwd_f64": (1, 2, 2, 2, 5, 5, 5, 4, 4, 2, 1, 5, 4, 2, 5),
    "vcnf_rqs_packed_bwd_f64": (1, 2, 2, 2, 2, 5, 5, 4, 4, 2, 1, 5, 4, 2, 2),
    "vcnf_rqs_layer_fused_f32": (1, 5, 5, 5, 5, 5, 5, 0, 0, 2, 1, 5, 2, 5, 5),
    "vcnf_rqs_stack_fused_f32": (1, 5, 5, 5, 5, 5, 5, 0, 0, 2, 1, 5, 2, 5, 5),
    "vcnf_rqs_final_fused_f32": (1, 5, 5, 5, 5, 5, 5, 0, 0, 2, 1, 5, 2, 5, 5),
    "vcnf_rqs_final_fused_presplit_f32": (1, 5, 5, 5, 5, 5, 5, 0, 0, 2, 1, 5, 2, 5, 5),
}


def status(L, entry, case, n):
    call, no_tails, f64 = ENTRY[entry]
    return call(L, _cfg(no_tails, case[1], f64), n)


def test_the_table_is_complete():
    assert len(ENTRY) == 21 and sorted(EXPECTED) == sorted(ENTRY)
    assert all(len(row) == len(CASES) for row in EXPECTED.values())
    assert all(name in _lib.PROTOTYPES for name in ENTRY)


@pytest.mark.parametrize("entry", sorted(ENTRY))
def test_status_codes(entry):
    L = vcnf_amd.lib()
    for case, want in zip(CASES, EXPECTED[entry]):
        assert not (case[2] and want == 0), "a negative size cannot pass"
        assert status(L, entry, case, -1 if case[2] else 0) == want, (entry, case[0])
