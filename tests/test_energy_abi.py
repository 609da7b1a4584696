"""The energy densities without a GPU, the C side: the five families' enum values, and the documented status codes of
all eleven entry points that take a family - vcnf_target_log_prob_*, vcnf_hmc_stack[_bwd]_*,
vcnf_hmc_annealed_stack[_bwd]_*, vcnf_mh_walk_* - with pointers that are never dereferenced, including the table lengths
the families read; the table check the _lib wrappers share."""
import ctypes

import pytest
import torch

import vcnf_amd as nf
from vcnf_amd import _lib

FAKE = ctypes.c_void_p(0x1000)         # never dereferenced: validation fails first / batch == 0
ODD = ctypes.c_void_p(0x1002)          # not aligned to a float or a double
# family -> entries of the table it reads (0: table and n_comp are ignored)
TABLE = {16: 1, 17: 1, 18: 4, 19: 4, 20: 0}

TARGET_PTRS = ("z", "table", "logp", "score")
HMC_PTRS = ("z", "noise", "unif", "step", "mass", "sqrt_mass", "table", "z_out", "log_det", "trace", "accept")
HMC_BWD_PTRS = ("trace", "accept", "noise", "step", "mass", "sqrt_mass", "table", "g_out", "g_logdet", "g_in", "g_step", "g_mass",
                "g_sqrt_mass", "workspace")
ANN_PTRS = ("z", "noise", "unif", "step", "mass", "sqrt_mass", "beta", "prior_loc", "prior_log_scale", "table", "z_out",
            "log_det", "logp_target", "trace", "accept")
ANN_BWD_PTRS = ("trace", "accept", "noise", "step", "mass", "sqrt_mass", "beta", "prior_loc", "prior_log_scale", "table", "g_out",
                "g_logdet", "g_in", "g_step", "g_mass", "g_sqrt_mass", "workspace")
MH_PTRS = ("z", "eps", "w", "prop_scale", "table", "z_out", "accept")
# (entry point, pointers, integer arguments between the pointers and n_comp, a required output)
ENTRIES = (("vcnf_target_log_prob", TARGET_PTRS, (4,), "logp"),
           ("vcnf_hmc_stack", HMC_PTRS, (4, 2, 3), "z_out"),
           ("vcnf_hmc_stack_bwd", HMC_BWD_PTRS, (4, 2, 3, 1), "g_in"),
           ("vcnf_hmc_annealed_stack", ANN_PTRS, (4, 2, 3), "z_out"),
           ("vcnf_hmc_annealed_stack_bwd", ANN_BWD_PTRS, (4, 2, 3, 1), "g_in"),
           ("vcnf_mh_walk", MH_PTRS, (4, 3), "z_out"))
OPTIONAL = {"score", "trace", "accept", "g_out", "g_logdet", "logp_target"}


def test_enum_values():
    assert (_lib.TARGET_TWO_MODES, _lib.TARGET_SINUSOIDAL, _lib.TARGET_SINUSOIDAL_GAP, _lib.TARGET_SINUSOIDAL_SPLIT,
            _lib.TARGET_SMILEY) == (16, 17, 18, 19, 20)
    assert (_lib.TARGET_TWO_MOONS, _lib.TARGET_CIRCULAR_GMM, _lib.TARGET_RING_MIXTURE) == (0, 1, 2)
    D = nf.distributions
    assert [c._family for c in (D.TwoModes, D.Sinusoidal, D.Sinusoidal_gap, D.Sinusoidal_split, D.Smiley)] == [16, 17, 18, 19, 20]


def _call(L, name, ptrs, ints, sfx, family, n=4, b=None, **given):
    ints = ((ints[0] if b is None else b),) + tuple(ints[1:])
    return getattr(L, name + sfx)(*[given.get(p, FAKE) for p in ptrs], *ints, n, family, 0.5, None)


@pytest.mark.parametrize("sfx", ["_f32", "_f64"])
@pytest.mark.parametrize("entry", ENTRIES, ids=[e[0] for e in ENTRIES])
def test_validation_status_codes(entry, sfx):
    name, ptrs, ints, required = entry
    L = nf.lib()
    assert len(ENTRIES) * 2 - 1 == 11                    # vcnf_target_log_prob has no backward of its own
    optional = OPTIONAL - ({"trace", "accept"} if name.endswith("_bwd") else set())
    for family, entries in TABLE.items():
        call = lambda **kw: _call(L, name, ptrs, ints, sfx, family, **kw)
        for p in ptrs:
            if p == "table" and not entries:             # Smiley ignores table and n_comp, like TwoMoons
                assert call(table=None, n=-1, **{required: None}) == 1
                assert call(table=None, n=0, **{required: ODD}) == 3
                assert call(table=None, n=-1, b=0) == 0
                continue
            if p not in optional:
                assert call(**{p: None}) == 1, p         # NULL required pointer
            if p != "accept":                            # bytes
                assert call(**{p: ODD}) == 3, p          # misaligned buffer
        assert call(b=-1) == 2
        assert call(b=0) == 0 and call(b=0, **{p: None for p in ptrs}) == 0        # empty batch: no launch
        if entries:
            # a table shorter than the family reads is a shape error, before any pointer is looked at
            for n in (entries - 1, 0, -5):
                assert call(n=n) == 2 and call(n=n, b=0) == 2 and call(n=n, table=None) == 2, (family, n)
            assert call(n=entries, z=None, trace=None) == 1 and call(n=1 << 30, b=0) == 0
            assert call(table=None) == 1
    for family in (3, 15, 21, -1, 1 << 20):
        assert _call(L, name, ptrs, ints, sfx, family) == 5 and _call(L, name, ptrs, ints, sfx, family, b=0) == 5
    # the order of the checks: batch, then the family, then n_comp
    assert _call(L, name, ptrs, ints, sfx, 3, b=-1) == 2 and _call(L, name, ptrs, ints, sfx, 3, n=0) == 5


def test_wrappers_check_the_constant_table():
    """_lib's table check, shared by target_log_prob and the stochastic wrappers: the constants' number, dtype and device."""
    z = torch.zeros(3, 2)
    check = lambda family, table: _lib._target_table("test", z, z.device, family, table)
    need = {_lib.TARGET_TWO_MODES: 1, _lib.TARGET_SINUSOIDAL: 1, _lib.TARGET_SINUSOIDAL_GAP: 4, _lib.TARGET_SINUSOIDAL_SPLIT: 4}
    for family, n in need.items():
        for table in (None, torch.zeros(n - 1), torch.zeros(n, dtype=torch.float64), torch.zeros(n, device="meta")):
            with pytest.raises(nf.VcnfError, match="constant table"):
                check(family, table)
        table, n_comp = check(family, torch.ones(n, requires_grad=True))
        assert n_comp == n and not table.requires_grad and table.is_contiguous()
        assert check(family, torch.ones(n + 2))[1] == n + 2                  # longer is the entry point's to ignore
    assert check(_lib.TARGET_SMILEY, torch.ones(3)) == (None, 0) and check(_lib.TARGET_TWO_MOONS, None) == (None, 0)
    with pytest.raises(nf.VcnfError, match="component table"):
        check(_lib.TARGET_RING_MIXTURE, None)
    assert check(_lib.TARGET_CIRCULAR_GMM, torch.ones(3, 2))[1] == 3
