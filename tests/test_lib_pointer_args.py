"""The pointer argument type of the binding without a GPU: an entry point called with tensors receives their own
addresses, None is NULL, and a plain int address or a ``c_void_p`` is the same pointer.  Shown through the host-side
validation of ``vcnf_tail_log_prob_f32`` (NULL check, then the alignment of every buffer, before anything is
launched): the CPU tensors used here are never dereferenced.  A spline entry point takes its ``vcnf_rqs_cfg`` as the
struct itself."""
import ctypes

import torch

import vcnf_amd as nf
from vcnf_amd import _lib

NULL, ALIGN, BAD_CFG = 1, 3, 4          # VCNF_ERR_NULL, VCNF_ERR_ALIGN, the spline's min_bin_width * K > 1
B, D = 4, 8


def _operands():
    """z [B, D], the rows loc / log_scale / shape / cst [D], logp [B]: aligned fp32 host tensors."""
    return [torch.zeros(B, D)] + [torch.zeros(D) for _ in range(4)] + [torch.zeros(B)]


def _log_prob(pointers):
    return nf.lib().vcnf_tail_log_prob_f32(*pointers, B, D, _lib.TAIL_STUDENT_T, _lib.LD_STORE, 1.0, None)


def _odd(t):
    """The bytes of ``t`` from its second byte on: a tensor whose address is odd."""
    view = t.reshape(-1).view(torch.uint8)[1:]
    assert view.data_ptr() == t.data_ptr() + 1 and view.data_ptr() % 2 == 1
    return view


def test_tensors_pass_as_pointers_and_none_as_null():
    assert all(t.data_ptr() % 4 == 0 for t in _operands())
    for missing in range(6):            # every pointer of this entry point is required
        ops = _operands()
        ops[missing] = None
        assert _log_prob(ops) == NULL, missing


def test_the_tensors_own_address_arrives():
    for moved in range(6):
        ops = _operands()
        keep = ops[moved]               # the storage the odd view points into
        ops[moved] = _odd(keep)
        assert _log_prob(ops) == ALIGN, moved


def test_int_and_c_void_p_are_the_same_pointer():
    ops = _operands()
    odd = _odd(ops[1])
    for as_pointer in (odd, ctypes.c_void_p(odd.data_ptr()), odd.data_ptr()):
        assert _log_prob([ops[0], as_pointer] + ops[2:]) == ALIGN, type(as_pointer)


def test_cfg_struct_passes_without_byref():
    bad = _lib.make_cfg(8, "linear", min_bin_width=0.2)
    x, y, lad = torch.zeros(4), torch.zeros(4), torch.zeros(4)
    uw, uh, ud = torch.zeros(4, 8), torch.zeros(4, 8), torch.zeros(4, 7)
    L = nf.lib()
    assert L.vcnf_rqs_elementwise_f32(x, uw, uh, ud, 8, 8, 7, y, lad, 4, bad, 0, None, None) == BAD_CFG
    assert L.vcnf_rqs_elementwise_f64(x, uw, uh, ud, 8, 8, 7, y, lad, 4, bad.f64, 0, None, None) == BAD_CFG
    assert L.vcnf_rqs_elementwise_f32(x, uw, uh, ud, 8, 8, 7, y, lad, 4, ctypes.byref(bad), 0, None, None) == BAD_CFG
