"""Layers for circular coordinates (normflow 1.2 flows/periodic.py): ``PeriodicWrap`` brings the columns ``ind`` of the
last axis back into [-bound, bound), ``PeriodicShift`` moves them by ``shift`` modulo the period first.  Both have
derivative 1 and log-det 0.

On the device a direction is one launch of vcnf_periodic_* (csrc/periodic.hip) over the whole tensor, with the bits of
the reference's ``torch.remainder`` composition, and under autograd one node whose backward hands the gradient on
without a launch.  The kernel reads two per-column tables - the bound of a wrapped column, 0 elsewhere, and the shift -
which are derived buffers (``derived.memo``) keyed by the number of columns, device, dtype and what ``ind``, ``bound``
and ``shift`` are.  ``PeriodicWrap.forward`` is the identity and launches no kernel; the zero log-det of the plain
``(z, log_det)`` contract is torch's, and ``forward_into`` / ``inverse_into`` (what NormalizingFlow calls) skip it.

The reference's composition itself, differentiable in z, serves what the kernel does not: CPU tensors, half precision,
non-contiguous inputs, a bound that is not positive, and - raising torch's own error - an index out of range, a
``bound`` / ``shift`` shaped neither as a scalar nor as [len(ind)], or one per index of a wider dtype than z (torch
computes in that dtype and refuses to store the result).  For a device tensor the index range is checked on the host
first and the IndexError raised there: torch's own check of a device index is an assertion inside its kernel."""
import torch

from .base import Flow
from .. import _lib, autograd
from ..derived import memo, tensor_key


def _key_of(value):
    """What ``value`` is, for a memo key: identity and version of a tensor, the value of anything else."""
    if torch.is_tensor(value):
        return tensor_key((value,))
    return tuple(value) if isinstance(value, (list, tuple)) else value


def _column_table(value, idx, d, dtype):
    """[d] CPU table with ``value`` (a scalar or one per index) at the columns ``idx`` and 0 elsewhere; None for any
    other shape.  A Python number is rounded from fp64 once, as torch rounds a scalar operand."""
    t = value.detach().cpu() if torch.is_tensor(value) else torch.tensor(value, dtype=torch.float64)
    if t.dim() == 0:
        t = t.expand(len(idx))
    elif tuple(t.shape) != (len(idx),):
        return None
    table = torch.zeros(d, dtype=dtype)
    table[idx] = t.to(dtype)
    return table


class _PeriodicMap(Flow):
    """Shared end of PeriodicWrap and PeriodicShift: z[..., ind] -> remainder(z[..., ind] + sign shift + bound, 2 bound)
    - bound."""

    def _keep(self, name, value, dtype=None):
        """A tensor argument is a buffer (state dict), anything else a plain attribute: as the reference has it."""
        if torch.is_tensor(value):
            self.register_buffer(name, value if dtype is None else value.to(dtype))
        else:
            setattr(self, name, value)

    def _operands(self):
        return self.ind, self.bound, getattr(self, 'shift', None)

    def _index(self, d):
        """The columns among ``d`` as a CPU int64 vector, negative indices normalised (memoised).  An index outside
        [-d, d) raises IndexError here, on the host: torch's indexing raises it for CPU tensors, but on the device its
        kernel asserts, which takes the process's GPU context down with it."""
        ind = self.ind

        def build(owner):
            idx = (ind.detach().cpu().to(torch.long) if torch.is_tensor(ind) else torch.tensor(ind, dtype=torch.long)).reshape(-1)
            bad = idx[(idx < -d) | (idx >= d)]
            if len(bad):
                raise IndexError("index %d is out of bounds for the last dimension with size %d" % (int(bad[0]), d))
            return idx % d if d else idx
        return memo(self, 'periodic_index', (d, _key_of(ind)), build, 8)

    def _build_tables(self, d, device, dtype):
        """(half, shift) [d] on the device - shift None for a layer without one - or (None, None) where the kernel
        does not serve the arguments."""
        _, bound, shift = self._operands()
        idx = self._index(d)
        half = _column_table(bound, idx, d, dtype)
        if half is None or not bool((half[idx] > 0).all()):
            return None, None
        if shift is None:
            return half.to(device), None
        table = _column_table(shift, idx, d, dtype)
        if table is None:
            return None, None
        return half.to(device), table.to(device)

    def _tables(self, z):
        ind, bound, shift = self._operands()
        for t in (bound, shift):            # a [len(ind)] tensor of a wider dtype makes the reference compute in that dtype
            if torch.is_tensor(t) and t.dim() > 0 and torch.promote_types(t.dtype, z.dtype) != z.dtype:
                return None, None
        d, device, dtype = z.shape[-1], z.device, z.dtype
        key = (d, device, dtype, _key_of(ind), _key_of(bound), _key_of(shift))
        return memo(self, 'periodic_tables', key, lambda owner: owner._build_tables(d, device, dtype), 8)

    def _torch(self, z, sign):
        """The reference's composition."""
        ind, bound, shift = self._operands()
        z_ = z.clone()
        a = z_[..., ind]
        if shift is not None:
            a = a + shift if sign > 0 else a - shift
        z_[..., ind] = torch.remainder(a + bound, 2 * bound) - bound
        return z_

    def _run(self, z, sign):
        half = None
        if z.is_cuda and z.dim() >= 1:
            self._index(z.shape[-1])
        if z.is_cuda and z.dtype in (torch.float32, torch.float64) and z.dim() >= 1 and z.shape[-1] >= 1 and z.is_contiguous():
            half, shift = self._tables(z)
        if half is None:
            return self._torch(z, sign)
        if autograd.needs_grad(z):
            return autograd.PeriodicFn.apply(z, half, shift, sign)
        return _lib.periodic(z, half, shift, sign)

    @staticmethod
    def _no_log_det(z):
        return torch.zeros(len(z), dtype=z.dtype, device=z.device)


class PeriodicWrap(_PeriodicMap):
    """The last layer of a flow on circular coordinates: sampling leaves z alone, the density direction maps the
    columns ``ind`` (an int, a list or a tensor of indices into the last axis) into [-bound, bound).  ``bound``: a number
    or a tensor, scalar or one per index.  Tensor arguments are buffers ``ind`` (int64) / ``bound``."""

    def __init__(self, ind, bound=1.0):
        super().__init__()
        self._keep('ind', ind, torch.long)
        self._keep('bound', bound)

    def forward(self, z):
        return z, self._no_log_det(z)

    def inverse(self, z):
        return self._run(z, 1.0), self._no_log_det(z)

    # the forms NormalizingFlow calls: the log-det is zero, log_q stays as it is
    def forward_into(self, z, log_q):
        return z

    def inverse_into(self, z, log_q):
        return self._run(z, 1.0)


class PeriodicShift(_PeriodicMap):
    """Shift of the circular columns ``ind`` by ``shift`` modulo the period 2 ``bound`` (sampling direction; the density
    direction shifts back), so that consecutive circular couplings do not share their fixed point.  ``bound`` and
    ``shift``: numbers or tensors, scalar or one per index; tensor arguments are buffers ``ind`` (int64) / ``bound`` /
    ``shift``."""

    def __init__(self, ind, bound=1.0, shift=0.0):
        super().__init__()
        self._keep('ind', ind, torch.long)
        self._keep('bound', bound)
        self._keep('shift', shift)

    def forward(self, z):
        return self._run(z, 1.0), self._no_log_det(z)

    def inverse(self, z):
        return self._run(z, -1.0), self._no_log_det(z)

    def forward_into(self, z, log_q):
        return self._run(z, 1.0)

    def inverse_into(self, z, log_q):
        return self._run(z, -1.0)
