"""ctypes binding of ``libvcnf_hip.so`` (the C ABI declared in include/vcnf_hip.h)
and thin tensor-level wrappers around each entry point.

There is no CPU implementation behind these wrappers: a CPU tensor, a missing
library or a non-zero status raises.  PyTorch is used for device memory and the
current HIP stream only.

How a wrapper calls the library (copy this for a new entry point):

* pointer arguments are declared ``_P`` in ``PROTOTYPES`` (read from the header) and the wrapper passes the tensor itself (or
  None for NULL); a ``vcnf_rqs_cfg`` argument is declared ``_CFG`` and the wrapper passes the struct (``_cfg_of``
  picks the fp64 twin) - ctypes converts both during the call;
* ``_call(name, dev, *args)`` enters the tensors' device, appends the current stream as the last argument, calls the
  entry point ``name`` and raises on a non-zero status, naming ``name``; ``tag=`` brackets the launch for bench.py;
* ``_ld_out`` gives the log-det / log-prob output and its ``LD_STORE | LD_ACCUM`` mode, ``_bad_if`` the inverse
  spline's discriminant counter.
"""
import ctypes
import math
import os

import torch

from . import _abi, build as _build


class _P:
    """``void*`` argument that takes the tensor itself.  ctypes calls ``from_param`` on each argument during the call:
    a tensor becomes its ``data_ptr()``, None is NULL, and a plain int address, a ``c_void_p`` or a ctypes array pass
    as they do for ``c_void_p``.  (A static method with its two globals bound as defaults: this runs once per pointer
    of every launch, and a classmethod on a ``c_void_p`` subclass cost 1.3 us more per 26-argument call.)"""

    @staticmethod
    def from_param(value, _as_void_p=ctypes.c_void_p.from_param, _tensor=torch.Tensor):
        return _as_void_p(value.data_ptr() if isinstance(value, _tensor) else value)


_ABI = _abi.read(_build.HEADER, pointer=_P)

# every VCNF_* constant of the header under its name without the prefix: OK, ERR_*, LD_*, TAILS_*, PREC_*, SCALE_*, TAIL_*,
# MVN_* (MVN_MAX_DIM among them), GMM_MAX_TABLE, PLANAR_TANH / PLANAR_LEAKY / RADIAL, TARGET_*, HMC_BLOCK,
# HMC_MAX_BWD_GROUPS, STOCH_MAX_POINTS, VAE_MAX_SAMPLES, AFFINE_STACK_MAX_LAYERS, PROBE_*
globals().update({name[len("VCNF_"):]: value for name, value in _ABI.constants.items()})
SCALE_MAPS = {"exp": SCALE_EXP, "sigmoid": SCALE_SIGMOID, "sigmoid_inv": SCALE_SIGMOID_INV}


def scale_code(scale, scale_map):
    """Kernel code of an affine coupling's ``scale`` / ``scale_map`` settings."""
    if not scale:
        return SCALE_NONE
    if scale_map not in SCALE_MAPS:
        raise NotImplementedError('This scale map is not implemented.')
    return SCALE_MAPS[scale_map]


RqsCfg, RqsCfg64 = _ABI.structs["vcnf_rqs_cfg"], _ABI.structs["vcnf_rqs_cfg_f64"]
RqsLimitBcast = _ABI.structs["vcnf_rqs_limit_bcast"]       # limit j of element i is lim_j[(i // inner[j]) % period[j]]
RqsStackLayer, AffineStackLayer = _ABI.structs["vcnf_rqs_stack_layer"], _ABI.structs["vcnf_affine_stack_layer"]
_CFG, _CFG64 = ctypes.POINTER(RqsCfg), ctypes.POINTER(RqsCfg64)
_I64 = ctypes.c_int64

# name -> (argtypes, restype): the prototypes of include/vcnf_hip.h, as vcnf_amd/_abi.py reads them
PROTOTYPES = _ABI.functions

_LIB = None


class VcnfError(RuntimeError):
    pass


def lib_path():
    """The in-tree library; VCNF_LIB selects another build of it (kernel variants of a measurement, profiles/tools)."""
    return os.environ.get("VCNF_LIB") or _build.LIB


def lib():
    """Load (once) and return the ctypes handle.  Raises if the library was not
    built - there is no fallback path."""
    global _LIB
    if _LIB is not None:
        return _LIB
    path = lib_path()
    if not os.path.exists(path):
        raise VcnfError("HIP library %s is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                        "(or python -m vcnf_amd.build); vcnf_amd has no CPU fallback" % path)
    # torch ships its own libamdhip64 (soname libamdhip64.so.7); make sure that one is
    # the HIP runtime our library binds to, so streams and pointers are shared with torch.
    hip_rt = os.path.join(os.path.dirname(torch.__file__), "lib", "libamdhip64.so")
    if os.path.exists(hip_rt):
        ctypes.CDLL(hip_rt, mode=ctypes.RTLD_GLOBAL)
    handle = ctypes.CDLL(path)
    for name, (args, res) in PROTOTYPES.items():
        fn = getattr(handle, name)      # AttributeError if the ABI is incomplete
        fn.argtypes, fn.restype = args, res
    if handle.vcnf_abi_version() != 1:
        raise VcnfError("libvcnf_hip.so ABI version mismatch")
    _LIB = handle
    return handle


def _check(status, what):
    if status != OK:
        msg = lib().vcnf_status_string(status).decode()
        if status == 4:       # splines.py:104-107 raises ValueError
            raise ValueError(msg.capitalize())
        raise VcnfError("%s: %s (status %d)" % (what, msg, status))


def _stream():
    # raw handle of the current stream of the current device (torch.cuda.current_stream() builds a Stream object
    # and resolves the device through three layers of helpers: 8 us per call, several calls per layer)
    return ctypes.c_void_p(torch._C._cuda_getCurrentRawStream(torch.cuda.current_device()))


def _ptr(t):
    # what _P does with a tensor, for callers that bind entry points of their own (profiles/tools)
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def require_device(*tensors, allow_grad=False, f64=False):
    """Every tensor must be an fp32 tensor on one HIP device.  Autograd reaches the
    kernels only through vcnf_amd.autograd (the spline VJP kernel); a plain wrapper
    called with a tensor that requires grad raises rather than silently dropping it."""
    dev = None
    for t in tensors:
        if t is None:
            continue
        if not t.is_cuda:
            raise VcnfError("vcnf_amd computes on MI355X only (tensor on %s); there is no CPU path" % t.device)
        if t.is_floating_point() and t.dtype != torch.float32 and not (f64 and t.dtype == torch.float64):
            raise VcnfError("this vcnf_amd kernel is fp32%s (got %s)" % (" / fp64" if f64 else "", t.dtype))
        if dev is None:
            dev = t.device
        elif t.device != dev:
            raise VcnfError("tensors on different devices: %s vs %s" % (dev, t.device))
        if not allow_grad and torch.is_grad_enabled() and t.requires_grad:
            raise NotImplementedError(
                "vcnf_amd: this HIP kernel has no backward pass; evaluate under torch.no_grad() "
                "(differentiable: the RQS couplings via vcnf_amd.autograd, SURVEY 8f row 1)")
    return dev


def _sfx(t):
    """Entry-point suffix of a tensor's dtype: the elementwise kernels exist for fp32 and fp64."""
    return "_f64" if t.dtype == torch.float64 else "_f32"


def n_derivatives(cfg):
    """Derivative logits per element: K-1 (linear tails), K (circular), K+1 (no tails)."""
    k = cfg.num_bins
    return k - 1 if cfg.tails == TAILS_LINEAR else k if cfg.tails == TAILS_CIRCULAR else k + 1


def make_cfg(num_bins, tails, tail_bound=1.0, left=0.0, right=1.0, bottom=0.0, top=1.0,
             min_bin_width=1e-3, min_bin_height=1e-3, min_derivative=1e-3, wh_scale=1.0):
    if tails == "linear":
        left, right, bottom, top = -tail_bound, tail_bound, -tail_bound, tail_bound
        mode = TAILS_LINEAR
    elif tails == "circular":
        left, right, bottom, top = -tail_bound, tail_bound, -tail_bound, tail_bound
        mode = TAILS_CIRCULAR
    elif tails is None:
        mode = TAILS_NONE
    else:
        # per-feature tail lists: SURVEY 8f row 4, not built
        raise RuntimeError("{} tails are not implemented.".format(tails))
    cfg = RqsCfg(int(num_bins), mode, float(left), float(right), float(bottom), float(top),
                 float(min_bin_width), float(min_bin_height), float(min_derivative), float(wh_scale))
    # the same constants at full double precision for the fp64 spline (1e-3 is not a float)
    cfg.f64 = RqsCfg64(int(num_bins), mode, float(left), float(right), float(bottom), float(top),
                       float(min_bin_width), float(min_bin_height), float(min_derivative), float(wh_scale))
    return cfg


def _cfg_of(cfg, x):
    """The spline constants in the precision of the inputs ``x``."""
    return cfg.f64 if x.dtype == torch.float64 else cfg


_BAD = {}

# bench.py hook: when set to a list, the bracketed wrappers (``_timed``) put a pair of HIP events around their kernel
# launch and append (start, end, tag) to it; the RQS coupling wrappers give their batch size as the tag.
EVENT_SINK = None


def device_index(device):
    """Explicit index of a CUDA device: 'cuda' without an index means the CURRENT device (the counters below
    are kept per device; a rank whose current device is not 0 must not read device 0's)."""
    dev = torch.device(device)
    if dev.type != "cuda":
        raise VcnfError("vcnf_amd runs on HIP devices only (got %s)" % dev)
    return torch.cuda.current_device() if dev.index is None else dev.index


def _counter(table, device):
    key = device_index(device)
    if key not in table:
        table[key] = torch.zeros(1, dtype=torch.int32, device=torch.device("cuda", key))
    return table[key]


class _timed:
    """bench.py hook: with EVENT_SINK set to a list, brackets a kernel launch with HIP events on the launch stream
    (torch's current stream = the stream the kernel is enqueued on) and appends (start, end, tag)."""

    def __init__(self, tag):
        self.tag, self.sink = tag, EVENT_SINK

    def __enter__(self):
        if self.sink is not None:
            self.e0, self.e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            self.e0.record()
        return self

    def __exit__(self, *exc):
        if self.sink is not None:
            self.e1.record()
            self.sink.append((self.e0, self.e1, self.tag))
        return False


def _launch(name, *args):
    """Status of the entry point ``name`` enqueued on the current stream of the current device."""
    return getattr(lib(), name)(*args, _stream())


def _call(name, dev, *args, tag=None):
    """One checked launch: the entry point ``name`` with ``args`` and, as its last argument, the current stream of
    ``dev``; raises on a non-zero status.  ``tag``: bracket the launch for bench.py (``_timed``)."""
    with torch.cuda.device(dev):
        if tag is None:
            st = _launch(name, *args)
        else:
            with _timed(tag):
                st = _launch(name, *args)
    _check(st, name)


def bad_discriminant_counter(device):
    """Device int32 that the inverse spline kernels bump when b^2-4ac < 0 (the
    reference asserts on the host, splines.py:164)."""
    return _counter(_BAD, device)


def _bad_if(inverse, dev):
    """The ``bad_count`` argument of the spline entry points: only the inverse direction has a discriminant."""
    return bad_discriminant_counter(dev) if inverse else None


_SAT = {}


def saturation_counter(device):
    """Device int32 that the fp16 split-half fused layer kernel bumps (once per workgroup) when an input, a
    context value or a hidden activation was clamped at +-65504."""
    return _counter(_SAT, device)


_REDO = {}


def range_redo_counter(device):
    """Device int32: tiles (128 samples) of fused RQS layers that held a value the fp16 split-half operands cannot
    carry and were therefore evaluated by the exact fp32 kernel instead (never clamped)."""
    return _counter(_REDO, device)


def range_redo_count(device="cuda"):
    """Host read (synchronises) and reset of ``range_redo_counter``: a statistic, not an error - those tiles have
    exact fp32 results."""
    c = range_redo_counter(device)
    n = int(c.item())
    c.zero_()
    return n


def check_discriminant(device="cuda"):
    """Host check (synchronises): raises AssertionError like splines.py:164 if an
    inverse spline saw a negative discriminant since the last check."""
    c = bad_discriminant_counter(device)
    n = int(c.item())
    c.zero_()
    assert n == 0, "negative discriminant in %d workgroup(s) of an inverse RQ spline" % n


def check_saturation(device="cuda", model=None):
    """Host check (synchronises) of the fp16 split-half matrix path: number of workgroups that clamped a value
    at the fp16 range since the last check (the reference is plain fp32 and does not clamp, nets/resnet.py:92-106).
    With ``model`` given and a non-zero count every fused RQS coupling of the model is switched to the exact
    fp32 matrix path (``fused_precision = 'fp32'``), so that re-running the evaluation gives reference results;
    and the training path's dense layers go back to the library's fp32 GEMMs (``autograd.TRAIN_MATRIX_PATH``);
    without a model a non-zero count raises VcnfError."""
    c = saturation_counter(device)
    n = int(c.item())
    c.zero_()
    if n and model is None:
        raise VcnfError("fp16 split-half matrix path clamped values at +-65504 in %d workgroup(s): "
                        "set fused_precision = 'fp32' on the couplings (or pass model=...) and re-run" % n)
    if n:
        from . import autograd
        autograd.TRAIN_MATRIX_PATH = "fp32"           # training path: the library's fp32 GEMMs (csrc/linear_f16x3.hip clamps too)
        for m in model.modules():
            if hasattr(m, "fused_precision"):
                m.fused_precision = "fp32"
            if hasattr(m, "fused_conv1x1"):           # ConvNet2d: back to the library's fp32 convolutions
                m.fused_conv1x1 = False
    return n


def _ld_out(out, b, dtype, dev, name=None):
    """(tensor, ld_mode) of a log-det / log-prob output: a fresh [batch] tensor to store into, or the caller's to
    accumulate into.  With ``name`` (the base distributions) the caller's tensor is checked first."""
    if out is None:
        return torch.empty(b, dtype=dtype, device=dev), LD_STORE
    if name is not None:
        require_device(out, f64=True)
        if out.dtype != dtype or not out.is_contiguous() or tuple(out.shape) != (b,):
            raise VcnfError(name + ": logp must be a contiguous [batch] tensor of the input's dtype")
    return out, LD_ACCUM


# ---------------------------------------------------------------- wrappers
def rqs_elementwise(x, uw, uh, ud, cfg, inverse, allow_grad=False):
    """x [...]; uw, uh [..., K]; ud [..., K-1 | K+1] (last dim contiguous)."""
    dev = require_device(x, uw, uh, ud, allow_grad=allow_grad, f64=True)
    shape = x.shape
    k = cfg.num_bins
    nd = n_derivatives(cfg)
    if uw.shape != shape + (k,) or uh.shape != shape + (k,) or ud.shape != shape + (nd,):
        raise VcnfError("spline parameter shapes %s %s %s do not match inputs %s with K=%d" % (
            tuple(uw.shape), tuple(uh.shape), tuple(ud.shape), tuple(shape), k))
    xf = x.reshape(-1).contiguous()

    def rows(t, width):
        t2 = t.reshape(-1, width)
        if t2.stride(1) != 1 or (t2.shape[0] > 1 and t2.stride(0) < width):
            t2 = t2.contiguous()
        return t2, (t2.stride(0) if t2.shape[0] > 1 else width)
    w2, ldw = rows(uw, k)
    h2, ldh = rows(uh, k)
    d2, ldd = rows(ud, nd)
    y = torch.empty_like(xf)
    lad = torch.empty_like(xf)
    if xf.dtype == torch.float64 and not all(t.dtype == torch.float64 for t in (w2, h2, d2)):
        raise VcnfError("fp64 spline: inputs and logits must all be fp64")
    _call("vcnf_rqs_elementwise" + _sfx(xf), dev, xf, w2, h2, d2, ldw, ldh, ldd, y, lad, xf.numel(), _cfg_of(cfg, xf),
          bool(inverse), _bad_if(inverse, dev))
    return y.view(shape), lad.view(shape)


def rqs_elementwise_image(x, params, cfg, inverse, allow_grad=False):
    """x [B, C, *inner] with the conditioner output params [B, C*P, *inner] read in place
    (the reference reshapes/permutes it to [B, C, *inner, P]; coupling.py:148-151).  fp32 or fp64 (both tensors)."""
    dev = require_device(x, params, allow_grad=allow_grad, f64=True)
    if params.dtype != x.dtype:
        raise VcnfError("rqs_elementwise_image: mixed dtypes (%s inputs, %s logits)" % (x.dtype, params.dtype))
    k, nd = cfg.num_bins, n_derivatives(cfg)
    p = 2 * k + nd
    b, c = x.shape[0], x.shape[1]
    inner = int(x[0, 0].numel())
    if tuple(params.shape) != (b, c * p) + tuple(x.shape[2:]):
        raise VcnfError("conditioner output %s does not match inputs %s with %d logits per element" % (
            tuple(params.shape), tuple(x.shape), p))
    x = x.contiguous()
    params = params.contiguous()
    y, lad = torch.empty_like(x), torch.empty_like(x)
    base, es = params.data_ptr(), params.element_size()     # widths | heights | derivatives: addresses inside params
    _call("vcnf_rqs_elementwise_strided" + _sfx(x), dev, x, base, base + es * k * inner, base + 2 * es * k * inner,
          p * inner, p * inner, p * inner, inner, inner, 0, y, lad, x.numel(), _cfg_of(cfg, x), bool(inverse),
          _bad_if(inverse, dev))
    return y, lad


def rqs_elementwise_shared(x, uw, uh, ud, cfg, inverse, allow_grad=False):
    """x [B, *shape] with one logit row per position of ``shape`` shared by the whole batch:
    uw, uh [*shape, K], ud [*shape, nd] (PiecewiseRationalQuadraticCDF, coupling.py:211-240)."""
    dev = require_device(x, uw, uh, ud, allow_grad=allow_grad)
    k, nd = cfg.num_bins, n_derivatives(cfg)
    shape = tuple(x.shape[1:])
    if tuple(uw.shape) != shape + (k,) or tuple(uh.shape) != shape + (k,) or tuple(ud.shape) != shape + (nd,):
        raise VcnfError("shared spline logits %s %s %s do not match positions %s with K=%d" % (
            tuple(uw.shape), tuple(uh.shape), tuple(ud.shape), shape, k))
    x = x.contiguous()
    uw, uh, ud = uw.contiguous(), uh.contiguous(), ud.contiguous()
    y, lad = torch.empty_like(x), torch.empty_like(x)
    period = int(x[0].numel())
    tables = torch.empty(period * 3 * (k + 1), dtype=torch.float32, device=dev)
    _call("vcnf_rqs_shared_f32", dev, x, uw, uh, ud, period, tables, y, lad, x.numel(), cfg, bool(inverse),
          _bad_if(inverse, dev))
    return y, lad


def rqs_packed_bwd(x, params, gy, glad, cfg, inverse):
    """VJP of rqs_elementwise_image: x, gy [B, C, *inner]; params [B, C*P, *inner]; glad [B]
    (gradient of the per-sample log-det).  Returns (g_x, g_params) in the layouts of x / params.  fp32 or fp64
    (every tensor)."""
    dev = require_device(x, params, gy, glad, allow_grad=True, f64=True)
    if any(t.dtype != x.dtype for t in (params, gy, glad)):
        raise VcnfError("rqs_packed_bwd: inputs, logits and upstream gradients must share one dtype")
    x, params = x.detach().contiguous(), params.detach().contiguous()
    gy, glad = gy.detach().contiguous(), glad.detach().contiguous()
    inner = int(x[0, 0].numel())
    gx, gp = torch.empty_like(x), torch.empty_like(params)
    _call("vcnf_rqs_packed_bwd" + _sfx(x), dev, x, params, inner, int(x[0].numel()), gy, glad, gx, gp, x.numel(),
          _cfg_of(cfg, x), bool(inverse))
    return gx, gp


SHARED_BWD_BINS = (4, 8, 10, 16)


def rqs_shared_bwd(x, uw, uh, ud, gy, glad, cfg, inverse):
    """VJP of rqs_elementwise_shared: x, gy [B, *shape]; glad [B]; returns (g_x, g_uw, g_uh, g_ud)."""
    dev = require_device(x, uw, uh, ud, gy, glad, allow_grad=True)
    k, nd = cfg.num_bins, n_derivatives(cfg)
    x, gy, glad = x.detach().contiguous(), gy.detach().contiguous(), glad.detach().contiguous()
    uw, uh, ud = uw.detach().contiguous(), uh.detach().contiguous(), ud.detach().contiguous()
    b, period = x.shape[0], int(x[0].numel())
    groups = int(lib().vcnf_rqs_shared_bwd_groups(b, period))
    gx = torch.empty_like(x)
    partial = torch.empty(groups, period, 2 * k + nd, dtype=torch.float32, device=dev)
    _call("vcnf_rqs_shared_bwd_f32", dev, x, uw, uh, ud, b, period, period, gy, glad, gx, partial, groups, cfg,
          bool(inverse))
    g = partial.sum(0)
    return gx, g[:, :k].reshape(uw.shape), g[:, k:2 * k].reshape(uh.shape), g[:, 2 * k:].reshape(ud.shape)


def rqs_elementwise_bwd(x, uw, uh, ud, gy, glad, cfg, inverse):
    """VJP of rqs_elementwise: returns (g_x, g_uw, g_uh, g_ud), shapes of the inputs.  fp32 or fp64 (every tensor)."""
    f64 = x.dtype == torch.float64
    dev = require_device(x, uw, uh, ud, gy, glad, allow_grad=True, f64=f64)
    if f64 and not all(t.dtype == torch.float64 for t in (uw, uh, ud, gy, glad)):
        raise VcnfError("fp64 spline VJP: inputs, logits and upstream gradients must all be fp64")
    k = cfg.num_bins
    nd = n_derivatives(cfg)
    shape = x.shape
    xf = x.detach().reshape(-1).contiguous()
    w2 = uw.detach().reshape(-1, k).contiguous()
    h2 = uh.detach().reshape(-1, k).contiguous()
    d2 = ud.detach().reshape(-1, nd).contiguous()
    gyf = gy.detach().reshape(-1).contiguous()
    glf = glad.detach().reshape(-1).contiguous()
    gx = torch.empty_like(xf)
    gw, gh, gd = torch.empty_like(w2), torch.empty_like(h2), torch.empty_like(d2)
    _call("vcnf_rqs_elementwise_bwd" + _sfx(xf), dev, xf, w2, h2, d2, k, k, nd, gyf, glf, gx, gw, gh, gd, xf.numel(),
          _cfg_of(cfg, xf), bool(inverse))
    return gx.view(shape), gw.view(shape + (k,)), gh.view(shape + (k,)), gd.view(shape + (nd,))


LIMIT_NAMES = ("left", "right", "bottom", "top")


def limit_layout(lim, shape):
    """(flat tensor, period, inner) of one interval limit broadcast against inputs of ``shape``: element i reads
    flat[(i // inner) % period].  Limits whose non-unit dimensions are one contiguous run of the inputs' dimensions
    (full shape, trailing shape, [B, 1], [C, 1, 1], 0-dim) are read in place; any other broadcastable shape is
    expanded to the full shape first."""
    shape = tuple(shape)
    try:
        ok = tuple(torch.broadcast_shapes(tuple(lim.shape), shape)) == shape
    except RuntimeError:
        ok = False
    if not ok:
        raise VcnfError("interval limit of shape %s does not broadcast to the inputs' shape %s" % (
            tuple(lim.shape), shape))
    ls = (1,) * (len(shape) - lim.dim()) + tuple(lim.shape)
    big = [j for j, s in enumerate(ls) if s != 1]
    if not big:
        return lim.reshape(1), 1, 1
    a, b = big[0], big[-1] + 1
    if all(ls[j] == shape[j] for j in range(a, b)):
        return lim.contiguous().reshape(-1), max(1, math.prod(shape[a:b])), max(1, math.prod(shape[b:]))
    return lim.expand(shape).contiguous().reshape(-1), max(1, math.prod(shape)), 1


def _limit_layouts(limits, x, allow_grad):
    """Checks of the four limit tensors against the inputs ``x`` and their layouts.  Same dtype as the inputs; on the
    inputs' device, except 0-dim host tensors (torch mixes those with device tensors), which are copied over."""
    lims = []
    for name, t in zip(LIMIT_NAMES, limits):
        if not torch.is_tensor(t):
            raise TypeError("interval limit %s is not a tensor" % name)
        if t.dtype != x.dtype:
            raise VcnfError("interval limit %s is %s, the inputs are %s" % (name, t.dtype, x.dtype))
        if not t.is_cuda:
            if t.dim() != 0:
                raise VcnfError("vcnf_amd computes on MI355X only (interval limit %s on %s); there is no CPU path"
                                % (name, t.device))
            t = t.to(x.device)
        lims.append(t)
    require_device(x, *lims, allow_grad=allow_grad, f64=True)
    return [limit_layout(t.detach(), x.shape) for t in lims]


def _limits_operands(x, uw, uh, ud, cfg, what):
    if cfg.tails != TAILS_NONE:
        raise VcnfError("%s: tensor interval limits belong to the spline without tails" % what)
    k = cfg.num_bins
    shape = tuple(x.shape)
    if tuple(uw.shape) != shape + (k,) or tuple(uh.shape) != shape + (k,) or tuple(ud.shape) != shape + (k + 1,):
        raise VcnfError("spline parameter shapes %s %s %s do not match inputs %s with K=%d" % (
            tuple(uw.shape), tuple(uh.shape), tuple(ud.shape), shape, k))
    if not all(t.dtype == x.dtype for t in (uw, uh, ud)):
        raise VcnfError("%s: inputs and logits must share one dtype" % what)
    return (x.detach().reshape(-1).contiguous(), uw.detach().reshape(-1, k).contiguous(),
            uh.detach().reshape(-1, k).contiguous(), ud.detach().reshape(-1, k + 1).contiguous())


def _bcast(lay):
    return RqsLimitBcast((_I64 * 4)(*[l[1] for l in lay]), (_I64 * 4)(*[l[2] for l in lay]))


def rqs_elementwise_limits(x, uw, uh, ud, limits, cfg, inverse, allow_grad=False):
    """rqs_elementwise with tensor interval limits ``limits`` = (left, right, bottom, top), each broadcastable to the
    shape of x (splines.py:99-102; no tails, K+1 derivative logits).  fp32 or fp64 (every tensor)."""
    dev = require_device(x, uw, uh, ud, allow_grad=allow_grad, f64=True)
    xf, w2, h2, d2 = _limits_operands(x, uw, uh, ud, cfg, "rqs_elementwise_limits")
    lay = _limit_layouts(limits, x, allow_grad)
    k = cfg.num_bins
    y, lad = torch.empty_like(xf), torch.empty_like(xf)
    _call("vcnf_rqs_elementwise_limits" + _sfx(xf), dev, xf, w2, h2, d2, k, k, k + 1, *[l[0] for l in lay], _bcast(lay),
          y, lad, xf.numel(), _cfg_of(cfg, xf), bool(inverse), _bad_if(inverse, dev))
    return y.view(x.shape), lad.view(x.shape)


def rqs_elementwise_limits_bwd(x, uw, uh, ud, limits, gy, glad, cfg, inverse, want=(True, True, True, True)):
    """VJP of rqs_elementwise_limits: (g_x, g_uw, g_uh, g_ud, [g_left, g_right, g_bottom, g_top]).  The kernel writes
    each limit's gradient per element; it is reduced to the limit's own shape with sum_to_size (deterministic, no
    atomics).  ``want[j]`` false: that limit's gradient is not computed (None)."""
    dev = require_device(x, uw, uh, ud, gy, glad, allow_grad=True, f64=True)
    if gy.dtype != x.dtype or glad.dtype != x.dtype:
        raise VcnfError("rqs_elementwise_limits_bwd: inputs and upstream gradients must share one dtype")
    xf, w2, h2, d2 = _limits_operands(x, uw, uh, ud, cfg, "rqs_elementwise_limits_bwd")
    lay = _limit_layouts(limits, x, True)
    k = cfg.num_bins
    shape = x.shape
    gyf, glf = gy.detach().reshape(-1).contiguous(), glad.detach().reshape(-1).contiguous()
    gx = torch.empty_like(xf)
    gw, gh, gd = torch.empty_like(w2), torch.empty_like(h2), torch.empty_like(d2)
    glim = [torch.empty_like(xf) if w else None for w in want]
    _call("vcnf_rqs_elementwise_limits_bwd" + _sfx(xf), dev, xf, w2, h2, d2, k, k, k + 1, *[l[0] for l in lay],
          _bcast(lay), gyf, glf, gx, gw, gh, gd, *glim, xf.numel(), _cfg_of(cfg, xf), bool(inverse))
    out = []
    for g, t in zip(glim, limits):
        out.append(None if g is None else g.view(shape).sum_to_size(t.shape).to(t.device))
    return gx.view(shape), gw.view(shape + (k,)), gh.view(shape + (k,)), gd.view(shape + (k + 1,)), out


def rqs_coupling(x, params, tf_idx, id_idx, shared, cfg, inverse, logdet=None, sign=1.0):
    """x [B,D] -> (y [B,D], logdet [B]).  ``logdet`` given: accumulate sign*sum
    into it; else a fresh tensor holding sign*sum."""
    dev = require_device(x, params, logdet, *(shared or ()))
    b, d = x.shape
    x = x.contiguous()
    params = params.contiguous()
    y = torch.empty_like(x)
    logdet, mode = _ld_out(logdet, b, torch.float32, dev)
    sw, sh, sd = shared if shared is not None else (None, None, None)
    _call("vcnf_rqs_coupling_f32", dev, x, params, tf_idx, tf_idx.numel(), id_idx, id_idx.numel(), sw, sh, sd, y,
          logdet, b, cfg, bool(inverse), mode, sign, _bad_if(inverse, dev), tag=b)
    return y, logdet


def rqs_conditioner_input(x, id_idx, context, shared, cfg, apply_inverse_shared):
    dev = require_device(x, context, *(shared or ()))
    b, d = x.shape
    x = x.contiguous()
    c = 0
    if context is not None:
        context = context.contiguous()
        c = context.shape[1]
    out = torch.empty(b, id_idx.numel() + c, dtype=torch.float32, device=dev)
    sw, sh, sd = shared if shared is not None else (None, None, None)
    _call("vcnf_rqs_conditioner_input_f32", dev, x, b, d, id_idx, id_idx.numel(), context, c, sw, sh, sd, cfg,
          bool(apply_inverse_shared), out)
    return out


_REDO_FLAGS = {}


def _redo_flags(dev, tiles):
    """Per-tile flag words of the split-half kernel's range check.  One grow-only buffer per (device, stream): the
    split-half launch writes it and the fp32 launch behind it on the same stream reads it, so consecutive layers can
    share it.  Under stream capture a fresh buffer is taken from the capturing allocator instead (a HIP graph keeps
    the address)."""
    if torch.cuda.is_current_stream_capturing():
        return torch.empty(tiles, dtype=torch.int32, device=dev)
    key = (device_index(dev), torch.cuda.current_stream().cuda_stream)
    buf = _REDO_FLAGS.get(key)
    if buf is None or buf.numel() < tiles:
        buf = torch.empty(max(tiles, 8192), dtype=torch.int32, device=dev)
        _REDO_FLAGS[key] = buf
    return buf


def small_batch_rows(rows=None):
    """Batch size up to which the fp16 split-half fused RQS layer runs on 32-sample tiles (csrc/fused_layer_v6s.hip)
    instead of 128-sample ones; ``rows`` sets it (0: never, a huge value: always), None only queries.  Returns the
    previous value.  Process-wide."""
    return int(lib().vcnf_rqs_layer_fused_small_batch_rows(-1 if rows is None else int(rows)))


def _range_safe_launches(name, dev, b, precision, first, second, launch):
    """The launch protocol of the fused RQS layer entry points (``name``) on a batch of ``b`` samples.
    ``launch(fn, operands, precision, counter, flags)`` makes one launch of the entry point ``fn`` and returns its
    status; ``first`` are the operands of the requested ``precision``, ``second`` the exact fp32 ones or None.
    precision 1 (fp16 split-half operands) with ``second`` is the range-safe pair: the split-half launch leaves tiles
    (32 samples, one flag each) that hold a non-finite input or a value beyond +-65504 unwritten, flags them and counts
    them in range_redo_counter; the fp32 launch behind it evaluates exactly the flagged tiles (normally none: it
    returns at once).  Without ``second`` the split-half kernel clamps and counts in saturation_counter.  bench.py's
    event bracket is around the first launch only."""
    safe = precision == 1 and second is not None
    fn = getattr(lib(), name)
    with torch.cuda.device(dev):
        flags = _redo_flags(dev, (b + 31) // 32) if safe and b > 0 else None
        counter = (range_redo_counter(dev) if safe else saturation_counter(dev)) if precision == 1 else None
        with _timed(b):
            st = launch(fn, first, precision, counter, flags)
        if st == OK and flags is not None:
            st = launch(fn, second, 0, None, flags)
    _check(st, name)


def rqs_layer_fused(x, context, tf_idx, id_idx, ctx_dim, hidden, num_blocks, precision, wpack, shared, cfg,
                    inverse, logdet=None, sign=1.0, wpack_f32=None, cfg_f32=None):
    """Whole coupling layer (conditioner included) in one kernel; see csrc/fused_layer.hip.
    precision 1 (fp16 split-half operands) with ``wpack_f32`` given is the range-safe form: the split-half launch
    leaves tiles that hold a non-finite input or a value beyond +-65504 unwritten and flags them, a launch of the
    exact fp32 kernel behind it evaluates exactly those tiles (normally none: it returns at once) - no host round
    trip, nothing clamped.  Without ``wpack_f32`` the split-half kernel clamps and counts (saturation_counter)."""
    dev = require_device(x, context, wpack, logdet, wpack_f32, *(shared or ()))
    b, d = x.shape
    x = x.contiguous()
    if context is not None:
        context = context.contiguous()
    y = torch.empty_like(x)
    logdet, mode = _ld_out(logdet, b, torch.float32, dev)
    sw, sh, sd = shared if shared is not None else (None, None, None)
    n_tf, n_id, ctx_dim, hidden, num_blocks = tf_idx.numel(), id_idx.numel(), int(ctx_dim), int(hidden), int(num_blocks)
    inverse, bad = bool(inverse), _bad_if(inverse, dev)

    def launch(fn, operands, prec, counter, flags):
        pack, cf = operands
        return fn(x, context, y, logdet, b, tf_idx, n_tf, id_idx, n_id, ctx_dim, hidden, num_blocks, prec, pack,
                  pack.numel(), sw, sh, sd, cf, inverse, mode, sign, bad, counter, flags, _stream())
    _range_safe_launches("vcnf_rqs_layer_fused_f32", dev, b, precision, (wpack, cfg),
                         None if wpack_f32 is None else (wpack_f32, cfg_f32 if cfg_f32 is not None else cfg), launch)
    return y, logdet


def rqs_stack_fused(x, context, layers, layers_f32, pack_floats, d_t, d_id, ctx_dim, hidden, num_blocks, precision, cfg,
                    inverse, logdet=None, sign=1.0):
    """A run of RQS coupling layers of one shape in ONE launch (csrc/fused_layer_v6s.hip; exact fp32:
    csrc/fused_layer.hip): ``layers`` is a ctypes array of RqsStackLayer in application order.  precision 1 with
    ``layers_f32`` (the same layers with their fp32 packings) is the range-safe pair of launches of rqs_layer_fused:
    tiles in which any layer left the fp16 range are re-evaluated through all layers on exact fp32 instructions."""
    dev = require_device(x, context, logdet)
    b = x.shape[0]
    x = x.contiguous()
    if context is not None:
        context = context.contiguous()
    y = torch.empty_like(x)
    logdet, mode = _ld_out(logdet, b, torch.float32, dev)
    dims = (int(d_t), int(d_id), int(ctx_dim), int(hidden), int(num_blocks))
    pack_floats, inverse, bad = int(pack_floats), bool(inverse), _bad_if(inverse, dev)

    def launch(fn, lay, prec, counter, flags):
        return fn(x, context, y, logdet, b, lay, len(lay), *dims, prec, pack_floats, cfg, inverse, mode, sign, bad,
                  counter, flags, _stream())
    _range_safe_launches("vcnf_rqs_stack_fused_f32", dev, b, precision, layers, layers_f32, launch)
    return y, logdet


def affine_coupling(z, param, t_off, d_t, scale_map, inverse, logdet=None, sign=1.0):
    """z [B, C, *inner] -> (out, logdet [B] or None when scale_map is NONE and no
    logdet was passed)."""
    dev = require_device(z, param, logdet, f64=True)
    if param.dtype != z.dtype or (logdet is not None and logdet.dtype != z.dtype):
        raise VcnfError("affine_coupling: mixed dtypes")
    z = z.contiguous()
    param = param.contiguous()
    b, c = z.shape[0], z.shape[1]
    inner = int(z[0, 0].numel()) if z.dim() > 2 else 1
    out = torch.empty_like(z)
    if logdet is None and scale_map == SCALE_NONE:      # a pure shift: no log-det tensor at all
        mode = LD_STORE
    else:
        logdet, mode = _ld_out(logdet, b, z.dtype, dev)
    _call("vcnf_affine_coupling" + _sfx(z), dev, z, param, out, logdet, b, c, inner, int(t_off), int(d_t),
          int(scale_map), bool(inverse), mode, sign)
    return out, logdet


def rqs_final_fused(x, h, out, tf_idx, d_t, hidden, wpack, cfg, inverse, partial=None, presplit=False):
    """Last conditioner layer + splines (csrc/fused_final.hip): writes out[:, tf_idx], returns the partial
    log-det rows [rows, B] (written into the first rows of ``partial`` when the caller brings the buffer)."""
    dev = require_device(x, h, out, wpack)
    x, h = x.contiguous(), h.contiguous()
    if not out.is_contiguous():
        raise VcnfError("rqs_final_fused writes into a contiguous output tensor")
    b, d = x.shape
    rows = int(lib().vcnf_rqs_final_fused_partial_rows(d_t, cfg.num_bins))
    if partial is None:
        partial = torch.empty(rows, b, dtype=torch.float32, device=dev)
    elif partial.shape[0] < rows or partial.shape[1] != b or not partial.is_contiguous():
        raise VcnfError("partial log-det buffer %s too small for %d rows of %d" % (tuple(partial.shape), rows, b))
    _call("vcnf_rqs_final_fused_presplit_f32" if presplit else "vcnf_rqs_final_fused_f32", dev, x, h, out, partial, b, d,
          tf_idx, int(d_t), int(hidden), wpack, wpack.numel(), cfg, bool(inverse), _bad_if(inverse, dev),
          tag="rqs_final_fused")
    return partial


def identity_half_rows(d_id, shared):
    return int(lib().vcnf_rqs_identity_half_partial_rows(d_id)) if shared is not None else 0


def rqs_identity_half(x, out, id_idx, d_id, shared, cfg, inverse, partial=None, want_cond_in=True):
    """Identity features of a coupling layer in one launch (csrc/rqs_kernels.hip::rqs_identity_half_kernel):
    out[:, id_idx] = S(x[:, id_idx]) (S^-1 when ``inverse``; the plain copy without ``shared`` logits), the
    conditioner's input rows [B, d_id] (raw columns in the density direction, S^-1 of them when sampling) and the
    log-det partial rows, written into ``partial`` (rows identity_half_rows(d_id, shared))."""
    dev = require_device(x, out, id_idx, *(shared or ()))
    x = x.contiguous()
    if not out.is_contiguous():
        raise VcnfError("rqs_identity_half writes into a contiguous output tensor")
    b, d = x.shape
    cond_in = torch.empty(b, d_id, dtype=torch.float32, device=dev) if want_cond_in else None
    if shared is not None:
        sw, sh, sd = (t.detach().contiguous() for t in shared)
        if partial is None or partial.shape[0] < identity_half_rows(d_id, shared) or partial.shape[1] != b:
            raise VcnfError("rqs_identity_half needs a [rows, B] partial log-det buffer")
    else:
        sw = sh = sd = None
    _call("vcnf_rqs_identity_half_f32", dev, x, out, cond_in, partial, b, d, id_idx, int(d_id), sw, sh,
          sd if sd is not None and sd.numel() else None, cfg, bool(inverse), bool(inverse), _bad_if(inverse, dev),
          tag="rqs_identity_half")
    return cond_in


def resnet_trunk(x, wpack, hidden, num_blocks, split=False):
    """ResidualNet trunk (initial layer + residual blocks) in one kernel; csrc/resnet_trunk.hip.  x [B, d_in] -> h [B, hidden]."""
    dev = require_device(x, wpack)
    x = x.contiguous()
    b, d_in = x.shape
    h = torch.empty(b, hidden, dtype=torch.float32, device=dev)
    args = (x, h, b, d_in, int(hidden), int(num_blocks), wpack, wpack.numel())
    if split:       # h: per row 128 fp16 hi halves | 128 fp16 lo halves, for rqs_final_fused(..., presplit=True)
        _call("vcnf_resnet_trunk_split_f32", dev, *args, saturation_counter(dev), tag="resnet_trunk")
    else:
        _call("vcnf_resnet_trunk_f32", dev, *args, tag="resnet_trunk")
    return h


def _affine_ld_out(logdet, b, scale_map, dev):
    """(logdet to return, logdet argument, ld_mode) of the fused affine wrappers: without a scale (a pure shift) the
    kernels take no log-det pointer, and a fresh log-det is zero."""
    if scale_map == SCALE_NONE:
        return (torch.zeros(b, dtype=torch.float32, device=dev) if logdet is None else logdet), None, \
            (LD_STORE if logdet is None else LD_ACCUM)
    logdet, mode = _ld_out(logdet, b, torch.float32, dev)
    return logdet, logdet, mode


def affine_layer_fused(z, wpack, cond_off, c_in, t_off, d_t, hidden, slope, scale_map, inverse, logdet=None,
                       sign=1.0, in_gather=None, out_gather=None):
    """Whole AffineCouplingBlock (MLP conditioner included) in one kernel; csrc/fused_affine.hip."""
    dev = require_device(z, wpack, logdet)
    z = z.contiguous()
    b, d = z.shape
    out = torch.empty_like(z)
    logdet, ld_arg, mode = _affine_ld_out(logdet, b, scale_map, dev)
    _call("vcnf_affine_layer_fused_f32", dev, z, out, ld_arg, b, d, int(cond_off), int(c_in), int(t_off), int(d_t),
          int(hidden), float(slope), int(scale_map), wpack, wpack.numel(), in_gather, out_gather, bool(inverse), mode,
          sign)
    return out, logdet


def affine_stack_fused(z, wpack, layers, gather_after, gathers, c_in, hidden, slope, scale_map, inverse, logdet=None,
                       sign=1.0, wpack_h3=None):
    """A run of AffineCouplingBlocks + the permutations between them in one kernel; csrc/fused_affine.hip.
    ``layers``: list of (cond_off, t_off, d_t, gather_before) in execution order; ``gathers`` int32 [rows, D] or None.
    ``wpack_h3``: the split-half fragments of the conditioners' second and third dense layers - then those run on the
    fp16 split-half matrix path (range fallback to the fp32 body on the device, counted in range_redo_counter)."""
    dev = require_device(z, wpack, logdet, gathers, wpack_h3)
    z = z.contiguous()
    b, d = z.shape
    out = torch.empty_like(z)
    logdet, ld_arg, mode = _affine_ld_out(logdet, b, scale_map, dev)
    arr = (AffineStackLayer * len(layers))(*[AffineStackLayer(*map(int, l)) for l in layers])
    head = (z, out, ld_arg, b, d, len(layers), arr, int(gather_after), int(c_in), int(hidden),
            float(slope), int(scale_map), wpack, wpack.numel())
    tail = (gathers, 0 if gathers is None else int(gathers.shape[0]), bool(inverse), mode, sign)
    if wpack_h3 is not None:
        _call("vcnf_affine_stack_fused_f16x3_f32", dev, *head, wpack_h3, wpack_h3.numel(), *tail,
              range_redo_counter(dev), tag="affine_stack_fused")
    else:
        _call("vcnf_affine_stack_fused_f32", dev, *head, *tail, tag="affine_stack_fused")
    return out, logdet


def masked_affine(z, s, t, bmask, inverse, logdet=None, sign=1.0):
    dev = require_device(z, s, t, bmask, logdet, f64=True)
    if any(u is not None and u.dtype != z.dtype for u in (s, t, bmask, logdet)):
        raise VcnfError("masked_affine: mixed dtypes")
    z = z.contiguous()
    s = s.contiguous() if s is not None else None
    t = t.contiguous() if t is not None else None
    b, d = z.shape
    out = torch.empty_like(z)
    logdet, mode = _ld_out(logdet, b, z.dtype, dev)
    _call("vcnf_masked_affine" + _sfx(z), dev, z, s, t, bmask, out, logdet, b, d, bool(inverse), mode, sign)
    return out, logdet


def maf_affine(x, params, inverse):
    """Masked-affine-autoregressive elementwise map on a MADE output [B, D * 2] (csrc/affine_kernels.hip::
    maf_affine_kernel): returns (y, log_det[B]) in the dtype of the inputs (fp32 or fp64)."""
    dev = require_device(x, params, f64=True)
    if params.dtype != x.dtype:
        raise VcnfError("maf_affine: mixed dtypes (%s inputs, %s params)" % (x.dtype, params.dtype))
    x, params = x.contiguous(), params.contiguous()
    b, d = x.shape
    if params.shape[0] != b or params[0].numel() != 2 * d:
        raise VcnfError("maf_affine: params %s do not match inputs %s" % (tuple(params.shape), tuple(x.shape)))
    out = torch.empty_like(x)
    ld = torch.empty(b, dtype=x.dtype, device=dev)
    _call("vcnf_maf_affine" + _sfx(x), dev, x, params, out, ld, b, d, bool(inverse), LD_STORE, 1.0)
    return out, ld


def made_sample_supported(features, hidden, num_blocks, params_per_feature, elem_size):
    """vcnf_made_sample_supported: whether the one-launch sampling kernel of the autoregressive flows has room for a
    MADE of this shape (its LDS budget; for splines, in both precisions, the bin counts with an instance: 8, 10, 16)."""
    return bool(lib().vcnf_made_sample_supported(int(features), int(hidden), int(num_blocks), int(params_per_feature),
                                                 int(elem_size)))


def made_sample(x, wpack, tables, ctx_add, ctx_gate, hidden, num_blocks, params_per_feature, cfg=None, logdet=None,
                sign=1.0):
    """vcnf_made_sample_*: the sampling direction of an autoregressive flow over x [B, D] in one launch from the packed
    operands of vcnf_amd.made_sample.pack (layouts: include/vcnf_hip.h).  ``cfg``: the spline constants, None for the
    affine map of the MAF (params_per_feature = 2).  Returns (y, logdet) - logdet a fresh [B] tensor holding
    sign * log|det|, or the caller's with that added.  fp32 or fp64, every floating tensor of x's dtype."""
    name = "vcnf_made_sample" + _sfx(x)
    dev = require_device(x, wpack, tables, ctx_add, ctx_gate, logdet, f64=True)
    if x.dim() != 2 or not x.is_contiguous():
        raise VcnfError(name + ": expects contiguous [batch, features] inputs")
    b, d = x.shape
    h, nb = int(hidden), int(num_blocks)
    if tables.dtype != torch.int32 or tuple(tables.shape) != (2 * d,) or not tables.is_contiguous():
        raise VcnfError(name + ": tables must be a contiguous int32 tensor of 2 * features entries")
    for what, t, shape in (("wpack", wpack, (wpack.numel(),)), ("ctx_add", ctx_add, (b, h)), ("ctx_gate", ctx_gate, (nb, b, h))):
        if t is not None and (t.dtype != x.dtype or tuple(t.shape) != shape or not t.is_contiguous()):
            raise VcnfError("%s: %s must be a contiguous %s tensor of shape %s" % (name, what, x.dtype, list(shape)))
    out = torch.empty_like(x)
    logdet, mode = _ld_out(logdet, b, x.dtype, dev, name)
    _call(name, dev, x, out, logdet, ctx_add, ctx_gate, wpack, wpack.numel(), tables, b, d, h, nb, int(params_per_feature),
          None if cfg is None else _cfg_of(cfg, x), mode, sign, None if cfg is None else bad_discriminant_counter(dev))
    return out, logdet


def affine_const(z, s, t, inverse):
    dev = require_device(z, s, t, f64=True)
    if any(u is not None and u.dtype != z.dtype for u in (s, t)):
        raise VcnfError("affine_const: mixed dtypes")
    z = z.contiguous()
    b, c = z.shape[0], z.shape[1]
    inner = int(z[0, 0].numel()) if z.dim() > 2 else 1
    out = torch.empty_like(z)
    _call("vcnf_affine_const" + _sfx(z), dev, z, s, t, out, b, c, inner, bool(inverse))
    return out


def conv1x1_fused(x, wpack, c_out, in_bias=None, out_bias=None, in_slope=None, out_slope=None):
    """act_out(W act_in(x + in_bias) + out_bias) for NCHW x in one pass (csrc/conv1x1.hip, fp16 split-half matrix path);
    a slope of None switches that LeakyReLU off."""
    dev = require_device(x, wpack, in_bias, out_bias)
    x = x.contiguous()
    b, c_in = x.shape[0], x.shape[1]
    inner = int(x[0, 0].numel())
    out = torch.empty((b, c_out) + tuple(x.shape[2:]), dtype=torch.float32, device=dev)
    _call("vcnf_conv1x1_f16x3_f32", dev, x, out, wpack, wpack.numel(), in_bias, out_bias, b, c_in, int(c_out), inner,
          in_slope is not None, float(in_slope or 0.0), out_slope is not None, float(out_slope or 0.0),
          saturation_counter(dev), tag="conv1x1_fused")
    return out


def masked_affine_stack(z, table, n_layers, inverse, logdet=None, sign=1.0):
    """A run of MaskedAffineFlow (+ MLP conditioners) and per-feature affine layers in one launch
    (csrc/masked_affine_stack.hip); ``table``: device int64 [n_layers, 12] as described in include/vcnf_hip.h."""
    dev = require_device(z, logdet, f64=True)
    z = z.contiguous()
    b, d = z.shape
    out = torch.empty_like(z)
    logdet, mode = _ld_out(logdet, b, z.dtype, dev)
    _call("vcnf_masked_affine_stack" + _sfx(z), dev, z, out, logdet, table, b, d, int(n_layers), bool(inverse), mode, sign)
    return out, logdet


def masked_affine_stack_bwd(z_out, g_out, g_ld, table, goff, n_layers, n_grad, inverse):
    """VJP of masked_affine_stack: (gradient of the run's input, flat parameter-gradient buffer [n_grad])."""
    dev = require_device(z_out, g_out, g_ld, f64=True, allow_grad=True)
    z_out, g_out = z_out.contiguous(), g_out.contiguous()
    if g_ld is not None:
        g_ld = g_ld.contiguous()
    b, d = z_out.shape
    g_in = torch.empty_like(z_out)
    grads = torch.zeros(n_grad, dtype=z_out.dtype, device=dev)
    _call("vcnf_masked_affine_stack_bwd" + _sfx(z_out), dev, z_out, g_out, g_ld, g_in, grads, table, goff, b, d,
          int(n_layers), bool(inverse))
    return g_in, grads


def _stream_key(dev):
    return (dev.index if dev.index is not None else torch.cuda.current_device(), torch.cuda.current_stream(dev).cuda_stream)


_AMAX_SCRATCH = {}    # per (device, stream), like _WGRAD_WS: the reduction's scratch.  Its first word must be zero
                      # between launches (the kernel leaves it so); a larger shape REPLACES the tensor, so a captured
                      # graph must have seen its largest cotangent during warm-up, as for _WGRAD_WS


def abs_max(t):
    """(row_amax [B], col_amax [N]): the largest |value| of every row and column of the fp32 matrix ``t`` [B, N], on the
    device (csrc/linear_wgrad.hip::abs_max_rows_cols_kernel; one launch, no host read).  The pair is what the ``amax``
    argument of linear_f16x3 (which takes the rows) and linear_wgrad (the columns) is."""
    dev = require_device(t, allow_grad=True)
    t = t.detach().contiguous()
    b, n = t.shape
    key = _stream_key(dev)
    scratch = _AMAX_SCRATCH.get(key)
    need = int(lib().vcnf_abs_max_rows_cols_scratch_floats(b, n))
    if need < 1:
        raise VcnfError("abs_max: unsupported shape %d x %d" % (b, n))
    if scratch is None or scratch.numel() < need:
        scratch = _AMAX_SCRATCH[key] = torch.zeros(need, dtype=torch.float32, device=dev)
    rows = torch.empty(b, dtype=torch.float32, device=dev)
    cols = torch.empty(n, dtype=torch.float32, device=dev)
    _call("vcnf_abs_max_rows_cols_f32", dev, t, b, n, rows, cols, scratch, scratch.numel(), tag="abs_max")
    return rows, cols


def _amax_or_none(t):
    """abs_max(t), or None for a shape the reduction does not take (more than 8192 columns): the kernels then run
    without the pre-scale, clamp and count."""
    return abs_max(t) if lib().vcnf_abs_max_rows_cols_scratch_floats(t.shape[0], t.shape[1]) > 0 else None


def linear_f16x3(x, weight, bias=None, input_grad=False, relu_in=False, relu_out=False, mask=None, addend=None,
                 prescale=None, amax=None):
    """nn.Linear on the fp16 split-half matrix path at training batch sizes (csrc/linear_f16x3.hip): ``x @ weight.T +
    bias`` for weight [out, in], or with ``input_grad`` the layer's input gradient ``x @ weight`` (x = the upstream
    gradient [B, out]).  The weight is read in place (no packed copy); ``relu_in`` / ``relu_out`` apply ReLU to x as it is
    read / to the result before it is stored; ``mask`` / ``addend`` [B, n]: result = addend + result * (mask > 0) (a ReLU's
    backward and a skip connection's gradient on the way out).  Clamped values are counted in saturation_counter
    (nf.check_saturation()).  ``prescale`` (default: with ``input_grad``, where x is a cotangent of any magnitude): every
    row of x travels times the power of two that puts its largest |value| in [2^14, 2^15), taken out of that row of the
    result exactly - nothing is clamped and 2^-k x gives 2^-k times the result bit for bit; ``amax``: ``abs_max(x)`` when
    the caller already has it (computed here otherwise)."""
    dev = require_device(x, weight, bias, allow_grad=True)
    x, weight = x.detach().contiguous(), weight.detach().contiguous()
    if input_grad if prescale is None else prescale:
        amax = _amax_or_none(x) if amax is None else amax
    else:
        amax = None
    b, k = x.shape
    n_out, n_in = weight.shape
    if input_grad:
        n, ldn, ldk = n_in, 1, n_in
        assert k == n_out and bias is None
    else:
        n, ldn, ldk = n_out, n_in, 1
        assert k == n_in
    y = torch.empty(b, n, dtype=torch.float32, device=dev)
    if bias is not None:
        bias = bias.detach().contiguous()
    if mask is not None:
        mask = mask.detach().contiguous()
    if addend is not None:
        addend = addend.detach().contiguous()
    _call("vcnf_linear_f16x3_f32", dev, x, weight, bias, y, b, k, n, ldn, ldk, bool(relu_in), bool(relu_out), mask,
          addend, amax[0] if amax is not None else None, saturation_counter(dev), tag="linear_f16x3")
    return y


_WGRAD_WS = {}        # workspace of the partial results per (device, stream): calls on one stream are ordered, calls on
                      # different streams (two models' backward passes, side streams) must not share it


def linear_wgrad(x, dy, want_bias=True, f16x3=False, relu_x=False, prescale=True, amax=None):
    """(dW [out, in], db [out] or None) of y = x W^T + b from x [B, in] and dy [B, out] (csrc/linear_wgrad.hip: the batch
    reduction split over the chip, deterministic; exact fp32 matrix instructions, or with ``f16x3`` the fp16 split-half
    matrix path - clamped values are counted in saturation_counter; there ``prescale`` / ``amax`` apply to the columns
    of dy as to the rows of x in linear_f16x3: a cotangent of any magnitude keeps its precision and is never clamped)."""
    dev = require_device(x, dy, allow_grad=True)
    x, dy = x.detach().contiguous(), dy.detach().contiguous()
    if relu_x and not f16x3:
        x = torch.relu(x)
    b, n_in = x.shape
    n_out = dy.shape[1]
    slices = int(lib().vcnf_linear_wgrad_slices(b, n_in, n_out))
    if slices < 1:
        raise VcnfError("linear_wgrad: unsupported layer shape %d -> %d" % (n_in, n_out))
    need = slices * (n_out * n_in + n_out)
    key = _stream_key(dev)
    ws = _WGRAD_WS.get(key)
    if ws is None or ws.numel() < need:
        ws = torch.empty(need, dtype=torch.float32, device=dev)
        _WGRAD_WS[key] = ws
    dw = torch.empty(n_out, n_in, dtype=torch.float32, device=dev)
    db = torch.empty(n_out, dtype=torch.float32, device=dev) if want_bias else None
    args = (x, dy, dw, db, ws, ws.numel(), b, n_in, n_out, 0)
    if f16x3:
        if prescale:
            amax = _amax_or_none(dy) if amax is None else amax
        _call("vcnf_linear_wgrad_f16x3_f32", dev, *args, bool(relu_x), amax[1] if prescale and amax is not None else None, saturation_counter(dev),
              tag="linear_wgrad")
    else:
        _call("vcnf_linear_wgrad_f32", dev, *args, tag="linear_wgrad")
    return dw, db


def conv3x3_1x1_fused(x, w1pack, w2pack, b1, b2, slope1, slope2):
    """leaky(W2 leaky(conv3x3(x) + b1) + b2) for NCHW x with 256 hidden / output channels in one launch
    (csrc/conv3x3_1x1.hip); the hidden activation between the layers never reaches memory."""
    dev = require_device(x, w1pack, w2pack, b1, b2)
    x = x.contiguous()
    b, c_in, h, w = x.shape
    out = torch.empty((b, 256, h, w), dtype=torch.float32, device=dev)
    _call("vcnf_conv3x3_1x1_f16x3_f32", dev, x, out, w1pack, w1pack.numel(), w2pack, w2pack.numel(), b1, b2, b, c_in, h, w,
          float(slope1), float(slope2), saturation_counter(dev), tag="conv3x3_1x1_fused")
    return out


def convnet3_fused(x, w1pack, w2pack, w3pack, b1, b2, b3, c_out, slope1, slope2):
    """Conv3x3 -> LeakyReLU -> Conv1x1 -> LeakyReLU -> Conv3x3 of the Glow conditioner (256 hidden channels) in two launches
    (csrc/conv3x3_1x1.hip): the fused kernel up to the last layer's nine tap results, then their shift-and-add."""
    dev = require_device(x, w1pack, w2pack, w3pack, b1, b2, b3)
    x = x.contiguous()
    b, c_in, h, w = x.shape
    z = torch.empty((b, 9 * c_out, h, w), dtype=torch.float32, device=dev)
    out = torch.empty((b, c_out, h, w), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):        # two entry points under one device context: _call would enter it twice
        with _timed("convnet3_taps"):
            st = _launch("vcnf_convnet3_taps_f16x3_f32", x, z, w1pack, w1pack.numel(), w2pack, w2pack.numel(), w3pack,
                         w3pack.numel(), b1, b2, b, c_in, int(c_out), h, w, float(slope1), float(slope2),
                         saturation_counter(dev))
        _check(st, "vcnf_convnet3_taps_f16x3_f32")
        with _timed("col2im3x3"):
            st = _launch("vcnf_col2im3x3_f32", z, b3, out, b, int(c_out), h, w)
    _check(st, "vcnf_col2im3x3_f32")
    return out


def resblock_op(op, a, b, c=None, two_outputs=False):
    """Fused elementwise map of csrc/resblock_ops.hip on contiguous fp32 tensors of one shape (ops 0-3, see the header)."""
    dev = require_device(a, b, c, allow_grad=True)
    a, b = a.detach().contiguous(), b.detach().contiguous()
    c = c.detach().contiguous() if c is not None else None
    out0 = torch.empty_like(a)
    out1 = torch.empty_like(a) if two_outputs else None
    _call("vcnf_resblock_elementwise_f32", dev, int(op), a, b, c, out0, out1, a.numel())
    return (out0, out1) if two_outputs else out0


def channel_mix(z, matrix, shift):
    """y[b, o, ...] = sum_c matrix[o, c] z[b, c, ...] + shift[o] (csrc/channel_mix.hip): invertible 1x1 convolution
    and ActNorm of a GlowBlock in one pass over the activations."""
    dev = require_device(z, matrix, shift)
    z = z.contiguous()
    b, c = z.shape[0], z.shape[1]
    if tuple(matrix.shape) != (c, c) or shift.numel() != c:
        raise VcnfError("channel_mix: matrix %s / shift %s do not match %d channels" % (
            tuple(matrix.shape), tuple(shift.shape), c))
    inner = int(z[0, 0].numel()) if z.dim() > 2 else 1
    out = torch.empty_like(z)
    _call("vcnf_channel_mix_f32", dev, z, out, matrix.contiguous(), shift.contiguous(), b, c, inner, tag="channel_mix")
    return out


def permute(z, idx32):
    dev = require_device(z, f64=True)
    z = z.contiguous()
    b, c = z.shape[0], z.shape[1]
    inner = int(z[0, 0].numel()) if z.dim() > 2 else 1
    out = torch.empty_like(z)
    _call("vcnf_permute" + _sfx(z), dev, z, idx32, out, b, c, inner)
    return out


def split_columns(z, idx32, first):
    """(z[:, idx[:first]], z[:, idx[first:]]) of z [B, C] as two contiguous tensors, one pass."""
    dev = require_device(z, f64=True)
    z = z.contiguous()
    b, c = z.shape
    if idx32.numel() != c or not 0 <= first <= c:
        raise VcnfError("split_columns: index of %d entries / first part of %d columns for %d columns" % (idx32.numel(), first, c))
    pa = torch.empty(b, first, dtype=z.dtype, device=dev)
    pb = torch.empty(b, c - first, dtype=z.dtype, device=dev)
    _call("vcnf_split_columns" + _sfx(z), dev, z, idx32, pa, pb, b, c, first)
    return pa, pb


def merge_columns(pa, pb, idx32):
    """cat([pa, pb], 1)[:, idx] for pa [B, Ca], pb [B, Cb] as one pass (no concatenated intermediate)."""
    dev = require_device(pa, pb, f64=True)
    if pa.dtype != pb.dtype or pa.shape[0] != pb.shape[0]:
        raise VcnfError("merge_columns: parts of different dtype / batch")
    pa, pb = pa.contiguous(), pb.contiguous()
    b, first = pa.shape
    c = first + pb.shape[1]
    if idx32.numel() != c:
        raise VcnfError("merge_columns: index of %d entries for %d columns" % (idx32.numel(), c))
    out = torch.empty(b, c, dtype=pa.dtype, device=dev)
    _call("vcnf_merge_columns" + _sfx(pa), dev, pa, pb, idx32, out, b, c, first)
    return out


def _log_t(temperature):
    return 0.0 if temperature is None else math.log(temperature)


def _check_index(idx, b, what, contiguous=False):
    """A per-sample index (class label, mixture mode): int32 [batch]."""
    if idx.dtype != torch.int32 or tuple(idx.shape) != (b,) or (contiguous and not idx.is_contiguous()):
        raise VcnfError("%s must be %s int32 tensor [batch]" % (what, "a contiguous" if contiguous else "an"))


def _like_input(t, x2, what, name, of="the input"):
    """Operand ``name`` of a base's entry point ``what`` that goes with the input rows ``x2`` [B, D] sample by sample
    (a cotangent, a second draw): cast to the input's dtype, as contiguous [B, D] rows."""
    if t.dim() < 1 or len(t) != len(x2) or t.numel() != x2.numel():
        raise VcnfError("%s: %s does not have the shape of %s" % (what, name, of))
    return t.to(x2.dtype).reshape(x2.shape).contiguous()


def _batch_vector(t, b, dtype, what, name):
    """Operand ``name`` of a base's entry point ``what`` with one value per sample: cast to ``dtype``, contiguous."""
    if tuple(t.shape) != (b,):
        raise VcnfError("%s: %s must be [batch]" % (what, name))
    return t.to(dtype).contiguous()


def _block_sums(dev, launch, what, outs, block, groups, reduce):
    """Tail of the VJPs that sum over the batch, under one device context.  ``launch`` (given the workspace or None)
    writes one partial block of shape ``block`` per workgroup and returns the status; ``groups`` = (entry point that
    gives the number of workgroups, its arguments (batch, ...)); ``reduce`` = (entry point that adds the blocks into the
    tensors ``outs`` in a fixed order, its size arguments).  ``outs`` None: nobody wants the sums - one launch without
    a workspace, None."""
    with torch.cuda.device(dev):
        if outs is None:
            _check(launch(None), what)
            return None
        (count, args), (red, dims) = groups, reduce
        if args[0] == 0:
            return tuple(t.zero_() for t in outs)
        n = int(getattr(lib(), count)(*args))
        if n < 1:
            _check(2, what)
        partials = torch.empty((n,) + tuple(block), dtype=outs[0].dtype, device=outs[0].device)
        _check(launch(partials), what)
        _check(_launch(red, partials, n, *dims, *outs), red)
        return outs


def diag_gaussian_log_prob(z, loc, log_scale, temperature=None, logp=None, sign=1.0):
    dev = require_device(z, loc, log_scale, logp, f64=True)
    if any(u is not None and u.dtype != z.dtype for u in (loc, log_scale, logp)):
        raise VcnfError("diag_gaussian_log_prob: mixed dtypes")
    b = z.shape[0]
    z2 = z.reshape(b, -1).contiguous()
    logp, mode = _ld_out(logp, b, z.dtype, dev)
    _call("vcnf_diag_gaussian_log_prob" + _sfx(z), dev, z2, loc.contiguous(), log_scale.contiguous(),
          _log_t(temperature), logp, b, z2.shape[1], mode, sign)
    return logp


def diag_gaussian_sample(eps, loc, log_scale, temperature=None):
    dev = require_device(eps, loc, log_scale, f64=True)
    if loc.dtype != eps.dtype or log_scale.dtype != eps.dtype:
        raise VcnfError("diag_gaussian_sample: mixed dtypes")
    b = eps.shape[0]
    e2 = eps.reshape(b, -1).contiguous()
    z = torch.empty_like(e2)
    logp = torch.empty(b, dtype=eps.dtype, device=dev)
    _call("vcnf_diag_gaussian_sample" + _sfx(eps), dev, e2, loc.contiguous(), log_scale.contiguous(),
          _log_t(temperature), z, logp, b, e2.shape[1])
    return z.view(eps.shape), logp


def _cc_operands(x, loc_rows, ls_rows, row_index, pixels, what):
    """Checked operands of the class-conditional Gaussian entry points: x [B, C, P...] (C * pixels elements per sample),
    tables [R, C], row_index int32 [B] or None (then R is 1 or B).  Returns (device, x as [B, d], B, C, R)."""
    dev = require_device(x, loc_rows, ls_rows, row_index, f64=True)
    if any(u is not None and u.dtype != x.dtype for u in (loc_rows, ls_rows)):
        raise VcnfError(what + ": mixed dtypes")
    b = x.shape[0]
    x2 = x.reshape(b, -1).contiguous()
    if ls_rows.dim() != 2 or (loc_rows is not None and loc_rows.shape != ls_rows.shape):
        raise VcnfError(what + ": parameter tables must be [rows, channels] of one shape")
    r, c = ls_rows.shape
    if pixels < 1 or c * pixels != x2.shape[1]:
        raise VcnfError("%s: %d channels x %d pixels for rows of %d elements" % (what, c, pixels, x2.shape[1]))
    if row_index is not None:
        _check_index(row_index, b, what + ": row_index")
    if row_index is None and r not in (1, b):
        raise VcnfError("%s: %d table rows for a batch of %d without row_index" % (what, r, b))
    return dev, x2, b, c, r


def cc_gaussian_log_prob(z, loc_rows, ls_rows, row_index, pixels, temperature=None, logp=None, sign=1.0):
    """vcnf_cc_gaussian_log_prob_*: log density [B] of z [B, C, pixels...] under per-sample, per-channel Gaussians from
    the tables loc_rows / ls_rows [R, C]; ``logp``: accumulate into it."""
    name = "vcnf_cc_gaussian_log_prob" + _sfx(z)
    dev, z2, b, c, r = _cc_operands(z, loc_rows, ls_rows, row_index, pixels, name)
    logp, mode = _ld_out(logp, b, z.dtype, dev, name)
    _call(name, dev, z2, loc_rows.contiguous(), ls_rows.contiguous(), row_index, _log_t(temperature), logp, b, c, pixels,
          r, mode, sign)
    return logp


def cc_gaussian_sample(eps, loc_rows, ls_rows, row_index, pixels, temperature=None):
    """vcnf_cc_gaussian_sample_*: (z, log p(z)) for the standard-normal draw eps [B, C, pixels...]."""
    name = "vcnf_cc_gaussian_sample" + _sfx(eps)
    dev, e2, b, c, r = _cc_operands(eps, loc_rows, ls_rows, row_index, pixels, name)
    z = torch.empty_like(e2)
    logp = torch.empty(b, dtype=eps.dtype, device=dev)
    _call(name, dev, e2, loc_rows.contiguous(), ls_rows.contiguous(), row_index, _log_t(temperature), z, logp, b, c,
          pixels, r)
    return z.view(eps.shape), logp


def cc_gaussian_log_prob_bwd(z, loc_rows, ls_rows, row_index, pixels, temperature, g):
    """vcnf_cc_gaussian_log_prob_bwd_*: (dz like z, d_loc [B, C], d_log_scale [B, C]) for the cotangent g [B]."""
    name = "vcnf_cc_gaussian_log_prob_bwd" + _sfx(z)
    dev, z2, b, c, r = _cc_operands(z, loc_rows, ls_rows, row_index, pixels, name)
    require_device(g, f64=True)
    dz = torch.empty_like(z2)
    d_loc = torch.empty(b, c, dtype=z.dtype, device=dev)
    d_ls = torch.empty(b, c, dtype=z.dtype, device=dev)
    _call(name, dev, z2, loc_rows.contiguous(), ls_rows.contiguous(), row_index, _log_t(temperature),
          g.to(z.dtype).contiguous(), dz, d_loc, d_ls, b, c, pixels, r)
    return dz.view(z.shape), d_loc, d_ls


def cc_gaussian_sample_bwd(eps, ls_rows, row_index, pixels, temperature, g_z, g_logp):
    """vcnf_cc_gaussian_sample_bwd_*: (d_eps like eps, d_loc [B, C], d_log_scale [B, C]) for the cotangents
    g_z (like eps) and g_logp [B]."""
    name = "vcnf_cc_gaussian_sample_bwd" + _sfx(eps)
    dev, e2, b, c, r = _cc_operands(eps, None, ls_rows, row_index, pixels, name)
    require_device(g_z, g_logp, f64=True)
    gz2 = g_z.to(eps.dtype).reshape(b, -1).contiguous()
    if gz2.shape != e2.shape:
        raise VcnfError(name + ": g_z does not have the shape of eps")
    d_eps = torch.empty_like(e2)
    d_loc = torch.empty(b, c, dtype=eps.dtype, device=dev)
    d_ls = torch.empty(b, c, dtype=eps.dtype, device=dev)
    _call(name, dev, e2, ls_rows.contiguous(), row_index, _log_t(temperature), gz2, g_logp.to(eps.dtype).contiguous(),
          d_eps, d_loc, d_ls, b, c, pixels, r)
    return d_eps.view(eps.shape), d_loc, d_ls


def cc_gaussian_reduce_rows(per_sample, row_index, rows):
    """vcnf_cc_gaussian_reduce_rows_*: [rows, C] sums of per_sample [B, C] over the samples of each row_index value, in
    a fixed order (bitwise reproducible; entries of row_index outside [0, rows) contribute to no row)."""
    name = "vcnf_cc_gaussian_reduce_rows" + _sfx(per_sample)
    dev = require_device(per_sample, row_index, f64=True)
    per_sample = per_sample.contiguous()
    b, c = per_sample.shape
    _check_index(row_index, b, name + ": row_index")
    out = torch.empty(rows, c, dtype=per_sample.dtype, device=dev)
    _call(name, dev, per_sample, row_index, out, b, c, rows)
    return out


def _gmm_operands(x, loc, ls, log_w, what):
    """Checked operands of the Gaussian mixture entry points: x [B, D], tables loc / ls [M, D], log_w [M], one dtype.
    Returns (device, x, loc, ls, log_w contiguous, B, D, M)."""
    dev = require_device(x, loc, ls, log_w, f64=True)
    if any(u.dtype != x.dtype for u in (loc, ls, log_w)):
        raise VcnfError(what + ": mixed dtypes")
    if ls.dim() != 2 or loc.shape != ls.shape or tuple(log_w.shape) != (ls.shape[0],):
        raise VcnfError(what + ": parameter tables must be [modes, features] and log_w [modes]")
    m, d = ls.shape
    if x.dim() != 2 or x.shape[1] != d:
        raise VcnfError("%s: inputs %s for %d features" % (what, tuple(x.shape), d))
    return dev, x.contiguous(), loc.contiguous(), ls.contiguous(), log_w.contiguous(), x.shape[0], d, m


def gmm_log_prob(z, loc, ls, log_w, logp=None, sign=1.0):
    """vcnf_gmm_log_prob_*: mixture log density [B] of z [B, D] under the modes loc / ls [M, D] with log weights
    log_w [M]; ``logp``: accumulate into it."""
    name = "vcnf_gmm_log_prob" + _sfx(z)
    dev, z2, loc, ls, log_w, b, d, m = _gmm_operands(z, loc, ls, log_w, name)
    logp, mode = _ld_out(logp, b, z.dtype, dev, name)
    _call(name, dev, z2, loc, ls, log_w, logp, b, d, m, mode, sign)
    return logp


def gmm_sample(eps, mode, loc, ls, log_w):
    """vcnf_gmm_sample_*: (z, log p(z)) for the standard-normal draw eps [B, D] and the drawn modes (int32 [B])."""
    name = "vcnf_gmm_sample" + _sfx(eps)
    dev, e2, loc, ls, log_w, b, d, m = _gmm_operands(eps, loc, ls, log_w, name)
    require_device(mode)
    _check_index(mode, b, name + ": mode", contiguous=True)
    z = torch.empty_like(e2)
    logp = torch.empty(b, dtype=eps.dtype, device=dev)
    _call(name, dev, e2, mode, loc, ls, log_w, z, logp, b, d, m)
    return z, logp


def gmm_log_prob_bwd(z, loc, ls, log_w, lse, g, gz_in=None, tables=True):
    """vcnf_gmm_log_prob_bwd_* and vcnf_gmm_reduce_partials_*: (dz [B, D], d_loc [M, D], d_log_scale [M, D],
    d_log_w [M]) for the cotangent g [B] of the log density; ``lse`` is the forward's result, ``gz_in`` [B, D] is added
    to dz.  ``tables`` false: no table needs a gradient - dz only (the three others are None), no workspace, one launch."""
    name = "vcnf_gmm_log_prob_bwd" + _sfx(z)
    dev, z2, loc, ls, log_w, b, d, m = _gmm_operands(z, loc, ls, log_w, name)
    require_device(lse, g, gz_in, f64=True)
    lse, g = _batch_vector(lse, b, z.dtype, name, "lse"), _batch_vector(g, b, z.dtype, name, "g")
    if gz_in is not None:
        gz_in = _like_input(gz_in, z2, name, "gz_in", "z")
    dz = torch.empty_like(z2)
    outs = (torch.empty_like(loc), torch.empty_like(ls), torch.empty_like(log_w)) if tables else None
    sums = _block_sums(dev, lambda ws: _launch(name, z2, loc, ls, log_w, lse, g, gz_in, dz, ws, b, d, m), name, outs,
                       (m, 2 * d + 1), ("vcnf_gmm_bwd_groups", (b, d, m)), ("vcnf_gmm_reduce_partials" + _sfx(z), (m, d)))
    return (dz,) + (sums or (None, None, None))


def _tail_operands(x, rows, what):
    """Checked operands of the heavy-tailed base entry points: x [B, ...] with D elements per sample and parameter rows of
    D elements each, one dtype.  Returns (device, x as [B, D] contiguous, the rows flat and contiguous, B, D)."""
    dev = require_device(x, *rows, f64=True)
    if any(u.dtype != x.dtype for u in rows):
        raise VcnfError(what + ": mixed dtypes")
    if x.dim() < 1:
        raise VcnfError(what + ": inputs need a batch dimension")
    b = x.shape[0]
    d = rows[0].numel()
    if d < 1 or any(u.numel() != d for u in rows) or x.numel() != b * d:
        raise VcnfError("%s: inputs %s for parameter rows of %s elements" % (what, tuple(x.shape), [u.numel() for u in rows]))
    return dev, x.reshape(b, d).contiguous(), [u.reshape(-1).contiguous() for u in rows], b, d


def tail_log_prob(z, loc, ls, shape, cst, family, logp=None, sign=1.0):
    """vcnf_tail_log_prob_*: log density [B] of z [B, ...] under the product of Student-t (family 0) or generalised
    Gaussian (1) factors with the rows loc / ls / shape / cst [D]; ``logp``: accumulate into it."""
    name = "vcnf_tail_log_prob" + _sfx(z)
    dev, z2, (loc, ls, shape, cst), b, d = _tail_operands(z, (loc, ls, shape, cst), name)
    logp, mode = _ld_out(logp, b, z.dtype, dev, name)
    _call(name, dev, z2, loc, ls, shape, cst, logp, b, d, int(family), mode, sign)
    return logp


def tail_sample(eps, gamma, loc, ls, shape, cst, family):
    """vcnf_tail_sample_*: (z like eps, log p(z) [B]) for the standard-normal draw eps and the gamma draw of its shape."""
    name = "vcnf_tail_sample" + _sfx(eps)
    dev, e2, (loc, ls, shape, cst), b, d = _tail_operands(eps, (loc, ls, shape, cst), name)
    require_device(gamma, f64=True)
    if gamma.dtype != eps.dtype:
        raise VcnfError(name + ": mixed dtypes")
    g2 = _like_input(gamma, e2, name, "gamma")
    z = torch.empty_like(e2)
    logp = torch.empty(b, dtype=eps.dtype, device=dev)
    _call(name, dev, e2, g2, loc, ls, shape, cst, z, logp, b, d, int(family))
    return z.view(eps.shape), logp


def _tail_row_sums(dev, launch, what, like, b, d, rows):
    """``launch`` and, with ``rows``, vcnf_tail_reduce_partials_*: (d_loc, d_log_scale, d_shape) [D], or three None."""
    outs = tuple(torch.empty(3, d, dtype=like.dtype, device=like.device)) if rows else None
    return _block_sums(dev, launch, what, outs, (3, d), ("vcnf_tail_bwd_groups", (b, d)),
                       ("vcnf_tail_reduce_partials" + _sfx(like), (d,))) or (None, None, None)


def tail_log_prob_bwd(z, loc, ls, shape, family, g, gz_in=None, rows=True):
    """vcnf_tail_log_prob_bwd_* and vcnf_tail_reduce_partials_*: (dz like z, d_loc, d_log_scale, d_shape [D]) for the
    cotangent g [B] of the log density; d_shape is the part that does not go through cst, ``gz_in`` (like z) is added
    to dz.  ``rows`` false: no row needs a gradient - dz only (the three others are None), no workspace, one launch."""
    name = "vcnf_tail_log_prob_bwd" + _sfx(z)
    dev, z2, (loc, ls, shape), b, d = _tail_operands(z, (loc, ls, shape), name)
    require_device(g, gz_in, f64=True)
    g = _batch_vector(g, b, z.dtype, name, "g")
    if gz_in is not None:
        gz_in = _like_input(gz_in, z2, name, "gz_in")
    dz = torch.empty_like(z2)
    family = int(family)
    sums = _tail_row_sums(dev, lambda ws: _launch(name, z2, loc, ls, shape, g, gz_in, dz, ws, b, d, family), name, z2,
                          b, d, rows)
    return (dz.view(z.shape),) + sums


def tail_sample_bwd(eps, gamma, loc, ls, shape, family, g_z=None, g_lp=None, rows=True, want_eps=True):
    """vcnf_tail_sample_bwd_* and vcnf_tail_reduce_partials_*: (d_eps like eps or None, d_gamma like eps, d_loc,
    d_log_scale, d_shape [D]) for the cotangents g_z (like eps) and g_lp [B] of vcnf_tail_sample_*; None is zero."""
    name = "vcnf_tail_sample_bwd" + _sfx(eps)
    dev, e2, (loc, ls, shape), b, d = _tail_operands(eps, (loc, ls, shape), name)
    require_device(gamma, g_z, g_lp, f64=True)
    g2 = _like_input(gamma, e2, name, "gamma")
    if g_z is not None:
        g_z = _like_input(g_z, e2, name, "g_z")
    if g_lp is not None:
        g_lp = _batch_vector(g_lp, b, eps.dtype, name, "g_lp")
    d_eps = torch.empty_like(e2) if want_eps else None
    d_gamma = torch.empty_like(e2)
    family = int(family)
    sums = _tail_row_sums(dev, lambda ws: _launch(name, e2, g2, loc, ls, shape, g_z, g_lp, d_eps, d_gamma, ws, b, d,
                                                  family), name, e2, b, d, rows)
    return (d_eps.view(eps.shape) if want_eps else None, d_gamma.view(eps.shape)) + sums


def _vae_rows(name, dtype, *operands):
    """Operands of a vcnf_vae_* entry point given as (tensor or None, rows, columns, what): each as contiguous
    [rows, columns] of ``dtype`` (None stays None).  Returns (device, the operands)."""
    dev = require_device(*[t for t, _, _, _ in operands], f64=True)
    out = []
    for t, rows, cols, what in operands:
        if t is not None:
            if t.dtype != dtype:
                raise VcnfError(name + ": mixed dtypes")
            if t.numel() != rows * cols:
                raise VcnfError("%s: %s %s is not [%d, %d]" % (name, what, tuple(t.shape), rows, cols))
            t = t.reshape(rows, cols).contiguous()
        out.append(t)
    return dev, out


def _vae_encode_sizes(name, h, eps):
    """(B, S, D) of h [B, 2 D elements] and eps [B, S, D elements]."""
    if h.dim() < 2 or eps.dim() < 2 or len(h) != len(eps) or h[0].numel() % 2:
        raise VcnfError("%s: h %s and eps %s are not [B, 2 D] and [B, S, D]" % (name, tuple(h.shape), tuple(eps.shape)))
    return len(h), eps.shape[1], h[0].numel() // 2


def vae_encode(h, eps):
    """vcnf_vae_encode_*: (z like eps, log q [B, S]) of the draw eps [B, S, ...] under the Gaussian whose parameter rows
    h [B, ...] hold [mean | log variance], D elements each."""
    name = "vcnf_vae_encode" + _sfx(eps)
    b, s, d = _vae_encode_sizes(name, h, eps)
    dev, (h2, e2) = _vae_rows(name, eps.dtype, (h, b, 2 * d, "h"), (eps, b * s, d, "eps"))
    z = torch.empty_like(e2)
    logq = torch.empty(b * s, dtype=eps.dtype, device=dev)
    if b * s:
        _call(name, dev, h2, e2, z, logq, b, s, d)
    return z.view(eps.shape), logq.view(b, s)


def vae_encode_bwd(h, eps, g_z=None, g_lq=None):
    """vcnf_vae_encode_bwd_*: d_h like h for the cotangents g_z (like eps) and g_lq [B, S] of vcnf_vae_encode_*; None is
    zero (not both).  At most VAE_MAX_SAMPLES samples per item."""
    name = "vcnf_vae_encode_bwd" + _sfx(eps)
    b, s, d = _vae_encode_sizes(name, h, eps)
    dev, (h2, e2, g_z, g_lq) = _vae_rows(name, eps.dtype, (h, b, 2 * d, "h"), (eps, b * s, d, "eps"),
                                         (g_z, b * s, d, "g_z"), (g_lq, b * s, 1, "g_lq"))
    d_h = torch.empty_like(h2)
    if b:
        _call(name, dev, h2, e2, g_z, g_lq, d_h, b, s, d)
    return d_h.view(h.shape)


def _vae_gauss_sizes(name, v, h, v_div, h_div):
    """(N, D) of v [N / v_div, D elements] and h [N / h_div, 2 D elements]."""
    n = len(v) * v_div
    if v.dim() < 2 or h.dim() < 2 or len(h) * h_div != n or h[0].numel() != 2 * v[0].numel():
        raise VcnfError("%s: v %s (divisor %d) and h %s (divisor %d) do not go together" % (
            name, tuple(v.shape), v_div, tuple(h.shape), h_div))
    return n, v[0].numel()


def vae_gauss_log_prob(v, h, v_div=1, h_div=1):
    """vcnf_vae_gauss_log_prob_*: log density [N] of the values v [N / v_div, ...] under the Gaussians with the parameter
    rows h [N / h_div, ...] = [mean | log variance]; row n reads v[n // v_div] and h[n // h_div]."""
    name = "vcnf_vae_gauss_log_prob" + _sfx(v)
    n, d = _vae_gauss_sizes(name, v, h, v_div, h_div)
    dev, (v2, h2) = _vae_rows(name, v.dtype, (v, n // v_div, d, "v"), (h, n // h_div, 2 * d, "h"))
    logp = torch.empty(n, dtype=v.dtype, device=dev)
    if n:
        _call(name, dev, v2, h2, logp, n, v_div, h_div, d)
    return logp


def vae_gauss_log_prob_bwd(v, h, g, v_div=1, h_div=1, want_v=True, want_h=True):
    """vcnf_vae_gauss_log_prob_bwd_*: (d_v like v or None, d_h like h or None) for the cotangent g [N]; the operand with
    the divisor is summed over its rows (at most VAE_MAX_SAMPLES of them)."""
    name = "vcnf_vae_gauss_log_prob_bwd" + _sfx(v)
    n, d = _vae_gauss_sizes(name, v, h, v_div, h_div)
    dev, (v2, h2, g) = _vae_rows(name, v.dtype, (v, n // v_div, d, "v"), (h, n // h_div, 2 * d, "h"), (g, n, 1, "g"))
    d_v = torch.empty_like(v2) if want_v else None
    d_h = torch.empty_like(h2) if want_h else None
    if n:
        _call(name, dev, v2, h2, g, d_v, d_h, n, v_div, h_div, d)
    return d_v.view(v.shape) if want_v else None, d_h.view(h.shape) if want_h else None


def _vae_bernoulli_sizes(name, x, score, x_div):
    if x.dim() < 2 or score.dim() < 2 or len(x) * x_div != len(score) or x[0].numel() != score[0].numel():
        raise VcnfError("%s: x %s (divisor %d) and the scores %s do not go together" % (
            name, tuple(x.shape), x_div, tuple(score.shape)))
    return len(score), x[0].numel()


def vae_bernoulli_log_prob(x, score, x_div=1):
    """vcnf_vae_bernoulli_log_prob_*: log likelihood [N] of the data x [N / x_div, ...] (values in [0, 1]) under the
    Bernoulli scores (logits) [N, ...]; row n reads x[n // x_div]."""
    name = "vcnf_vae_bernoulli_log_prob" + _sfx(score)
    n, d = _vae_bernoulli_sizes(name, x, score, x_div)
    dev, (x2, s2) = _vae_rows(name, score.dtype, (x, n // x_div, d, "x"), (score, n, d, "score"))
    logp = torch.empty(n, dtype=score.dtype, device=dev)
    if n:
        _call(name, dev, x2, s2, logp, n, x_div, d)
    return logp


def vae_bernoulli_log_prob_bwd(x, score, g, x_div=1):
    """vcnf_vae_bernoulli_log_prob_bwd_*: d_score like the scores for the cotangent g [N]; x gets no gradient.  At most
    VAE_MAX_SAMPLES rows per data item."""
    name = "vcnf_vae_bernoulli_log_prob_bwd" + _sfx(score)
    n, d = _vae_bernoulli_sizes(name, x, score, x_div)
    dev, (x2, s2, g) = _vae_rows(name, score.dtype, (x, n // x_div, d, "x"), (score, n, d, "score"), (g, n, 1, "g"))
    d_score = torch.empty_like(s2)
    if n:
        _call(name, dev, x2, s2, g, d_score, n, x_div, d)
    return d_score.view(score.shape)


def periodic(z, half, shift, sign, out=None):
    """vcnf_periodic_*: z [..., D] contiguous with the columns where half [D] is non-zero wrapped into [-half, half) after
    adding sign * shift [D] (None: no shift); ``out``: write there (``out is z``: in place)."""
    name = "vcnf_periodic" + _sfx(z)
    dev = require_device(z, half, shift, out, f64=True)
    d = half.numel()
    if z.dim() < 1 or z.shape[-1] != d or not z.is_contiguous():
        raise VcnfError("%s: inputs %s are not contiguous rows of %d columns" % (name, tuple(z.shape), d))
    if any(t is not None and (t.dtype != z.dtype or t.numel() != d or not t.is_contiguous()) for t in (half, shift)):
        raise VcnfError(name + ": the tables must be contiguous [features] tensors of the input's dtype")
    if out is None:
        out = torch.empty_like(z)
    elif out is not z and (out.shape != z.shape or out.dtype != z.dtype or not out.is_contiguous()):
        raise VcnfError(name + ": out must be a contiguous tensor of the input's shape and dtype")
    _call(name, dev, z, half, shift, out, z.numel() // d, d, float(sign))
    return out


def uniform_gaussian_log_prob(z, inv_scale_g, const_term, logp=None):
    """vcnf_uniform_gaussian_log_prob_*: const_term - sum((z inv_scale_g)^2) / 2 per row of z [B, D]; ``logp``: accumulate
    into it."""
    name = "vcnf_uniform_gaussian_log_prob" + _sfx(z)
    dev, z2, (inv,), b, d = _tail_operands(z, (inv_scale_g,), name)
    logp, mode = _ld_out(logp, b, z.dtype, dev, name)
    _call(name, dev, z2, inv, float(const_term), logp, b, d, mode)
    return logp


def uniform_gaussian_sample(eps, src, offset, scale, const_term, inv_scale_g):
    """vcnf_uniform_gaussian_sample_*: (z [B, D], log p(z) [B]) with z[:, j] = scale[j] (eps[:, src[j]] - offset[j])."""
    name = "vcnf_uniform_gaussian_sample" + _sfx(eps)
    dev, e2, (offset, scale, inv), b, d = _tail_operands(eps, (offset, scale, inv_scale_g), name)
    require_device(src)
    if src.dtype != torch.int32 or src.numel() != d or not src.is_contiguous():
        raise VcnfError(name + ": src must be a contiguous int32 tensor [features]")
    z = torch.empty_like(e2)
    logp = torch.empty(b, dtype=eps.dtype, device=dev)
    _call(name, dev, e2, src, offset, scale, float(const_term), inv, z, logp, b, d)
    return z, logp


def uniform_gaussian_log_prob_bwd(z, inv_scale_g, g):
    """vcnf_uniform_gaussian_log_prob_bwd_*: d_z like z for the cotangent g [B] of the log density."""
    name = "vcnf_uniform_gaussian_log_prob_bwd" + _sfx(z)
    dev, z2, (inv,), b, d = _tail_operands(z, (inv_scale_g,), name)
    require_device(g, f64=True)
    g = _batch_vector(g, b, z.dtype, name, "g")
    dz = torch.empty_like(z2)
    _call(name, dev, z2, inv, g, dz, b, d)
    return dz.view(z.shape)


def _logit_rows(name, x, *like):
    """Checked operands of the vcnf_logit_* entry points: x [B, ...] contiguous with D >= 1 elements per item, the
    tensors ``like`` (None allowed) contiguous, of its shape, dtype and device.  Returns (device, B, D)."""
    dev = require_device(x, *like, f64=True)
    d = math.prod(x.shape[1:]) if x.dim() >= 1 else 0
    if d < 1 or not x.is_contiguous():
        raise VcnfError("%s: inputs %s are not contiguous [batch, ...] items of at least one element" % (name, tuple(x.shape)))
    if any(t is not None and (t.shape != x.shape or t.dtype != x.dtype or not t.is_contiguous()) for t in like):
        raise VcnfError(name + ": every operand must be a contiguous tensor of the input's shape and dtype")
    return dev, len(x), d


def logit(x, alpha, inverse, logdet=None, sign=1.0):
    """vcnf_logit_inverse_* / vcnf_logit_forward_*: (out like x, log-det [B]) of the Logit transform in the density
    direction (``inverse``) or the sampling direction; ``logdet``: add sign * log-det into it."""
    name = ("vcnf_logit_inverse" if inverse else "vcnf_logit_forward") + _sfx(x)
    dev, b, d = _logit_rows(name, x)
    out = torch.empty_like(x)
    logdet, mode = _ld_out(logdet, b, x.dtype, dev, name)
    if b:                       # an empty tensor has no address: nothing to launch
        _call(name, dev, x, float(alpha), out, logdet, b, d, mode, float(sign))
    return out, logdet


def logit_bwd(x, alpha, inverse, g_out=None, g_ld=None):
    """vcnf_logit_inverse_bwd_* / vcnf_logit_forward_bwd_*: the gradient like x of a direction's input for the
    cotangents g_out (like x) and g_ld [B] of its two outputs; None: zero."""
    name = ("vcnf_logit_inverse_bwd" if inverse else "vcnf_logit_forward_bwd") + _sfx(x)
    if g_out is not None:
        g_out = g_out.contiguous()
    dev, b, d = _logit_rows(name, x, g_out)
    if g_ld is not None:
        require_device(g_ld, f64=True)
        g_ld = _batch_vector(g_ld, b, x.dtype, name, "g_ld")
    d_x = torch.empty_like(x)
    if b:
        _call(name, dev, x, float(alpha), g_out, g_ld, d_x, b, d)
    return d_x


def logit_inverse_u8(x_u8, noise, jitter, scale, alpha, logdet=None, sign=1.0):
    """vcnf_logit_inverse_u8_*: (z, log-det [B]) of the Logit density direction at ((byte / 255) + noise * jitter) *
    scale for the bytes x_u8 [B, ...] and the uniform draws ``noise`` of their shape, in the dtype of ``noise``."""
    name = "vcnf_logit_inverse_u8" + _sfx(noise)
    dev, b, d = _logit_rows(name, noise)
    require_device(x_u8)
    if x_u8.dtype != torch.uint8 or x_u8.shape != noise.shape or not x_u8.is_contiguous() or x_u8.device != dev:
        raise VcnfError(name + ": the bytes must be a contiguous uint8 tensor of the noise's shape on its device")
    z = torch.empty_like(noise)
    logdet, mode = _ld_out(logdet, b, noise.dtype, dev, name)
    if b:
        _call(name, dev, x_u8, noise, float(jitter), float(scale), float(alpha), z, logdet, b, d, mode, float(sign))
    return z, logdet


_COLUMN_TABLES = {}


def column_tables(columns, levels, features, device):
    """(slot [D] int32, levels [C] int32) on ``device`` for the categorical ``columns`` of rows of D = ``features``: slot
    holds -1 for a continuous column and otherwise the column's index into the [B, C] operands of the vcnf_dequant_*
    entry points.  Built once per (columns, levels, D, device) and kept."""
    key = (tuple(columns), tuple(levels), int(features), torch.device(device))
    if key not in _COLUMN_TABLES:
        if len(key[0]) != len(key[1]) or len(set(key[0])) != len(key[0]) or any(not 0 <= c < features for c in key[0]) \
                or any(k < 1 for k in key[1]):
            raise VcnfError("categorical columns %s with levels %s do not fit rows of %d features" % (key[0], key[1], features))
        slot = [-1] * int(features)
        for i, c in enumerate(key[0]):
            slot[c] = i
        _COLUMN_TABLES[key] = (torch.tensor(slot, dtype=torch.int32, device=device),
                               torch.tensor(key[1], dtype=torch.int32, device=device).reshape(len(key[1])))
    return _COLUMN_TABLES[key]


def _dequant_rows(name, x, slot, levels, *per_column, like=()):
    """Checked operands of the vcnf_dequant_* / vcnf_quantize_* entry points: rows x [B, D] contiguous, the tables of
    ``column_tables`` for D, the tensors ``per_column`` [B, C] and ``like`` [B, D] (None allowed) contiguous, of its
    dtype and device.  Returns (device, B, D, C)."""
    dev = require_device(x, *per_column, *like, f64=True)
    require_device(slot, levels)
    if x.dim() != 2 or x.shape[1] < 1 or not x.is_contiguous():
        raise VcnfError("%s: inputs %s are not contiguous [batch, features] rows" % (name, tuple(x.shape)))
    b, d = x.shape
    c = len(levels)
    if slot.dtype != torch.int32 or levels.dtype != torch.int32 or tuple(slot.shape) != (d,) or levels.dim() != 1 \
            or c > d or slot.device != dev or levels.device != dev:
        raise VcnfError(name + ": slot [features] and levels [n_cat <= features] must be int32 tensors on the rows' device")
    for t, shape in [(t, (b, c)) for t in per_column] + [(t, (b, d)) for t in like]:
        if t is not None and (tuple(t.shape) != shape or t.dtype != x.dtype or not t.is_contiguous()):
            raise VcnfError("%s: every operand must be a contiguous %s tensor of the rows' dtype" % (name, list(shape)))
    return dev, b, d, c


def dequant_prepare(x, slot, levels, u, alpha, logdet=None, sign=1.0):
    """vcnf_dequant_prepare_*: (v, ctx, log-det [B]) for the rows x [B, D] and the uniform draws u [B, C]: the logit of
    the draws, the rows' categories scaled to [-1, 1] and the log-det of u -> v; ``logdet``: add sign * log-det into it."""
    name = "vcnf_dequant_prepare" + _sfx(x)
    dev, b, d, c = _dequant_rows(name, x, slot, levels, u)
    v, ctx = torch.empty_like(u), torch.empty_like(u)
    logdet, mode = _ld_out(logdet, b, x.dtype, dev, name)
    if b and c:
        _call(name, dev, x, slot, levels, u, float(alpha), v, ctx, logdet, b, d, c, mode, float(sign))
    elif mode == LD_STORE:
        logdet.zero_()
    return v, ctx, logdet


def dequant_merge(x, slot, levels, w, noise_is_logit, alpha, logdet=None, sign=1.0):
    """vcnf_dequant_merge_*: (out [B, D], log-det [B]) of the rows x with the noise w [B, C] merged into their categorical
    columns; ``noise_is_logit``: w is the logit of the noise (variational) and not the noise itself."""
    name = "vcnf_dequant_merge" + _sfx(x)
    dev, b, d, c = _dequant_rows(name, x, slot, levels, w)
    out = torch.empty_like(x)
    logdet, mode = _ld_out(logdet, b, x.dtype, dev, name)
    if b:                       # an empty tensor has no address: nothing to launch
        _call(name, dev, x, slot, levels, w if c else x, int(bool(noise_is_logit)), float(alpha), out, logdet, b, d, c, mode,
              float(sign))
    return out, logdet


def dequant_merge_bwd(x, slot, levels, w, noise_is_logit, alpha, g_out=None, g_ld=None, want_x=False):
    """vcnf_dequant_merge_bwd_*: (d_w [B, C], d_x [B, D] or None) for the cotangents g_out [B, D] and g_ld [B] of
    ``dequant_merge``'s two outputs; None: zero."""
    name = "vcnf_dequant_merge_bwd" + _sfx(x)
    if g_out is not None:
        g_out = g_out.contiguous()
    dev, b, d, c = _dequant_rows(name, x, slot, levels, w, like=(g_out,))
    if g_ld is not None:
        require_device(g_ld, f64=True)
        g_ld = _batch_vector(g_ld, b, x.dtype, name, "g_ld")
    d_w = torch.empty_like(w)
    d_x = torch.empty_like(x) if want_x else None
    if b:
        _call(name, dev, x, slot, levels, w if c else x, int(bool(noise_is_logit)), float(alpha), g_out, g_ld,
              d_w if c else x, d_x, b, d, c)
    return d_w, d_x


def quantize(z, slot, levels, alpha, logdet=None, sign=1.0):
    """vcnf_quantize_*: (out [B, D], log-det [B]): the categorical columns of z mapped back to integer codes, the others
    copied, and the log-det of the continuous map in front of the floor."""
    name = "vcnf_quantize" + _sfx(z)
    dev, b, d, c = _dequant_rows(name, z, slot, levels)
    out = torch.empty_like(z)
    logdet, mode = _ld_out(logdet, b, z.dtype, dev, name)
    if b:
        _call(name, dev, z, slot, levels, float(alpha), out, logdet, b, d, c, mode, float(sign))
    return out, logdet


def _mvn_operands(x, loc, tri, consts, what):
    """Checked operands of the full-covariance base entry points: x [B, D], loc [D] (or None), tri [D, D], consts [2],
    one dtype.  Returns (device, x, loc, tri, consts contiguous, B, D)."""
    dev = require_device(x, loc, tri, consts, f64=True)
    if any(u is not None and u.dtype != x.dtype for u in (loc, tri, consts)):
        raise VcnfError(what + ": mixed dtypes")
    if tri.dim() != 2 or tri.shape[0] != tri.shape[1] or tuple(consts.shape) != (2,):
        raise VcnfError(what + ": tri must be [features, features] and consts [2]")
    d = tri.shape[0]
    if x.dim() != 2 or x.shape[1] != d or (loc is not None and loc.numel() != d):
        raise VcnfError("%s: inputs %s for %d features" % (what, tuple(x.shape), d))
    return (dev, x.contiguous(), None if loc is None else loc.reshape(-1).contiguous(), tri.contiguous(),
            consts.contiguous(), x.shape[0], d)


def mvn_log_prob(z, loc, tri_inv, consts, family, logp=None, sign=1.0):
    """vcnf_mvn_log_prob_*: log density [B] of z [B, D] under the multivariate Gaussian (family 0) or Student-t (1) with
    location loc [D], inverse scale factor tri_inv [D, D] (lower triangle) and consts = (cst, nu); ``logp``: accumulate
    into it."""
    name = "vcnf_mvn_log_prob" + _sfx(z)
    dev, z2, loc, tri_inv, consts, b, d = _mvn_operands(z, loc, tri_inv, consts, name)
    logp, mode = _ld_out(logp, b, z.dtype, dev, name)
    _call(name, dev, z2, loc, tri_inv, consts, logp, b, d, int(family), mode, sign)
    return logp


def mvn_sample(eps, gamma, loc, tri, consts, family):
    """vcnf_mvn_sample_*: (z [B, D], log p(z) [B]) for the standard-normal draw eps [B, D] and, for the Student-t, the
    gamma draw [B] (None for the Gaussian); tri [D, D] is the scale factor L."""
    name = "vcnf_mvn_sample" + _sfx(eps)
    dev, e2, loc, tri, consts, b, d = _mvn_operands(eps, loc, tri, consts, name)
    require_device(gamma, f64=True)
    if gamma is not None:
        gamma = _batch_vector(gamma, b, eps.dtype, name, "gamma")
    z = torch.empty_like(e2)
    logp = torch.empty(b, dtype=eps.dtype, device=dev)
    _call(name, dev, e2, gamma, loc, tri, consts, z, logp, b, d, int(family))
    return z, logp


def _mvn_block_sums(dev, launch, what, like, b, d, sums):
    """``launch`` and, with ``sums``, vcnf_mvn_reduce_partials_*: (d_loc [D], d_tri [D, D], d_nu [1]), or three None."""
    outs = None
    if sums:
        outs = (torch.empty(d, dtype=like.dtype, device=like.device), torch.empty(d, d, dtype=like.dtype, device=like.device),
                torch.empty(1, dtype=like.dtype, device=like.device))
    return _block_sums(dev, launch, what, outs, (d * d + d + 1,), ("vcnf_mvn_bwd_groups", (b, d)),
                       ("vcnf_mvn_reduce_partials" + _sfx(like), (d,))) or (None, None, None)


def mvn_log_prob_bwd(z, loc, tri_inv, consts, family, g, gz_in=None, sums=True):
    """vcnf_mvn_log_prob_bwd_* and vcnf_mvn_reduce_partials_*: (dz [B, D], d_loc [D], Y = tril(sum_b c_b y_b y_b^T) [D, D]
    with zeros above the diagonal, d_nu [1]) for the cotangent g [B] of the log density; the gradient of the scale factor
    L = tri_inv^-1 is -tril(tri_inv^T (Y + strict(Y)^T)); d_nu is the part that does not go through cst,
    ``gz_in`` [B, D] is added to dz.  ``sums`` false: dz only (the three others are None), no workspace, one launch."""
    name = "vcnf_mvn_log_prob_bwd" + _sfx(z)
    dev, z2, loc, tri_inv, consts, b, d = _mvn_operands(z, loc, tri_inv, consts, name)
    require_device(g, gz_in, f64=True)
    g = _batch_vector(g, b, z.dtype, name, "g")
    if gz_in is not None:
        gz_in = _like_input(gz_in, z2, name, "gz_in", "z")
    dz = torch.empty_like(z2)
    family = int(family)
    out = _mvn_block_sums(dev, lambda ws: _launch(name, z2, loc, tri_inv, consts, g, gz_in, dz, ws, b, d, family), name,
                          z2, b, d, sums)
    return (dz,) + out


def mvn_sample_bwd(eps, gamma, tri, consts, family, g_z=None, g_lp=None, sums=True, want_eps=True):
    """vcnf_mvn_sample_bwd_* and vcnf_mvn_reduce_partials_*: (d_eps [B, D] or None, d_gamma [B] or None for the Gaussian,
    d_loc [D], d_tri [D, D], d_nu [1]) for the cotangents g_z [B, D] and g_lp [B] of vcnf_mvn_sample_*; None is zero."""
    name = "vcnf_mvn_sample_bwd" + _sfx(eps)
    dev, e2, _, tri, consts, b, d = _mvn_operands(eps, None, tri, consts, name)
    require_device(gamma, g_z, g_lp, f64=True)
    if gamma is not None:
        gamma = _batch_vector(gamma, b, eps.dtype, name, "gamma")
    if g_z is not None:
        g_z = _like_input(g_z, e2, name, "g_z", "eps")
    if g_lp is not None:
        g_lp = _batch_vector(g_lp, b, eps.dtype, name, "g_lp")
    d_eps = torch.empty_like(e2) if want_eps else None
    d_gamma = torch.empty(b, dtype=eps.dtype, device=dev) if gamma is not None else None
    family = int(family)
    out = _mvn_block_sums(dev, lambda ws: _launch(name, e2, gamma, tri, consts, g_z, g_lp, d_eps, d_gamma, ws, b, d,
                                                  family), name, e2, b, d, sums)
    return (d_eps, d_gamma) + out


def planar_radial_kinds(kinds, device):
    """(host int32 array, device int32 tensor) of a run's layer kinds: the entry points validate the host copy before
    they launch and the kernels read the device copy."""
    kinds = [int(k) for k in kinds]
    return (ctypes.c_int32 * len(kinds))(*kinds), torch.tensor(kinds, dtype=torch.int32, device=device)


def _planar_radial_operands(x, kinds, va, vb, sc, what):
    """Checked operands of vcnf_planar_radial_stack*: x [B, D], va / vb [K, D] and sc [K, 2] contiguous, of x's dtype and
    on its device.  Returns (device, x, va, vb, sc, B, D, K)."""
    dev = require_device(x, va, vb, sc, kinds[1], f64=True, allow_grad=True)
    if x.dim() != 2:
        raise VcnfError(what + ": expects [batch, features] inputs")
    b, d = x.shape
    k = len(kinds[0])
    if kinds[1].dtype != torch.int32 or tuple(kinds[1].shape) != (k,):
        raise VcnfError(what + ": kinds must be planar_radial_kinds(...) of the run")
    for name, t, shape in (("va", va, (k, d)), ("vb", vb, (k, d)), ("sc", sc, (k, 2))):
        if t.dtype != x.dtype or tuple(t.shape) != shape:
            raise VcnfError("%s: %s must be a %s tensor of shape %s" % (what, name, x.dtype, list(shape)))
    return dev, x.contiguous(), va.contiguous(), vb.contiguous(), sc.contiguous(), b, int(d), k


def planar_radial_stack(z, kinds, va, vb, sc, inverse=False, logdet=None, sign=1.0, want_trace=False):
    """vcnf_planar_radial_stack_*: a run of Planar / Radial layers over z [B, D] in one launch from the effective operands
    described in include/vcnf_hip.h (``kinds`` from planar_radial_kinds).  Returns (out, logdet) - logdet a fresh [B]
    tensor holding sign * log|det|, or the caller's with that added - and with ``want_trace`` what the VJP needs besides:
    the trace [K, B] and the row checkpoints [(K - 1) / C, B, D] (None when there is none)."""
    name = "vcnf_planar_radial_stack" + _sfx(z)
    dev, z, va, vb, sc, b, d, k = _planar_radial_operands(z.detach(), kinds, va.detach(), vb.detach(), sc.detach(), name)
    logdet, mode = _ld_out(logdet, b, z.dtype, dev, name)
    out = torch.empty_like(z)
    trace = ckpt = None
    if want_trace:
        trace = torch.empty((k, b), dtype=z.dtype, device=dev)
        n_ck = (k - 1) // max(1, int(lib().vcnf_planar_radial_checkpoint_every(d)))
        ckpt = torch.empty((n_ck, b, d), dtype=z.dtype, device=dev) if n_ck else None
    _call(name, dev, z, out, logdet, trace, ckpt, kinds[0], kinds[1], va, vb, sc, b, d, k, bool(inverse), mode, sign)
    return (out, logdet, trace, ckpt) if want_trace else (out, logdet)


def planar_radial_stack_bwd(z_out, trace, ckpt, kinds, va, vb, sc, g_out=None, g_ld=None):
    """vcnf_planar_radial_stack_bwd_*: (g_in [B, D], g_va [K, D], g_vb [K, D], g_sc [K, 2]) of the forward run for the
    cotangents g_out [B, D] and g_ld [B] of (out, log|det|); None is zero.  ``trace`` and ``ckpt`` (or None) as the forward
    run returned them.  Two launches, no atomics."""
    name = "vcnf_planar_radial_stack_bwd" + _sfx(z_out)
    dev, z_out, va, vb, sc, b, d, k = _planar_radial_operands(z_out, kinds, va, vb, sc, name)
    require_device(trace, ckpt, g_out, g_ld, f64=True, allow_grad=True)
    if ckpt is not None:
        every = int(lib().vcnf_planar_radial_checkpoint_every(d))
        if ckpt.dtype != z_out.dtype or tuple(ckpt.shape) != ((k - 1) // max(1, every), b, d) or not ckpt.is_contiguous():
            raise VcnfError(name + ": ckpt must be the contiguous checkpoint tensor of the forward run")
    if trace.dtype != z_out.dtype or tuple(trace.shape) != (k, b) or not trace.is_contiguous():
        raise VcnfError(name + ": trace must be the contiguous [layers, batch] tensor of the forward run")
    if g_out is not None:
        if g_out.dtype != z_out.dtype or g_out.shape != z_out.shape:
            raise VcnfError(name + ": g_out must be like the run's output")
        g_out = g_out.contiguous()
    if g_ld is not None:
        if g_ld.dtype != z_out.dtype or tuple(g_ld.shape) != (b,):
            raise VcnfError(name + ": g_ld must be a [batch] tensor of the run's dtype")
        g_ld = g_ld.contiguous()
    g_in = torch.empty_like(z_out)
    if b == 0:
        return g_in, torch.zeros_like(va), torch.zeros_like(vb), torch.zeros_like(sc)
    g_va, g_vb, g_sc = torch.empty_like(va), torch.empty_like(vb), torch.empty_like(sc)
    groups = int(lib().vcnf_planar_radial_bwd_groups(b, d, k))
    if groups < 1:
        _check(2, name)
    work = torch.empty((groups, k, 2 * d + 2), dtype=z_out.dtype, device=dev)
    _call(name, dev, z_out, trace, ckpt, g_out, g_ld, kinds[0], kinds[1], va, vb, sc, g_in, g_va, g_vb, g_sc, work, b, d, k)
    return g_in, g_va, g_vb, g_sc


# what ``table`` holds per family: (entries per component, least number of components); a mixture has any number of
# components, an energy's constants are one component of 1 or 4 entries.  _TABLE_FREE: families without a table.
_TABLE_FREE = (TARGET_TWO_MOONS, TARGET_SMILEY)
_TABLE_ENTRIES = {TARGET_CIRCULAR_GMM: (2, 0), TARGET_RING_MIXTURE: (1, 0), TARGET_TWO_MODES: (1, 1), TARGET_SINUSOIDAL: (1, 1),
                  TARGET_SINUSOIDAL_GAP: (1, 4), TARGET_SINUSOIDAL_SPLIT: (1, 4)}


def _target_table(name, z, dev, family, table):
    """(table detached and contiguous, n_comp) of a target entry point, (None, 0) for a family that reads no table (an
    unknown family is the entry point's to refuse)."""
    if family not in _TABLE_ENTRIES:
        return None, 0
    per, least = _TABLE_ENTRIES[family]
    if table is None or table.dtype != z.dtype or table.device != dev or table.numel() % per or table.numel() // per < least:
        raise VcnfError("%s: the %s table must be a %s tensor on %s" % (name, "constant" if least else "component", z.dtype, dev))
    return table.detach().contiguous(), table.numel() // per


def target_log_prob(z, family, table=None, scale=0.0, want_score=False):
    """vcnf_target_log_prob_*: (log density [B], score d logp / d z [B, 2] or None) of z [B, 2] under TwoMoons (family 0),
    the circular Gaussian mixture with the centres ``table`` [n, 2] (1) or the ring mixture with the radii ``table`` [n]
    (2), both of standard deviation ``scale``, or one of the energy densities of include/vcnf_hip.h of scale ``scale``:
    TwoModes with ``table`` {loc}, Sinusoidal {period}, Sinusoidal_gap / Sinusoidal_split {period, amp, mu, width}, Smiley
    (no table).  One launch; without ``want_score`` none of the score's arithmetic runs."""
    name = "vcnf_target_log_prob" + _sfx(z)
    dev = require_device(z, table, f64=True, allow_grad=True)
    if z.dtype not in (torch.float32, torch.float64):
        raise VcnfError("%s: z must be fp32 or fp64 (got %s)" % (name, z.dtype))
    if z.dim() != 2 or z.shape[1] != 2:
        raise VcnfError("%s: expects [batch, 2] inputs (got %s)" % (name, list(z.shape)))
    table, n = _target_table(name, z, dev, family, table)
    z = z.detach().contiguous()
    b = len(z)
    logp = torch.empty(b, dtype=z.dtype, device=dev)
    score = torch.empty_like(z) if want_score else None
    _call(name, dev, z, table, logp, score, b, n, int(family), float(scale))
    return logp, score


def _stochastic_target(z, family, table, name):
    """Checked (device, z, table, n_comp) of the stochastic entry points: z [B, 2] fp32 / fp64 contiguous and detached,
    the family's table like z (None for TwoMoons and Smiley)."""
    dev = require_device(z, table, f64=True, allow_grad=True)
    if z.dtype not in (torch.float32, torch.float64):
        raise VcnfError("%s: z must be fp32 or fp64 (got %s)" % (name, z.dtype))
    if z.dim() != 2 or z.shape[1] != 2:
        raise VcnfError("%s: expects [batch, 2] inputs (got %s)" % (name, list(z.shape)))
    if family not in _TABLE_FREE and family not in _TABLE_ENTRIES:
        raise VcnfError("%s: unknown target family %r" % (name, family))
    table, n = _target_table(name, z, dev, family, table)
    if table is not None and not n:
        raise VcnfError("%s: the component table must be a %s tensor on %s" % (name, z.dtype, dev))
    return dev, z.detach().contiguous(), table, n


def _stochastic_like(name, what, t, z, shape):
    """``t`` detached and contiguous after the check that it is a ``shape`` tensor of z's dtype on z's device."""
    if not torch.is_tensor(t) or t.dtype != z.dtype or t.device != z.device or tuple(t.shape) != tuple(shape):
        raise VcnfError("%s: %s must be a %s tensor of shape %s on %s" % (name, what, z.dtype, list(shape), z.device))
    return t.detach().contiguous()


def hmc_stack(z, noise, unif, step, mass, sqrt_mass, steps, family, table=None, scale=0.0, want_trace=False):
    """vcnf_hmc_stack_*: a run of K HamiltonianMonteCarlo layers of ``steps`` leapfrog steps over z [B, 2] in one launch
    against the target ``family`` (``table`` and ``scale`` as for target_log_prob), from the operands described in
    include/vcnf_hip.h: step, mass, sqrt_mass [K, 2] and the draws noise [K, B, 2], unif [K, B].  Returns (z_out, log_det)
    - log_det a fresh [B] tensor holding the sum of the layers' log p(z) - log p(z_out) - and with ``want_trace`` what
    the VJP needs besides: each layer's entrance row trace [K, B, 2] and its decision accept [K, B] (uint8)."""
    return _hmc_stack("vcnf_hmc_stack", z, noise, unif, step, mass, sqrt_mass, None, steps, family, table, scale, want_trace)


def _annealing(name, prior, z, k):
    """The checked (beta [K], prior_loc [2], prior_log_scale [2]) of an annealed run."""
    beta, loc, log_scale = prior
    return (_stochastic_like(name, "beta", beta, z, (k,)), _stochastic_like(name, "prior_loc", loc, z, (2,)),
            _stochastic_like(name, "prior_log_scale", log_scale, z, (2,)))


def hmc_annealed_stack(z, noise, unif, step, mass, sqrt_mass, beta, prior_loc, prior_log_scale, steps, family, table=None,
                       scale=0.0, want_trace=False, want_logp=False):
    """vcnf_hmc_annealed_stack_*: ``hmc_stack`` for the layers of Hamiltonian annealed importance sampling: layer k's
    density is beta[k] log p + (1 - beta[k]) log N(prior_loc, exp(prior_log_scale)^2), beta [K] and the prior's
    parameters [2] device tensors of z's dtype.  Returns what ``hmc_stack`` returns and, with ``want_logp``, as the last
    element the target's log p [B] at z_out, which the kernel carries anyway."""
    return _hmc_stack("vcnf_hmc_annealed_stack", z, noise, unif, step, mass, sqrt_mass, (beta, prior_loc, prior_log_scale),
                      steps, family, table, scale, want_trace, want_logp)


def _hmc_stack(base, z, noise, unif, step, mass, sqrt_mass, prior, steps, family, table, scale, want_trace, want_logp=False):
    """The plain (``prior`` None) or annealed forward run: one statement of the operands' checks and outputs."""
    name = base + _sfx(z)
    dev, z, table, n = _stochastic_target(z, family, table, name)
    b, steps = len(z), int(steps)
    if step.dim() != 2 or step.shape[0] < 1:
        raise VcnfError(name + ": step must be a [layers, 2] tensor")
    k = step.shape[0]
    if steps < 0:
        raise VcnfError(name + ": steps must not be negative")
    step, mass, sqrt_mass = (_stochastic_like(name, what, t, z, (k, 2))
                             for what, t in (("step", step), ("mass", mass), ("sqrt_mass", sqrt_mass)))
    noise = _stochastic_like(name, "noise", noise, z, (k, b, 2))
    unif = _stochastic_like(name, "unif", unif, z, (k, b))
    out = torch.empty_like(z)
    log_det = torch.empty(b, dtype=z.dtype, device=dev)
    trace = accept = None
    if want_trace:
        trace = torch.empty((k, b, 2), dtype=z.dtype, device=dev)
        accept = torch.empty((k, b), dtype=torch.uint8, device=dev)
    logp = torch.empty(b, dtype=z.dtype, device=dev) if want_logp else None
    extra, outs = ((), (out, log_det)) if prior is None else (_annealing(name, prior, z, k), (out, log_det, logp))
    _call(name, dev, z, noise, unif, step, mass, sqrt_mass, *extra, table, *outs, trace, accept, b, k, steps, n, int(family),
          float(scale))
    result = (out, log_det, trace, accept) if want_trace else (out, log_det)
    return result + (logp,) if want_logp else result


def hmc_stack_bwd(trace, accept, noise, step, mass, sqrt_mass, steps, family, table=None, scale=0.0, g_out=None, g_ld=None):
    """vcnf_hmc_stack_bwd_*: (g_in [B, 2], g_step [K, 2], g_mass [K, 2], g_sqrt_mass [K, 2]) of the forward run for the
    cotangents g_out [B, 2] and g_ld [B] of (z_out, log_det); None is zero.  ``trace`` and ``accept`` as the forward run
    returned them, the other operands as it took them.  The score and the decisions are constants, as in the reference.
    Two launches, no atomics."""
    return _hmc_stack_bwd("vcnf_hmc_stack_bwd", trace, accept, noise, step, mass, sqrt_mass, None, steps, family, table, scale,
                          g_out, g_ld)


def hmc_annealed_stack_bwd(trace, accept, noise, step, mass, sqrt_mass, beta, prior_loc, prior_log_scale, steps, family,
                           table=None, scale=0.0, g_out=None, g_ld=None):
    """vcnf_hmc_annealed_stack_bwd_*: ``hmc_stack_bwd`` for the annealed run; beta and the prior's parameters are
    constants and get no gradient."""
    return _hmc_stack_bwd("vcnf_hmc_annealed_stack_bwd", trace, accept, noise, step, mass, sqrt_mass,
                          (beta, prior_loc, prior_log_scale), steps, family, table, scale, g_out, g_ld)


def _hmc_stack_bwd(base, trace, accept, noise, step, mass, sqrt_mass, prior, steps, family, table, scale, g_out, g_ld):
    """The VJP of the plain (``prior`` None) or annealed run."""
    name = base + _sfx(trace)
    if trace.dim() != 3:
        raise VcnfError(name + ": trace must be the [layers, batch, 2] tensor of the forward run")
    k, b = int(trace.shape[0]), int(trace.shape[1])
    dev, z, table, n = _stochastic_target(trace.reshape(-1, 2), family, table, name)
    require_device(accept, noise, step, mass, sqrt_mass, g_out, g_ld, f64=True, allow_grad=True)
    if k < 1 or not torch.is_tensor(accept) or accept.dtype != torch.uint8 or tuple(accept.shape) != (k, b) or accept.device != dev:
        raise VcnfError(name + ": accept must be the uint8 [layers, batch] tensor of the forward run")
    step, mass, sqrt_mass = (_stochastic_like(name, what, t, z, (k, 2))
                             for what, t in (("step", step), ("mass", mass), ("sqrt_mass", sqrt_mass)))
    noise = _stochastic_like(name, "noise", noise, z, (k, b, 2))
    prior = None if prior is None else _annealing(name, prior, z, k)
    g_out = None if g_out is None else _stochastic_like(name, "g_out", g_out, z, (b, 2))
    g_ld = None if g_ld is None else _stochastic_like(name, "g_ld", g_ld, z, (b,))
    g_in = torch.empty((b, 2), dtype=z.dtype, device=dev)
    if b == 0:
        return g_in, torch.zeros_like(step), torch.zeros_like(mass), torch.zeros_like(sqrt_mass)
    g_step, g_mass, g_sqm = torch.empty_like(step), torch.empty_like(mass), torch.empty_like(sqrt_mass)
    groups = min((b + HMC_BLOCK - 1) // HMC_BLOCK, HMC_MAX_BWD_GROUPS)
    work = torch.empty((groups, k, 3, 2), dtype=z.dtype, device=dev)
    extra = () if prior is None else prior
    _call(name, dev, z, accept.contiguous(), noise, step, mass, sqrt_mass, *extra, table, g_out, g_ld, g_in, g_step, g_mass,
          g_sqm, work, b, k, int(steps), groups, n, int(family), float(scale))
    return g_in, g_step, g_mass, g_sqm


def mh_walk(z, eps, w, prop_scale, family, table=None, scale=0.0, want_accept=False):
    """vcnf_mh_walk_*: the random walk of a MetropolisHastings layer with a diagonal Gaussian proposal over z [B, 2] in
    one launch: eps [steps, B, 2] and w [steps, B] the draws, prop_scale [2] the proposal's standard deviations,
    ``family``, ``table`` and ``scale`` the target as for target_log_prob.  Returns z_out, with ``want_accept``
    (z_out, accept [steps, B] uint8).  The layer's log_det is zero and its derivative the identity: both are the
    caller's."""
    name = "vcnf_mh_walk" + _sfx(z)
    dev, z, table, n = _stochastic_target(z, family, table, name)
    b = len(z)
    if not torch.is_tensor(eps) or eps.dim() != 3:
        raise VcnfError(name + ": eps must be a [steps, batch, 2] tensor")
    steps = int(eps.shape[0])
    eps = _stochastic_like(name, "eps", eps, z, (steps, b, 2))
    w = _stochastic_like(name, "w", w, z, (steps, b))
    prop_scale = _stochastic_like(name, "prop_scale", prop_scale, z, (2,))
    out = torch.empty_like(z)
    accept = torch.empty((steps, b), dtype=torch.uint8, device=dev) if want_accept else None
    _call(name, dev, z, eps, w, prop_scale, table, out, accept, b, steps, n, int(family), float(scale))
    return (out, accept) if want_accept else out


def linear_probe(x, weight, bias, mode, relu_input=False):
    """Diagnostic (vcnf_linear_probe_f32): one dense layer evaluated with the arithmetic of one matrix path of the
    fused RQS layer kernels.  x [B, K], weight [N, K], bias [N] or None -> y [B, N]."""
    dev = require_device(x, weight, bias)
    x, weight = x.contiguous(), weight.contiguous()
    b, k = x.shape
    n = weight.shape[0]
    if weight.shape[1] != k or (bias is not None and bias.shape != (n,)):
        raise VcnfError("linear_probe: shapes %s %s" % (tuple(x.shape), tuple(weight.shape)))
    y = torch.empty(b, n, device=dev, dtype=torch.float32)
    _check(_launch("vcnf_linear_probe_f32", x, weight, bias.contiguous() if bias is not None else None, y, b, k, n,
                   int(mode), bool(relu_input), saturation_counter(dev)), "vcnf_linear_probe_f32")
    return y
