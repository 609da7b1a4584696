"""Base distribution end caps of the flow: the diagonal Gaussian (SURVEY 2 row 10;
normflow/distributions/base.py:609-652) and the class-conditional bases of the
reference's Glow, ClassCondDiagGaussian (:715-775) and GlowBase (:778-869), and the
GaussianMixture of normflow 1.2.  Of the heavy-tailed bases the followed fork adds, the
product Student-t (its T) and the generalised Gaussian (its GGD) are StudentT and
GeneralizedGaussian here, with one trainable tail parameter per feature, and its
full-covariance bases (its MultivariateGaussian and TMV) are MultivariateGaussian and
MultivariateStudentT, parametrised by a lower-triangular scale factor; its other
research distributions (GenNormal, ...) are out of scope.  UniformGaussian is the base
of normflow 1.2's circular models: uniform on the angles, Gaussian on the rest."""
import math

import numpy as np
import torch
from torch import nn

from .. import _lib, autograd
from ..derived import memo, tensor_key


class BaseDistribution(nn.Module):
    def forward(self, num_samples=1):
        raise NotImplementedError

    def log_prob(self, z):
        raise NotImplementedError


class DiagGaussian(BaseDistribution):
    """N(loc, diag(exp(log_scale))^2) over ``shape``; parameters [1, *shape].
    ``temperature`` T (optional) widens the scale by T, i.e. adds log T to
    log_scale (base.py:635-638)."""

    def __init__(self, shape, trainable=True):
        super().__init__()
        if isinstance(shape, int):
            shape = (shape,)
        self.shape = tuple(shape)
        self.n_dim = len(self.shape)
        self.d = int(np.prod(self.shape))
        if trainable:
            self.loc = nn.Parameter(torch.zeros(1, *self.shape))
            self.log_scale = nn.Parameter(torch.zeros(1, *self.shape))
        else:
            self.register_buffer("loc", torch.zeros(1, *self.shape))
            self.register_buffer("log_scale", torch.zeros(1, *self.shape))
        self.temperature = None

    def _flat(self):
        return self.loc.reshape(-1), self.log_scale.reshape(-1)

    def forward(self, num_samples=1):
        """Draw on the device with torch.randn, then one kernel for z and log p."""
        eps = torch.randn((num_samples,) + self.shape, dtype=self.loc.dtype, device=self.loc.device)
        return self.from_noise(eps)

    def from_noise(self, eps):
        """base.py:639-641 with the standard-normal draw supplied (parity tests
        feed the reference's captured draw; RNG streams differ across devices)."""
        loc, ls = self._flat()
        if autograd.needs_grad(eps, loc, ls):
            return autograd.DiagGaussianSampleFn.apply(eps, loc, ls, self.temperature)
        return _lib.diag_gaussian_sample(eps, loc, ls, self.temperature)

    def log_prob(self, z, out=None):
        """base.py:644-652.  ``out`` [B]: accumulate into it instead of allocating."""
        loc, ls = self._flat()
        if autograd.needs_grad(z, loc, ls, out):
            lp = autograd.DiagGaussianLogProbFn.apply(z, loc, ls, self.temperature)
            return lp if out is None else out.add_(lp)
        return _lib.diag_gaussian_log_prob(z, loc, ls, self.temperature, logp=out)

    def _torch_log_prob(self, z):
        """base.py:644-652 as the reference composes it, for the callers that serve tensors the kernels do not compute
        on (NormalizingFlowVAE off the device); ``log_prob`` itself refuses those."""
        log_scale = self.log_scale if self.temperature is None else self.log_scale + np.log(self.temperature)
        return -0.5 * self.d * np.log(2 * np.pi) - torch.sum(
            log_scale + 0.5 * torch.pow((z - self.loc) / torch.exp(log_scale), 2), list(range(1, self.n_dim + 1)))


class _ClassCondBase(BaseDistribution):
    """Shared end of the class-conditional bases: labels to kernel operands, and the calls of the
    vcnf_cc_gaussian_* kernels (csrc/class_cond_gaussian.hip) with or without autograd.  A subclass provides
    ``_tables(row_index, soft)`` -> (loc_rows, ls_rows) [R, C] and ``_pixels`` (elements per channel)."""
    takes_labels = True

    def _labels(self, y, like):
        """(row_index, soft): int32 labels [B] for the kernel's table lookup (hard labels; nothing indexes a tensor
        with them, an out-of-range label ends as NaN in the kernel), or the float matrix [B, num_classes] the
        reference takes as is."""
        if not y.is_cuda:
            raise _lib.VcnfError("vcnf_amd computes on MI355X only (labels on %s); there is no CPU path" % y.device)
        if len(y) != len(like):
            raise _lib.VcnfError("%d labels for a batch of %d" % (len(y), len(like)))
        if y.dim() == 1:
            return y.to(torch.int32).contiguous(), None
        return None, y.to(like.dtype)

    def _draw_labels(self, num_samples):
        return torch.randint(self.num_classes, (num_samples,), device=self.loc.device)

    def forward(self, num_samples=1, y=None):
        """Labels drawn with torch.randint when the distribution is class-conditional and none are given, the
        standard-normal draw with torch.randn, then one kernel for z and log p."""
        if y is not None:
            num_samples = len(y)
        eps = torch.randn((num_samples,) + self.shape, dtype=self.loc.dtype, device=self.loc.device)
        return self.from_noise(eps, y)

    def from_noise(self, eps, y=None):
        """``forward`` with the standard-normal draw supplied."""
        _lib.require_device(eps, allow_grad=True, f64=True)
        row_index, soft = self._operand_labels(eps, y, draw=True)
        loc, ls = self._tables(row_index, soft)
        if autograd.needs_grad(eps, loc, ls):
            return autograd.ClassCondGaussianSampleFn.apply(eps, loc, ls, row_index, self._pixels, self.temperature)
        return _lib.cc_gaussian_sample(eps, loc.detach(), ls.detach(), row_index, self._pixels, self.temperature)

    def log_prob(self, z, y=None, out=None):
        """``out`` [B]: accumulate into it instead of allocating."""
        _lib.require_device(z, allow_grad=True, f64=True)
        row_index, soft = self._operand_labels(z, y, draw=False)
        loc, ls = self._tables(row_index, soft)
        if autograd.needs_grad(z, loc, ls, out):
            lp = autograd.ClassCondGaussianLogProbFn.apply(z, loc, ls, row_index, self._pixels, self.temperature)
            return lp if out is None else out.add_(lp)
        return _lib.cc_gaussian_log_prob(z, loc.detach(), ls.detach(), row_index, self._pixels, self.temperature, logp=out)

    def _operand_labels(self, x, y, draw):
        if self.num_classes is None:
            return None, None
        if y is None:
            if not draw:
                raise _lib.VcnfError("%s.log_prob needs the labels y of a class-conditional base" % type(self).__name__)
            y = self._draw_labels(len(x))
        return self._labels(y, x)


class ClassCondDiagGaussian(_ClassCondBase):
    """One diagonal Gaussian over ``shape`` per class (base.py:715-775); parameters [*shape, num_classes], zeros.
    ``y``: int64 labels [B], or a float matrix [B, num_classes] whose rows mix the classes' parameters
    (loc_b = loc @ y_b).  Kernel mapping: every element is its own channel (C = d, P = 1); hard labels look their row
    up in the [num_classes, d] table inside the kernel, a float ``y`` gives one row per sample."""

    def __init__(self, shape, num_classes):
        super().__init__()
        if isinstance(shape, int):
            shape = (shape,)
        self.shape = tuple(shape)
        self.n_dim = len(self.shape)
        self.perm = [self.n_dim] + list(range(self.n_dim))
        self.d = int(np.prod(self.shape))
        self.num_classes = num_classes
        self.loc = nn.Parameter(torch.zeros(*self.shape, num_classes))
        self.log_scale = nn.Parameter(torch.zeros(*self.shape, num_classes))
        self.temperature = None
        self._pixels = 1

    def _tables(self, row_index, soft):
        loc, ls = self.loc.reshape(self.d, self.num_classes).t(), self.log_scale.reshape(self.d, self.num_classes).t()
        if soft is not None:
            return soft @ loc, soft @ ls
        return loc.contiguous(), ls.contiguous()


class GlowBase(_ClassCondBase):
    """Glow's base (base.py:778-869): per channel loc * exp(loc_logs * logscale_factor) and the same form for
    log_scale, shared by the channel's ``num_pix`` pixels, plus the class rows y_onehot @ loc_cc / log_scale_cc when
    ``num_classes`` is given.  Parameters [1, C, 1, ...] and [num_classes, C], zeros.  Kernel mapping: P = num_pix;
    hard labels look their row up in the [num_classes, C] table inside the kernel, a float ``y`` [B, num_classes] gives
    one row per sample, ``num_classes=None`` one row for all (``y`` is ignored)."""

    def __init__(self, shape, num_classes=None, logscale_factor=3.):
        super().__init__()
        if isinstance(shape, int):
            shape = (shape,)
        self.shape = tuple(shape)
        self.n_dim = len(self.shape)
        self.num_pix = int(np.prod(self.shape[1:]))
        self.d = int(np.prod(self.shape))
        self.sum_dim = list(range(1, self.n_dim + 1))
        self.num_classes = num_classes
        self.class_cond = num_classes is not None
        self.logscale_factor = logscale_factor
        per_channel = (1, self.shape[0]) + (self.n_dim - 1) * (1,)
        self.loc = nn.Parameter(torch.zeros(*per_channel))
        self.loc_logs = nn.Parameter(torch.zeros(*per_channel))
        self.log_scale = nn.Parameter(torch.zeros(*per_channel))
        self.log_scale_logs = nn.Parameter(torch.zeros(*per_channel))
        if self.class_cond:
            self.loc_cc = nn.Parameter(torch.zeros(num_classes, self.shape[0]))
            self.log_scale_cc = nn.Parameter(torch.zeros(num_classes, self.shape[0]))
        self.temperature = None
        self._pixels = self.num_pix

    def _tables(self, row_index, soft):
        loc = (self.loc * torch.exp(self.loc_logs * self.logscale_factor)).reshape(1, -1)
        ls = (self.log_scale * torch.exp(self.log_scale_logs * self.logscale_factor)).reshape(1, -1)
        if soft is not None:
            return loc + soft @ self.loc_cc, ls + soft @ self.log_scale_cc
        if row_index is not None:
            return loc + self.loc_cc, ls + self.log_scale_cc
        return loc, ls


class GaussianMixture(BaseDistribution):
    """Mixture of ``n_modes`` diagonal Gaussians over ``dim`` features (normflow 1.2 GaussianMixture).  Parameters
    (buffers with ``trainable=False``): loc, log_scale [1, n_modes, dim] and weight_scores [1, n_modes], the log of
    the normalised ``weights``; the mixture weights are softmax(weight_scores).  ``loc=None`` draws np.random.randn,
    ``scale=None`` / ``weights=None`` give ones.  Tensors are created in torch's default dtype (the reference builds
    float64 tensors from numpy arrays and its users cast the model).  Density, sampling and their gradients run on the
    vcnf_gmm_* kernels (csrc/gaussian_mixture.hip); the mode draw is a torch.multinomial on the device and carries no
    gradient."""
    MAX_TABLE = _lib.GMM_MAX_TABLE

    def __init__(self, n_modes, dim, loc=None, scale=None, weights=None, trainable=True):
        super().__init__()
        self.n_modes = n_modes
        self.dim = dim
        loc = np.random.randn(n_modes, dim) if loc is None else np.array(loc, dtype=np.float64)
        scale = np.ones((n_modes, dim)) if scale is None else np.array(scale, dtype=np.float64)
        weights = np.ones(n_modes) if weights is None else np.array(weights, dtype=np.float64)
        loc, scale, weights = loc.reshape(1, n_modes, dim), scale.reshape(1, n_modes, dim), weights.reshape(1, n_modes)
        weights = weights / weights.sum(1)
        dtype = torch.get_default_dtype()
        tensors = (("loc", torch.tensor(loc, dtype=dtype)), ("log_scale", torch.tensor(np.log(scale), dtype=dtype)),
                   ("weight_scores", torch.tensor(np.log(weights), dtype=dtype)))
        for name, t in tensors:
            if trainable:
                setattr(self, name, nn.Parameter(t))
            else:
                self.register_buffer(name, t)

    def _tables(self):
        """(loc [M, D], log_scale [M, D], log w [M]); the step from weight_scores to log w stays torch autograd."""
        if self.n_modes * self.dim > self.MAX_TABLE:
            raise NotImplementedError("GaussianMixture: n_modes * dim = %d is beyond the kernels' limit of %d table "
                                      "entries" % (self.n_modes * self.dim, self.MAX_TABLE))
        return self.loc[0], self.log_scale[0], torch.log_softmax(self.weight_scores, 1)[0]

    def forward(self, num_samples=1):
        """Modes drawn with torch.multinomial, the standard-normal draw with torch.randn, then one kernel for z and
        log p."""
        _lib.require_device(self.loc, allow_grad=True, f64=True)
        eps = torch.randn(num_samples, self.dim, dtype=self.loc.dtype, device=self.loc.device)
        return self.from_noise(eps)

    def from_noise(self, eps, mode=None):
        """``forward`` with the standard-normal draw supplied, and optionally the modes (integer tensor [B]; a mode
        outside [0, n_modes) ends as NaN in that sample's z and log p)."""
        _lib.require_device(eps, self.loc, mode, allow_grad=True, f64=True)
        loc, ls, log_w = self._tables()
        if mode is None:
            with torch.no_grad():
                mode = torch.multinomial(torch.softmax(self.weight_scores, 1)[0], len(eps), replacement=True)
        mode = mode.to(torch.int32).contiguous()
        if autograd.needs_grad(eps, loc, ls, log_w):
            return autograd.GaussianMixtureSampleFn.apply(eps, loc, ls, log_w, mode)
        return _lib.gmm_sample(eps, mode, loc.detach(), ls.detach(), log_w.detach())

    def log_prob(self, z, out=None):
        """``out`` [B]: accumulate into it instead of allocating."""
        _lib.require_device(z, self.loc, allow_grad=True, f64=True)
        loc, ls, log_w = self._tables()
        if autograd.needs_grad(z, loc, ls, log_w, out):
            lp = autograd.GaussianMixtureLogProbFn.apply(z, loc, ls, log_w)
            return lp if out is None else out.add_(lp)
        return _lib.gmm_log_prob(z, loc.detach(), ls.detach(), log_w.detach(), logp=out)


class _HeavyTailBase(BaseDistribution):
    """Shared end of the heavy-tailed product bases: location-scale families over ``shape`` with one tail parameter per
    feature, u = (z - loc) / exp(log_scale) and a density cst - log_scale + f(u; tail) per feature.  Density, sampling
    and their gradients run on the vcnf_tail_* kernels (csrc/heavy_tail.hip).  Everything of size [D] stays in torch:
    a subclass gives ``_tail_rows()`` -> (tail row, normaliser row cst, gamma concentration), all functions of its log
    tail parameter, and autograd carries the kernels' row gradients through them.  cst is computed in fp64 whatever the
    module's dtype (in fp32 its lgamma terms cancel), then cast.  The random draws are torch's - a standard normal and a
    gamma per element - and the kernels only transform them; the gamma draw is taken with autograd on, so torch's
    implicit derivative carries the pathwise gradient to the tail parameter."""
    _family = None
    _tail = None          # name of the log tail parameter

    def __init__(self, shape, tail, trainable):
        super().__init__()
        if isinstance(shape, int):
            shape = (shape,)
        self.shape = tuple(shape)
        self.n_dim = len(self.shape)
        self.d = int(np.prod(self.shape))
        tail = np.broadcast_to(np.asarray(tail, dtype=np.float64), self.shape)
        if not (tail > 0).all():
            raise ValueError("%s: the tail parameter must be positive" % type(self).__name__)
        dtype = torch.get_default_dtype()
        tensors = (("loc", torch.zeros(1, *self.shape, dtype=dtype)), ("log_scale", torch.zeros(1, *self.shape, dtype=dtype)),
                   (self._tail, torch.tensor(np.log(tail), dtype=dtype).reshape(1, *self.shape)))
        for name, t in tensors:
            if trainable:
                setattr(self, name, nn.Parameter(t))
            else:
                self.register_buffer(name, t)

    def _rows(self):
        """(loc, log_scale, tail, cst [D], gamma concentration [1, *shape])"""
        tail, cst, conc = self._tail_rows(getattr(self, self._tail))
        return self.loc.reshape(-1), self.log_scale.reshape(-1), tail.reshape(-1), cst.to(tail.dtype).reshape(-1), conc

    def forward(self, num_samples=1):
        """Both draws on the device with torch, then one kernel for z and log p."""
        _lib.require_device(self.loc, allow_grad=True, f64=True)
        eps = torch.randn((num_samples,) + self.shape, dtype=self.loc.dtype, device=self.loc.device)
        return self.from_noise(eps)

    def from_noise(self, eps, gamma=None):
        """``forward`` with the standard-normal draw supplied, and optionally the gamma draw (like eps)."""
        _lib.require_device(eps, self.loc, gamma, allow_grad=True, f64=True)
        loc, ls, tail, cst, conc = self._rows()
        if gamma is None:
            gamma = torch._standard_gamma(conc.expand(eps.shape))
        if autograd.needs_grad(eps, gamma, loc, ls, tail, cst):
            return autograd.HeavyTailSampleFn.apply(eps, gamma, loc, ls, tail, cst, self._family)
        return _lib.tail_sample(eps, gamma, loc, ls, tail, cst, self._family)

    def log_prob(self, z, out=None):
        """``out`` [B]: accumulate into it instead of allocating."""
        _lib.require_device(z, self.loc, allow_grad=True, f64=True)
        loc, ls, tail, cst, _ = self._rows()
        if autograd.needs_grad(z, loc, ls, tail, cst, out):
            lp = autograd.HeavyTailLogProbFn.apply(z, loc, ls, tail, cst, self._family)
            return lp if out is None else out.add_(lp)
        return _lib.tail_log_prob(z, loc.detach(), ls.detach(), tail.detach(), cst.detach(), self._family, logp=out)


class StudentT(_HeavyTailBase):
    """Product of Student-t factors over ``shape``: per feature lgamma((nu+1)/2) - lgamma(nu/2) - log(nu pi)/2 -
    log_scale - (nu+1)/2 log1p(u^2/nu).  Parameters (buffers with ``trainable=False``) loc, log_scale, log_df
    [1, *shape] with nu = exp(log_df); zeros, zeros, log(df), ``df`` a float or an array of ``shape``.  Sampling:
    u = eps sqrt(nu / (2 gamma)) with eps ~ N(0, 1) and gamma ~ Gamma(nu/2, 1)."""
    _family = _lib.TAIL_STUDENT_T
    _tail = "log_df"

    def __init__(self, shape, df=3.0, trainable=True):
        super().__init__(shape, df, trainable)

    def _tail_rows(self, log_df):
        nu = torch.exp(log_df)
        l64 = log_df.double()
        n64 = torch.exp(l64)
        cst = torch.lgamma(0.5 * (n64 + 1.0)) - torch.lgamma(0.5 * n64) - 0.5 * (l64 + math.log(math.pi))
        return nu, cst, 0.5 * nu


class GeneralizedGaussian(_HeavyTailBase):
    """Product of generalised Gaussian factors over ``shape``: per feature log(beta) - log 2 - lgamma(1/beta) -
    log_scale - |u|^beta; beta = 2 is a Gaussian of scale exp(log_scale) / sqrt 2, beta = 1 is Laplace.  Parameters
    (buffers with ``trainable=False``) loc, log_scale, log_beta [1, *shape]; zeros, zeros, log(beta), ``beta`` a float or
    an array of ``shape``.  At u == 0 the gradients of |u|^beta with respect to u and beta are 0 for every beta (for
    beta < 1 a convention: the derivative is unbounded there).  Sampling: u = sign(eps) gamma^(1/beta) with
    gamma ~ Gamma(1/beta, 1), so |u|^beta is gamma itself."""
    _family = _lib.TAIL_GEN_GAUSSIAN
    _tail = "log_beta"

    def __init__(self, shape, beta=2.0, trainable=True):
        super().__init__(shape, beta, trainable)

    def _tail_rows(self, log_beta):
        beta = torch.exp(log_beta)
        l64 = log_beta.double()
        cst = l64 - math.log(2.0) - torch.lgamma(torch.exp(-l64))
        return beta, cst, 1.0 / beta


class _FullCovarianceBase(BaseDistribution):
    """Shared end of the full-covariance bases over ``n_dim`` features: z = loc + s L eps with the lower-triangular
    L = tril(lower, -1) + diag(exp(log_diag)), and a density cst + f(q), q = |L^-1 (z - loc)|^2.  Density, sampling and
    their gradients run on the vcnf_mvn_* kernels (csrc/mvn_base.hip).  Everything of size [D, D] or smaller stays in
    torch: building L and the scalar cst = normaliser - sum log_diag (fp64) with autograd, and the inverse of L (one
    triangular solve against the identity, in fp64 whatever the module's dtype, cast once; computed afresh on every
    call), whose gradient autograd.MultivariateLogProbFn hands to L in closed form.  The kernels never solve and never
    call lgamma.  Parameters (buffers with ``trainable=False``): loc, log_diag
    [1, D] and lower [D, D], of which only the strictly lower triangle is ever used: the rest is created zero, never
    read, and receives exactly zero gradient."""
    _family = None
    MAX_DIM = _lib.MVN_MAX_DIM

    def __init__(self, n_dim, loc, scale_tril, trainable, extra=()):
        super().__init__()
        self.n_dim = self.d = int(n_dim)
        self.shape = (self.d,)
        d = self.d
        loc = np.zeros(d) if loc is None else np.array(loc, dtype=np.float64).reshape(-1)
        tril = np.eye(d) if scale_tril is None else np.array(scale_tril, dtype=np.float64)
        name = type(self).__name__
        if loc.shape != (d,):
            raise ValueError("%s: loc must have %d elements" % (name, d))
        if tril.shape != (d, d) or np.any(np.triu(tril, 1) != 0) or not (np.diagonal(tril) > 0).all():
            raise ValueError("%s: scale_tril must be [%d, %d] with a zero upper triangle and a positive diagonal" % (name, d, d))
        dtype = torch.get_default_dtype()
        tensors = (("loc", torch.tensor(loc, dtype=dtype).reshape(1, d)),
                   ("log_diag", torch.tensor(np.log(np.diagonal(tril)), dtype=dtype).reshape(1, d)),
                   ("lower", torch.tensor(np.tril(tril, -1), dtype=dtype))) + tuple(extra)
        for key, t in tensors:
            if trainable:
                setattr(self, key, nn.Parameter(t))
            else:
                self.register_buffer(key, t)

    @property
    def scale_tril(self):
        """L = tril(lower, -1) + diag(exp(log_diag))"""
        return torch.tril(self.lower, -1) + torch.diag(torch.exp(self.log_diag[0]))

    def _check_dim(self):
        if self.d > self.MAX_DIM:
            raise NotImplementedError("%s: n_dim = %d is beyond the kernels' limit of %d features"
                                      % (type(self).__name__, self.d, self.MAX_DIM))

    def _consts(self):
        """consts [2] = (cst, nu) in the module's dtype, cst evaluated in fp64"""
        norm, nu = self._normaliser()
        cst = norm - self.log_diag.double().sum()
        return torch.stack([cst.reshape(()), nu.double().reshape(())]).to(self.loc.dtype)

    def _inverse(self, tri):
        eye = torch.eye(self.d, dtype=torch.float64, device=tri.device)
        return torch.linalg.solve_triangular(tri.double(), eye, upper=False).to(tri.dtype)

    def _gamma(self, num_samples):
        return None

    def forward(self, num_samples=1):
        """The draws on the device with torch, then one kernel for z and log p."""
        self._check_dim()
        _lib.require_device(self.loc, allow_grad=True, f64=True)
        eps = torch.randn(num_samples, self.d, dtype=self.loc.dtype, device=self.loc.device)
        return self.from_noise(eps)

    def _from_noise(self, eps, gamma):
        self._check_dim()
        _lib.require_device(eps, self.loc, gamma, allow_grad=True, f64=True)
        if gamma is None:
            gamma = self._gamma(len(eps))
        loc, tri, consts = self.loc.reshape(-1), self.scale_tril, self._consts()
        if autograd.needs_grad(eps, gamma, loc, tri, consts):
            return autograd.MultivariateSampleFn.apply(eps, gamma, loc, tri, consts, self._family)
        return _lib.mvn_sample(eps, gamma, loc, tri, consts, self._family)

    def log_prob(self, z, out=None):
        """``out`` [B]: accumulate into it instead of allocating."""
        self._check_dim()
        _lib.require_device(z, self.loc, allow_grad=True, f64=True)
        loc, tri, consts = self.loc.reshape(-1), self.scale_tril, self._consts()
        with torch.no_grad():
            tri_inv = self._inverse(tri)
        if autograd.needs_grad(z, loc, tri, consts, out):
            lp = autograd.MultivariateLogProbFn.apply(z, loc, tri, tri_inv, consts, self._family)
            return lp if out is None else out.add_(lp)
        return _lib.mvn_log_prob(z, loc.detach(), tri_inv, consts.detach(), self._family, logp=out)


class MultivariateGaussian(_FullCovarianceBase):
    """N(loc, L L^T) over ``n_dim`` <= 128 features: log p = -D/2 log 2 pi - sum log_diag - |L^-1 (z - loc)|^2 / 2, sampling
    z = loc + L eps.  ``loc=None`` gives zeros, ``scale_tril=None`` the identity; a given ``scale_tril`` [D, D] must have
    a zero upper triangle and a positive diagonal.  state_dict: loc, log_diag [1, D], lower [D, D]."""
    _family = _lib.MVN_GAUSSIAN

    def __init__(self, n_dim, loc=None, scale_tril=None, trainable=True):
        super().__init__(n_dim, loc, scale_tril, trainable)

    def _normaliser(self):
        z = torch.zeros((), dtype=torch.float64, device=self.loc.device)
        return z - 0.5 * self.d * math.log(2.0 * math.pi), z

    def from_noise(self, eps):
        """``forward`` with the standard-normal draw eps [B, D] supplied."""
        return self._from_noise(eps, None)


class MultivariateStudentT(_FullCovarianceBase):
    """Multivariate Student-t over ``n_dim`` <= 128 features with nu = exp(log_df) degrees of freedom, location loc and
    scale factor L: log p = lgamma((nu+D)/2) - lgamma(nu/2) - D/2 log(nu pi) - sum log_diag - (nu+D)/2 log1p(q/nu),
    q = |L^-1 (z - loc)|^2.  Sampling: z = loc + s L eps with s = sqrt(nu / (2 gamma)) and one gamma ~ Gamma(nu/2, 1)
    per sample; the density of a draw uses q = s^2 |eps|^2 directly.  The gamma draw is taken with autograd on, so
    torch's implicit derivative carries the pathwise gradient to log_df.  state_dict: loc, log_diag [1, D], lower
    [D, D], log_df [1]."""
    _family = _lib.MVN_STUDENT_T

    def __init__(self, n_dim, df=3.0, loc=None, scale_tril=None, trainable=True):
        df = float(df)
        if not df > 0:
            raise ValueError("MultivariateStudentT: df must be positive")
        super().__init__(n_dim, loc, scale_tril, trainable,
                         extra=(("log_df", torch.tensor([math.log(df)], dtype=torch.get_default_dtype())),))

    def _normaliser(self):
        l64 = self.log_df.double()[0]
        nu = torch.exp(l64)
        norm = torch.lgamma(0.5 * (nu + self.d)) - torch.lgamma(0.5 * nu) - 0.5 * self.d * (l64 + math.log(math.pi))
        return norm, nu

    def _gamma(self, num_samples):
        return torch._standard_gamma((0.5 * torch.exp(self.log_df)).expand(num_samples))

    def from_noise(self, eps, gamma=None):
        """``forward`` with the standard-normal draw eps [B, D] supplied, and optionally the gamma draw [B]."""
        return self._from_noise(eps, gamma)


class UniformGaussian(BaseDistribution):
    """Uniform on the columns ``ind`` and Gaussian on the others (normflow 1.2 base.py UniformGaussian): the base of a
    flow whose coordinates ``ind`` are angles.  ``scale`` [ndim] (ones when None) is the width of the uniform columns -
    for an angle the whole period, 2 bound - and the standard deviation of the Gaussian ones; it is a buffer, as are
    ``ind``, ``ind_`` (the other indices, ascending) and ``inv_perm`` (the inverse of cat(ind, ind_)), all int64.
    log p = -sum log scale - (ndim - len(ind)) / 2 log 2 pi - sum over ind_ of (z / scale)^2 / 2; the uniform part does not
    test its range, so a point outside it gets no -inf.

    Density, sampling and the gradient of the density run on the vcnf_uniform_gaussian_* kernels (csrc/periodic.hip),
    one launch each, from per-column tables that are derived buffers; the constant of the density is evaluated on the
    host in fp64.  The draws are torch's, in the reference's order (the uniform columns, then the Gaussian ones).  CPU
    tensors, half precision, inputs that are not [B, ndim] of the scale's dtype and a draw that requires grad evaluate
    the reference's composition in torch."""

    def __init__(self, ndim, ind, scale=None):
        super().__init__()
        self.ndim = ndim
        if isinstance(ind, int):
            ind = [ind]
        self.register_buffer("ind", ind.to(torch.long) if torch.is_tensor(ind) else torch.tensor(ind, dtype=torch.long))
        taken = set(self.ind.tolist())
        self.register_buffer("ind_", torch.tensor([i for i in range(ndim) if i not in taken], dtype=torch.long))
        perm = torch.cat((self.ind, self.ind_))
        inv_perm = torch.zeros_like(perm)
        inv_perm[perm] = torch.arange(ndim)
        self.register_buffer("inv_perm", inv_perm)
        self.register_buffer("scale", torch.ones(ndim) if scale is None else scale)

    def _build_tables(self):
        """(inv_scale_g, scale, src, offset, const_term): 1 / scale on the Gaussian columns and 0 on the uniform ones,
        the scale, the source column of each output column as int32, 0.5 where that source is a uniform draw, and the
        density's constant as a Python float from fp64 arithmetic."""
        scale, device, dtype = self.scale, self.scale.device, self.scale.dtype
        s64 = scale.detach().double().cpu().reshape(-1)
        inv = torch.zeros(self.ndim, dtype=torch.float64)
        gauss = self.ind_.cpu()
        inv[gauss] = 1.0 / s64[gauss]
        const_term = float(-torch.log(s64).sum()) - 0.5 * len(gauss) * math.log(2.0 * math.pi)
        src = self.inv_perm.cpu()
        offset = torch.where(src < len(self.ind), 0.5, 0.0)
        return (inv.to(device=device, dtype=dtype), scale.detach().reshape(-1).contiguous(),
                src.to(device=device, dtype=torch.int32), offset.to(device=device, dtype=dtype), const_term)

    def _tables(self):
        key = tensor_key((self.scale, self.ind, self.ind_, self.inv_perm)) + (self.scale.dtype,)
        return memo(self, 'uniform_gaussian_tables', key, UniformGaussian._build_tables, 4)

    def _on_kernels(self, z):
        return z.is_cuda and z.dtype in (torch.float32, torch.float64) and z.dtype == self.scale.dtype and \
            z.device == self.scale.device and z.dim() == 2 and z.shape[1] == self.ndim and self.ndim >= 1

    def forward(self, num_samples=1):
        """The two draws in the reference's order, joined, then one kernel for z and log p."""
        like = dict(dtype=self.scale.dtype, device=self.scale.device)
        eps = torch.cat((torch.rand((num_samples, len(self.ind)), **like),
                         torch.randn((num_samples, len(self.ind_)), **like)), -1)
        return self.from_noise(eps)

    def sample(self, num_samples=1):
        return self.forward(num_samples)[0]

    def from_noise(self, eps):
        """``forward`` with the draws eps [B, ndim] supplied in the order drawn: the first len(ind) columns uniform on
        [0, 1), the rest standard normal."""
        if self._on_kernels(eps) and not autograd.needs_grad(eps):
            inv, scale, src, offset, const_term = self._tables()
            return _lib.uniform_gaussian_sample(eps, src, offset, scale, const_term, inv)
        k = len(self.ind)
        z = self.scale * torch.cat((eps[..., :k] - 0.5, eps[..., k:]), -1)[..., self.inv_perm]
        return z, self._torch_log_prob(z)

    def log_prob(self, z, out=None):
        """``out`` [B]: accumulate into it instead of allocating."""
        if not self._on_kernels(z):
            lp = self._torch_log_prob(z)
            return lp if out is None else out.add_(lp)
        inv, _, _, _, const_term = self._tables()
        if autograd.needs_grad(z, out):
            lp = autograd.UniformGaussianLogProbFn.apply(z, inv, const_term)
            return lp if out is None else out.add_(lp)
        return _lib.uniform_gaussian_log_prob(z, inv, const_term, logp=out)

    def _torch_log_prob(self, z):
        """The density as the reference composes it."""
        log_p_u = torch.broadcast_to(-torch.log(self.scale[self.ind]), (len(z), -1))
        log_p_g = -0.5 * np.log(2 * np.pi) - torch.log(self.scale[self.ind_]) \
            - 0.5 * torch.pow(z[..., self.ind_] / self.scale[self.ind_], 2)
        return torch.sum(log_p_u, -1) + torch.sum(log_p_g, -1)
