"""Masked affine autoregressive flow (MAF): every variable is scaled and shifted by parameters a MADE network
computes from the variables of lower degree.  ``forward`` is one MADE pass + one launch of the elementwise kernel
(csrc/affine_kernels.hip::maf_affine_kernel reads the MADE output [B, D * 2] in place); ``inverse`` is one launch of
csrc/made_sample.hip, which completes the MADE's hidden units degree by degree and inverts one variable between stages
(vcnf_amd/made_sample.py says which layers and calls take it); every other call runs the reference's loop of D passes.
Reference: normflow/flows/affine/autoregressive.py:11-45 (Autoregressive), :48-103 (MaskedAffineAutoregressive)."""
import numpy as np
import torch
from torch.nn import functional as F

from ..base import Flow, fold_log_det
from ... import _lib, autograd, made_sample
from ...nets.made import MADE


class Autoregressive(Flow):
    """autoregressive.py:11-45: elementwise invertible map whose parameters come from ``autoregressive_net``."""
    takes_context = True
    fuse_sampling = True        # ``inverse`` in one launch where vcnf_amd.made_sample.plan allows; False: always the loop

    def __init__(self, autoregressive_net):
        super().__init__()
        self.autoregressive_net = autoregressive_net

    def forward(self, inputs, context=None):
        return self._elementwise_forward(inputs, self.autoregressive_net(inputs, context))

    def _fused_inverse(self, inputs, context, log_q, sign):
        """(outputs, log_det) of ``inverse`` in one launch, or None: a subclass with such a kernel overrides this."""
        return None

    def _inverse_run(self, inputs, context, log_q, sign):
        """(outputs, log_det) of ``inverse``, with ``sign * log_det`` added into ``log_q`` in place where one is given."""
        fused = self._fused_inverse(inputs, context, log_q, sign)
        if fused is not None:
            return fused
        outputs = torch.zeros_like(inputs)
        logabsdet = None
        for _ in range(int(np.prod(inputs.shape[1:]))):
            outputs, logabsdet = self._elementwise_inverse(inputs, self.autoregressive_net(outputs, context))
        return fold_log_det(outputs, logabsdet, log_q, sign) if log_q is not None else (outputs, logabsdet)

    def inverse(self, inputs, context=None):
        return self._inverse_run(inputs, context, None, 1.0)

    def inverse_into(self, z, log_q, context=None):
        """``inverse`` with the log-det added into ``log_q`` (inside the kernel on the one-launch path)."""
        return self._inverse_run(z, context, log_q, 1.0)[0]

    def _output_dim_multiplier(self):
        raise NotImplementedError()

    def _elementwise_forward(self, inputs, autoregressive_params):
        raise NotImplementedError()

    def _elementwise_inverse(self, inputs, autoregressive_params):
        raise NotImplementedError()


class MaskedAffineAutoregressive(Autoregressive):
    def __init__(self, features, hidden_features, context_features=None, num_blocks=2, use_residual_blocks=True,
                 random_mask=False, activation=F.relu, dropout_probability=0., use_batch_norm=False):
        self.features = features
        made = MADE(features=features, hidden_features=hidden_features, context_features=context_features,
                    num_blocks=num_blocks, output_multiplier=self._output_dim_multiplier(),
                    use_residual_blocks=use_residual_blocks, random_mask=random_mask, activation=activation,
                    dropout_probability=dropout_probability, use_batch_norm=use_batch_norm)
        super().__init__(made)

    def _output_dim_multiplier(self):
        return 2

    def _fused_inverse(self, inputs, context, log_q, sign):
        """One launch (csrc/made_sample.hip) for the layers and calls vcnf_amd.made_sample.plan accepts.  On its first
        use a layer packs its weights and copies small tables to the device: call it once before a graph capture."""
        packed = made_sample.plan(self, inputs, context, 2)
        return None if packed is None else made_sample.run(self, packed, inputs, context, None, log_q, sign)

    def _elementwise(self, inputs, params, inverse):
        if inputs.dim() != 2 or inputs.shape[1] != self.features:
            raise ValueError('Expected inputs [B, {}], got {}.'.format(self.features, tuple(inputs.shape)))
        if autograd.needs_grad(inputs, params):
            # differentiable path: the reference's own composition (:75-89), autograd through torch ops
            p = params.view(-1, self.features, 2)
            scale = torch.sigmoid(p[..., 0] + 2.) + 1e-3
            log_scale = torch.log(scale).sum(1)
            if inverse:
                return (inputs - p[..., 1]) / scale, -log_scale
            return scale * inputs + p[..., 1], log_scale
        return _lib.maf_affine(inputs, params, inverse)

    def _elementwise_forward(self, inputs, autoregressive_params):
        return self._elementwise(inputs, autoregressive_params, False)

    def _elementwise_inverse(self, inputs, autoregressive_params):
        return self._elementwise(inputs, autoregressive_params, True)
