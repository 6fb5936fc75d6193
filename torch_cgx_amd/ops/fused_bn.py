"""BatchNorm2d fused with the residual add and ReLU that follow it.

``bn_act(bn, x, identity, relu)`` computes ``relu(bn(x) + identity)``.  For a
channels_last bf16 CUDA activation in training mode it runs the native NHWC
kernels (csrc/bn_kernels.hip): one statistics pass, one apply pass that also
adds, clamps and records the ReLU mask as one bit per element, and a backward
of one reduce pass and one dx pass.  In every other case it executes the
stock composition, module call by module call.

``CGX_FUSED_BN=0`` switches the native path off.
"""

from __future__ import annotations

import os

import torch
import torch.nn.functional as F

from .. import _C


class _BnAct(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, identity, weight, bias, running_mean, running_var,
                momentum, eps, relu):
        out, mean, invstd, mask = _C.bn_act_forward(
            x, identity, weight, bias, running_mean, running_var, momentum,
            eps, relu)
        ctx.save_for_backward(x, mean, invstd, weight, mask)
        ctx.has_identity = identity is not None
        return out

    @staticmethod
    def backward(ctx, dy):
        x, mean, invstd, weight, mask = ctx.saved_tensors
        dx, dgamma, dbeta, didentity = _C.bn_act_backward(
            dy, x, mean, invstd, weight, mask, ctx.has_identity)
        return (dx, didentity, dgamma, dbeta, None, None, None, None, None)


def fused_bn_enabled() -> bool:
    return os.environ.get("CGX_FUSED_BN", "1") != "0"


def _native(bn, x, identity) -> bool:
    if not (bn.training and bn.track_running_stats
            and bn.momentum is not None and fused_bn_enabled()):
        return False
    if bn.weight is None or bn.bias is None:
        return False
    if not (x.is_cuda and _C.bn_eligible(x)):
        return False
    if identity is not None and not (
            identity.shape == x.shape and identity.device == x.device
            and _C.bn_eligible(identity)):
        return False
    return bn.weight.dtype == torch.float32


def bn_act(bn: torch.nn.BatchNorm2d, x: torch.Tensor,
           identity: torch.Tensor = None, relu: bool = True) -> torch.Tensor:
    """``relu(bn(x) + identity)``; ``identity`` and ``relu`` are optional."""
    if _native(bn, x, identity):
        bn.num_batches_tracked.add_(1)
        return _BnAct.apply(x, identity, bn.weight, bn.bias, bn.running_mean,
                            bn.running_var, bn.momentum, bn.eps, relu)
    out = bn(x)
    if identity is not None:
        out = out + identity
    if relu:
        out = F.relu(out, inplace=True)
    return out
