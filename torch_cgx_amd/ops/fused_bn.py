"""BatchNorm2d fused with what follows it in a ResNet.

``bn_act(bn, x, identity, relu)`` computes ``relu(bn(x) + identity)``.  For a
channels_last bf16 CUDA activation in training mode it runs the native NHWC
kernels (csrc/bn_kernels.hip): one statistics pass, one apply pass that also
adds, clamps and records the ReLU mask as one bit per element, and a backward
of one reduce pass and one dx pass.  In every other case it executes the
stock composition, module call by module call.

``bn_act(bn, x, identity, relu, identity_bn=bn_d)`` computes
``relu(bn(x) + bn_d(identity))``, the join of a downsampling bottleneck:
``identity`` is then the raw output of the downsample convolution.  Natively
the normalised identity and its gradient never go through memory: the apply
pass reads both raw tensors, the backward's reduce pass sums for both
BatchNorms at once and its dx pass writes both input gradients.

``bn_act_pool(bn, x, pool)`` computes ``pool(relu(bn(x)))``, the stem.  For a
3x3 / stride 2 / padding 1 max-pool the native path writes only the pooled
tensor and one byte per pooled element (which of the nine window positions
won), and the backward builds each pixel's gradient from those.

``CGX_FUSED_BN=0`` switches the native paths off.
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


class _BnActJoin(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, xd, weight, bias, running_mean, running_var, momentum,
                eps, weightd, biasd, running_meand, running_vard, momentumd,
                epsd, relu):
        out, mean, invstd, meand, invstdd, mask = _C.bn_act2_forward(
            x, xd, weight, bias, running_mean, running_var, momentum, eps,
            weightd, biasd, running_meand, running_vard, momentumd, epsd, relu)
        ctx.save_for_backward(x, xd, mean, invstd, weight, meand, invstdd,
                              weightd, mask)
        return out

    @staticmethod
    def backward(ctx, dy):
        (x, xd, mean, invstd, weight, meand, invstdd, weightd,
         mask) = ctx.saved_tensors
        dx, dxd, dgamma, dbeta, dgammad, dbetad = _C.bn_act2_backward(
            dy, x, xd, mean, invstd, weight, meand, invstdd, weightd, mask)
        return (dx, dxd, dgamma, dbeta, None, None, None, None, dgammad,
                dbetad, None, None, None, None, None)


class _BnActPool(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, running_mean, running_var, momentum,
                eps):
        out, mean, invstd, arg = _C.bn_act_pool_forward(
            x, weight, bias, running_mean, running_var, momentum, eps)
        ctx.save_for_backward(x, mean, invstd, weight, arg)
        return out

    @staticmethod
    def backward(ctx, dy):
        x, mean, invstd, weight, arg = ctx.saved_tensors
        dx, dgamma, dbeta = _C.bn_act_pool_backward(dy, x, mean, invstd,
                                                    weight, arg)
        return (dx, dgamma, dbeta, None, None, None, None)


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


def _bn_args(bn):
    return (bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.momentum,
            bn.eps)


def bn_act(bn: torch.nn.BatchNorm2d, x: torch.Tensor,
           identity: torch.Tensor = None, relu: bool = True,
           identity_bn: torch.nn.BatchNorm2d = None) -> torch.Tensor:
    """``relu(bn(x) + identity)``; ``identity`` and ``relu`` are optional.
    With ``identity_bn`` it is ``relu(bn(x) + identity_bn(identity))``."""
    if identity_bn is not None:
        if _native(bn, x, identity) and _native(identity_bn, identity, x):
            bn.num_batches_tracked.add_(1)
            identity_bn.num_batches_tracked.add_(1)
            return _BnActJoin.apply(x, identity, *_bn_args(bn),
                                    *_bn_args(identity_bn), relu)
        out = bn(x) + identity_bn(identity)
        return F.relu(out, inplace=True) if relu else out
    if _native(bn, x, identity):
        bn.num_batches_tracked.add_(1)
        return _BnAct.apply(x, identity, *_bn_args(bn), relu)
    out = bn(x)
    if identity is not None:
        out = out + identity
    if relu:
        out = F.relu(out, inplace=True)
    return out


def _pool_is_3x3_s2_p1(pool) -> bool:
    def pair(v):
        return tuple(v) if isinstance(v, (tuple, list)) else (v, v)

    return (type(pool) is torch.nn.MaxPool2d
            and pair(pool.kernel_size) == (3, 3) and pair(pool.stride) == (2, 2)
            and pair(pool.padding) == (1, 1) and pair(pool.dilation) == (1, 1)
            and not pool.ceil_mode and not pool.return_indices)


def bn_act_pool(bn: torch.nn.BatchNorm2d, x: torch.Tensor,
                pool: torch.nn.Module) -> torch.Tensor:
    """``pool(relu(bn(x)))``."""
    if _pool_is_3x3_s2_p1(pool) and _native(bn, x, None):
        bn.num_batches_tracked.add_(1)
        return _BnActPool.apply(x, *_bn_args(bn))
    return pool(bn_act(bn, x))
