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

``conv_bn_act(conv, bn, x, ...)`` is ``bn_act(bn, conv(x), ...)``.  Where
``conv`` is a 1x1 / stride 1 convolution at a shape the plan
(csrc/conv1x1_plan.cc) has measured faster, the native GEMM kernel
(csrc/conv1x1_kernels.hip) computes it and hands the BatchNorm the
per-channel partial statistics of its output, so the statistics pass over
that output is skipped.  ``identity_conv`` does the same for the downsample
convolution of a join.  ``CGX_NATIVE_CONV1X1=0`` switches this off,
``CGX_NATIVE_CONV1X1=all`` takes every shape the kernel accepts, measured
faster or not.

The input gradient of such a convolution is the same GEMM with the roles of
its channels exchanged (``_C.conv1x1_bwd_data``), taken where its own table
in the plan has measured it faster than the stock backward-data.
``conv_bn_act_fork`` is ``conv_bn_act`` at the input of a residual block: it
also returns the tensor the skip path continues from, and the gradient
arriving over that path is then added in the GEMM's epilogue, not by
autograd in a pass of its own.
``CGX_NATIVE_CONV1X1_BWD=0|1|all`` works like the forward switch and is off
wherever that one is.

The weight gradient is the third GEMM, ``dW = dY^T X`` with the rows
contracted (``_C.conv1x1_wrw``): a split over the rows whose fp32 partials a
second kernel sums in a fixed order, so it gives the same bits every run.  It
too is taken where its own table has measured it faster than the stock
weight gradient; ``CGX_NATIVE_CONV1X1_WRW=0|1|all`` is its switch, off
wherever the forward switch is.

``CGX_FUSED_BN=0`` switches all native paths off.
"""

from __future__ import annotations

import os

import torch
import torch.nn.functional as F

from .. import _C


class _BnAct(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, identity, weight, bias, running_mean, running_var,
                momentum, eps, relu, part):
        out, mean, invstd, mask = _C.bn_act_forward(
            x, identity, weight, bias, running_mean, running_var, momentum,
            eps, relu, part)
        ctx.save_for_backward(x, mean, invstd, weight, mask)
        ctx.has_identity = identity is not None
        return out

    @staticmethod
    def backward(ctx, dy):
        x, mean, invstd, weight, mask = ctx.saved_tensors
        dx, dgamma, dbeta, didentity = _C.bn_act_backward(
            dy, x, mean, invstd, weight, mask, ctx.has_identity)
        return (dx, didentity, dgamma, dbeta, None, None, None, None, None,
                None)


class _BnActJoin(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, xd, weight, bias, running_mean, running_var, momentum,
                eps, weightd, biasd, running_meand, running_vard, momentumd,
                epsd, relu, part, partd):
        out, mean, invstd, meand, invstdd, mask = _C.bn_act2_forward(
            x, xd, weight, bias, running_mean, running_var, momentum, eps,
            weightd, biasd, running_meand, running_vard, momentumd, epsd, relu,
            part, partd)
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
                dbetad, None, None, None, None, None, None, None)


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
           identity_bn: torch.nn.BatchNorm2d = None,
           part: torch.Tensor = None,
           identity_part: torch.Tensor = None) -> torch.Tensor:
    """``relu(bn(x) + identity)``; ``identity`` and ``relu`` are optional.
    With ``identity_bn`` it is ``relu(bn(x) + identity_bn(identity))``.
    ``part`` / ``identity_part`` are the statistics partials that came with
    ``x`` / ``identity`` from the native 1x1 convolution, if it produced
    them."""
    if identity_bn is not None:
        if _native(bn, x, identity) and _native(identity_bn, identity, x):
            bn.num_batches_tracked.add_(1)
            identity_bn.num_batches_tracked.add_(1)
            return _BnActJoin.apply(x, identity, *_bn_args(bn),
                                    *_bn_args(identity_bn), relu, part,
                                    identity_part)
        out = bn(x) + identity_bn(identity)
        return F.relu(out, inplace=True) if relu else out
    if _native(bn, x, identity):
        bn.num_batches_tracked.add_(1)
        return _BnAct.apply(x, identity, *_bn_args(bn), relu, part)
    out = bn(x)
    if identity is not None:
        out = out + identity
    if relu:
        out = F.relu(out, inplace=True)
    return out


class _Conv1x1Stats(torch.autograd.Function):
    """The 1x1 convolution and the BatchNorm partials of its output; the
    backward is the stock convolution backward on the same operands, but for
    the weight gradient where the native one is taken."""

    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda", cast_inputs=torch.bfloat16)
    def forward(ctx, x, weight):
        y, part = _C.conv1x1_stats(x, weight)
        ctx.save_for_backward(x, weight)
        ctx.mark_non_differentiable(part)
        return y, part

    @staticmethod
    @torch.amp.custom_bwd(device_type="cuda")
    def backward(ctx, dy, _dpart):
        x, weight = ctx.saved_tensors
        need_dx, need_dw = ctx.needs_input_grad[:2]
        if need_dw and _conv1x1_dw_native(dy, x):
            dw = _conv1x1_dw(dy, x, weight)
            dx = None
            if need_dx:
                dx = _conv1x1_backward(dy, x, weight, (True, False, False))[0]
            return dx, dw
        dx, dw, _ = _conv1x1_backward(dy, x, weight, (need_dx, need_dw, False))
        return dx, dw


class _Conv1x1Fork(torch.autograd.Function):
    """``(y, part, skip) = f(x, weight)``: the 1x1 convolution, native with
    partials or stock with ``part`` None as ``native_fwd`` says, and with
    ``fork`` its input once more as ``skip``, for the residual path to go on
    from.  The backward then receives the gradients of both at once, and the
    native backward-data GEMM adds the skip gradient in its epilogue instead
    of autograd in a pass of its own."""

    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda", cast_inputs=torch.bfloat16)
    def forward(ctx, x, weight, native_fwd, fork):
        if native_fwd:
            y, part = _C.conv1x1_stats(x, weight)
            ctx.mark_non_differentiable(part)
        else:
            y, part = F.conv2d(x, weight), None
        ctx.save_for_backward(x, weight)
        # an unused output arrives as None, not as a tensor of zeros to add
        ctx.set_materialize_grads(False)
        return y, part, (x.view_as(x) if fork else None)

    @staticmethod
    @torch.amp.custom_bwd(device_type="cuda")
    def backward(ctx, dy, _dpart, dskip):
        x, weight = ctx.saved_tensors
        dx = dw = None
        if dy is not None and ctx.needs_input_grad[1]:
            dw = _conv1x1_dw(dy, x, weight)
        if ctx.needs_input_grad[0]:
            dx = dskip if dy is None else _conv1x1_dx(dy, x, weight, dskip)
        return dx, dw, None, None


def _conv1x1_backward(dy, x, weight, mask):
    return torch.ops.aten.convolution_backward(
        dy, x, weight, None, (1, 1), (0, 0), (1, 1), False, (0, 0), 1, mask)


def _conv1x1_dw_native(dy, x) -> bool:
    mode = native_conv1x1_wrw_mode()
    if mode == "0" or not _C.conv1x1_wrw_eligible(dy, x):
        return False
    plan = _C.conv1x1_wrw_plan(x.numel() // x.shape[1], x.shape[1],
                               dy.shape[1])
    return plan["native"] or mode == "all"


def _conv1x1_dw(dy, x, weight):
    """The weight gradient: the native GEMM where the plan has measured it
    faster, else the stock one."""
    if _conv1x1_dw_native(dy, x):
        return _C.conv1x1_wrw(dy, x)
    return _conv1x1_backward(dy, x, weight, (False, True, False))[1]


def _conv1x1_dx(dy, x, weight, dskip):
    """The input gradient plus ``dskip`` (or None): one native GEMM where the
    plan has measured it faster, else the stock backward-data and a ``+``."""
    mode = native_conv1x1_bwd_mode()
    if mode != "0" and _C.conv1x1_bwd_eligible(dy, weight, dskip):
        plan = _C.conv1x1_bwd_plan(x.numel() // x.shape[1], x.shape[1],
                                   weight.shape[0], dskip is not None)
        if plan["native"] or mode == "all":
            return _C.conv1x1_bwd_data(dy, weight, dskip)
    dx = _conv1x1_backward(dy, x, weight, (True, False, False))[0]
    return dx if dskip is None else dx + dskip


def native_conv1x1_mode() -> str:
    """"0": off; "all": every eligible shape; else the plan decides."""
    if not fused_bn_enabled():
        return "0"
    return os.environ.get("CGX_NATIVE_CONV1X1", "1")


def native_conv1x1_bwd_mode() -> str:
    """As native_conv1x1_mode, for the backward-data GEMM; off wherever the
    forward switch is."""
    if native_conv1x1_mode() == "0":
        return "0"
    return os.environ.get("CGX_NATIVE_CONV1X1_BWD", "1")


def native_conv1x1_wrw_mode() -> str:
    """As native_conv1x1_mode, for the backward-weights GEMM; off wherever
    the forward switch is."""
    if native_conv1x1_mode() == "0":
        return "0"
    return os.environ.get("CGX_NATIVE_CONV1X1_WRW", "1")


def _conv1x1_shape(conv, bn, x):
    """(rows, K, N) where everything but the plan admits the native kernels,
    else None."""
    if native_conv1x1_mode() == "0":
        return None
    if not (type(conv) is torch.nn.Conv2d and conv.kernel_size == (1, 1)
            and conv.stride == (1, 1) and conv.padding == (0, 0)
            and conv.dilation == (1, 1) and conv.groups == 1
            and conv.bias is None and conv.padding_mode == "zeros"):
        return None
    if not (bn.training and bn.track_running_stats
            and bn.momentum is not None and bn.weight is not None
            and bn.bias is not None and bn.weight.dtype == torch.float32):
        return None
    if not (x.is_cuda and x.dim() == 4 and x.dtype == torch.bfloat16
            and _C.bn_eligible(x)):
        return None
    w = conv.weight
    # under bf16 autocast the fp32 weight reaches the kernel as bf16
    autocast = (torch.is_autocast_enabled("cuda")
                and torch.get_autocast_dtype("cuda") == torch.bfloat16)
    if not (w.device == x.device and w.shape[1] == x.shape[1]
            and (w.dtype == torch.bfloat16
                 or (autocast and w.dtype == torch.float32))):
        return None
    if w.dtype == torch.bfloat16 and not _C.conv1x1_eligible(x, w):
        return None  # e.g. a weight view that is not dense or not aligned
    return x.numel() // x.shape[1], x.shape[1], w.shape[0]


def _conv1x1_native(shape) -> bool:
    plan = _C.conv1x1_plan(*shape)
    return plan["eligible"] and (plan["native"]
                                 or native_conv1x1_mode() == "all")


def _conv1x1_bwd_native(shape, with_add) -> bool:
    mode = native_conv1x1_bwd_mode()
    if mode == "0":
        return False
    plan = _C.conv1x1_bwd_plan(*shape, with_add)
    return plan["eligible"] and (plan["native"] or mode == "all")


def _conv1x1_wrw_native(shape) -> bool:
    mode = native_conv1x1_wrw_mode()
    if mode == "0":
        return False
    plan = _C.conv1x1_wrw_plan(*shape)
    return plan["eligible"] and (plan["native"] or mode == "all")


def _conv(conv, bn, x, fork=False):
    """``(conv(x), part, skip)``: ``part`` are the partials for ``bn``, or
    None where the stock convolution ran; ``skip`` is what a residual path
    continues from instead of ``x``.  It is ``x`` itself unless ``fork`` is
    set and the native backward-data is to add the path's gradient."""
    shape = _conv1x1_shape(conv, bn, x)
    if shape is None:
        return conv(x), None, x
    fwd = _conv1x1_native(shape)
    if torch.is_grad_enabled():
        fork = fork and _conv1x1_bwd_native(shape, True)
        if (fork or _conv1x1_bwd_native(shape, False)
                or _conv1x1_wrw_native(shape)):
            y, part, skip = _Conv1x1Fork.apply(x, conv.weight, fwd, fork)
            return y, part, (skip if fork else x)
    if fwd:
        return _Conv1x1Stats.apply(x, conv.weight) + (x,)
    return conv(x), None, x


def conv_bn_act(conv: torch.nn.Conv2d, bn: torch.nn.BatchNorm2d,
                x: torch.Tensor, identity: torch.Tensor = None,
                relu: bool = True, identity_conv: torch.nn.Conv2d = None,
                identity_bn: torch.nn.BatchNorm2d = None) -> torch.Tensor:
    """``relu(bn(conv(x)) + identity)``, or with ``identity_conv`` and
    ``identity_bn`` ``relu(bn(conv(x)) + identity_bn(identity_conv(identity)))``."""
    y, part, _ = _conv(conv, bn, x)
    if identity_conv is None:
        return bn_act(bn, y, identity, relu, part=part)
    yd, partd, _ = _conv(identity_conv, identity_bn, identity)
    return bn_act(bn, y, yd, relu, identity_bn=identity_bn, part=part,
                  identity_part=partd)


def conv_bn_act_fork(conv: torch.nn.Conv2d, bn: torch.nn.BatchNorm2d,
                     x: torch.Tensor, relu: bool = True):
    """``(relu(bn(conv(x))), skip)`` at the input of a residual block:
    ``skip`` has the value of ``x`` and is what the skip path must use in its
    place, so that the path's gradient reaches the convolution's backward
    (``_Conv1x1Fork``).  Where that does not apply ``skip`` is ``x``."""
    y, part, skip = _conv(conv, bn, x, fork=True)
    return bn_act(bn, y, None, relu, part=part), skip


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
