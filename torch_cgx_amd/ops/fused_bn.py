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

``conv_bn_act(conv, bn, x, ...)`` is ``bn_act(bn, conv(x), ...)``, and
``identity_conv`` the downsample convolution of a join.  A 1x1 / stride 1
convolution has three native GEMMs (csrc/conv1x1_kernels.hip), each taken at
the shapes its own table in the plan (csrc/conv1x1_plan.cc) has measured
faster than the stock path:

* the forward (``_C.conv1x1_stats``) also hands the BatchNorm the per-channel
  partial statistics of its output, so the statistics pass is skipped;
* the input gradient (``_C.conv1x1_bwd_data``) can add a second tensor in
  its epilogue.  ``conv_bn_act_fork`` is ``conv_bn_act`` at the input of a
  residual block: it also returns the tensor the skip path continues from,
  and the gradient arriving over that path is added there, not by autograd
  in a pass of its own;
* the weight gradient (``_C.conv1x1_wrw``) splits the rows and sums the
  fp32 partials in a fixed order: the same bits every run.  For the deep
  layers, where a workgroup walks few and large chunks, a second kernel
  (``_C.conv1x1_wrw_ring``) loads them straight into a ring of LDS buffers;
  it has a table of its own, is asked first, and gives the bits of the first
  wherever both split the rows alike.

The forward and the input gradient each have a second kernel for the shapes
whose weight tile does not stay in LDS (``_C.conv1x1_tiled_stats``,
``_C.conv1x1_tiled_bwd_data``: 256-row tiles, the weight double-buffered in
LDS chunk by chunk).  They give the bits of the first two, have tables of their
own, and are asked first.

``CGX_NATIVE_CONV1X1``, ``CGX_NATIVE_CONV1X1_BWD``,
``CGX_NATIVE_CONV1X1_WRW``, ``CGX_NATIVE_CONV1X1_WRW_RING`` and
``CGX_NATIVE_CONV1X1_TILED`` (both tiled kernels) switch them: ``0`` off,
``all`` every shape the kernel accepts, measured faster or not.  The backward
switches and the tiled one are off wherever the forward one is, the tiled
input gradient also wherever ``CGX_NATIVE_CONV1X1_BWD`` is, and the ring
wherever ``CGX_NATIVE_CONV1X1_WRW`` is.

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


class _Conv1x1(torch.autograd.Function):
    """``(y, part, skip) = f(x, weight)``: the 1x1 convolution, native with
    partials (``native_fwd`` "tiled": by the tiled kernel) or stock with
    ``part`` None as ``native_fwd`` says, and with
    ``fork`` its input once more as ``skip``, for the residual path to go on
    from.  The backward then receives the gradients of both at once, and the
    native backward-data GEMM adds the skip gradient in its epilogue instead
    of autograd in a pass of its own.  Each gradient comes from its native
    GEMM where that is taken; where neither is, both come from one stock
    convolution backward."""

    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda", cast_inputs=torch.bfloat16)
    def forward(ctx, x, weight, native_fwd, fork):
        if native_fwd:
            y, part = (_C.conv1x1_tiled_stats(x, weight)
                       if native_fwd == "tiled"
                       else _C.conv1x1_stats(x, weight))
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
        need_dx, need_dw = ctx.needs_input_grad[:2]
        if dy is None:
            return (dskip if need_dx else None), None, None, None
        if (need_dx and need_dw and not _conv1x1_dw_native(dy, x)
                and not _conv1x1_dx_native(dy, weight, dskip)):
            dx, dw, _ = _conv1x1_backward(dy, x, weight, (True, True, False))
            return (dx if dskip is None else dx + dskip), dw, None, None
        dw = _conv1x1_dw(dy, x, weight) if need_dw else None
        dx = _conv1x1_dx(dy, x, weight, dskip) if need_dx else None
        return dx, dw, None, None


def _conv1x1_backward(dy, x, weight, mask):
    return torch.ops.aten.convolution_backward(
        dy, x, weight, None, (1, 1), (0, 0), (1, 1), False, (0, 0), 1, mask)


def _conv1x1_dw_kernel(dy, x):
    """The native backward-weights entry point that takes this problem, the
    ring first, or None."""
    if not _C.conv1x1_wrw_eligible(dy, x):
        return None
    shape = (x.numel() // x.shape[1], x.shape[1], dy.shape[1])
    for kernel, entry in (("wrw_ring", "conv1x1_wrw_ring"),
                          ("wrw", "conv1x1_wrw")):
        if _conv1x1_takes(kernel, shape):
            return getattr(_C, entry)
    return None


def _conv1x1_dw_native(dy, x) -> bool:
    return _conv1x1_dw_kernel(dy, x) is not None


def _conv1x1_dx_kernel(dy, weight, dskip):
    """The native backward-data entry point that takes this problem, the
    tiled one first, or None."""
    if not _C.conv1x1_bwd_eligible(dy, weight, dskip):
        return None
    shape = (dy.numel() // dy.shape[1], weight.shape[1], weight.shape[0])
    for kernel, entry in (("tiled_bwd", "conv1x1_tiled_bwd_data"),
                          ("bwd", "conv1x1_bwd_data")):
        if _conv1x1_takes(kernel, shape, dskip is not None):
            return getattr(_C, entry)
    return None


def _conv1x1_dx_native(dy, weight, dskip) -> bool:
    return _conv1x1_dx_kernel(dy, weight, dskip) is not None


def _conv1x1_dw(dy, x, weight):
    """The weight gradient: the native GEMM where the plan has measured it
    faster, else the stock one."""
    kernel = _conv1x1_dw_kernel(dy, x)
    if kernel is not None:
        return kernel(dy, x)
    return _conv1x1_backward(dy, x, weight, (False, True, False))[1]


def _conv1x1_dx(dy, x, weight, dskip):
    """The input gradient plus ``dskip`` (or None): one native GEMM where the
    plan has measured it faster, else the stock backward-data and a ``+``."""
    kernel = _conv1x1_dx_kernel(dy, weight, dskip)
    if kernel is not None:
        return kernel(dy, weight, dskip)
    dx = _conv1x1_backward(dy, x, weight, (True, False, False))[0]
    return dx if dskip is None else dx + dskip


# kernel -> (its switch, its plan in _C)
_CONV1X1_KERNELS = {
    "fwd": ("CGX_NATIVE_CONV1X1", "conv1x1_plan"),
    "bwd": ("CGX_NATIVE_CONV1X1_BWD", "conv1x1_bwd_plan"),
    "wrw": ("CGX_NATIVE_CONV1X1_WRW", "conv1x1_wrw_plan"),
    "wrw_ring": ("CGX_NATIVE_CONV1X1_WRW_RING", "conv1x1_wrw_ring_plan"),
    "tiled_fwd": ("CGX_NATIVE_CONV1X1_TILED", "conv1x1_tiled_plan"),
    "tiled_bwd": ("CGX_NATIVE_CONV1X1_TILED", "conv1x1_tiled_bwd_plan"),
}


def _conv1x1_mode(kernel: str) -> str:
    """The switch of the forward ("fwd"), backward-data ("bwd") or
    backward-weights ("wrw") GEMM, or of the tiled forward ("tiled_fwd") or
    backward-data ("tiled_bwd") or the ring backward-weights ("wrw_ring").
    "0": off; "all": every eligible shape; else the plan decides.  All are
    off where ``CGX_FUSED_BN`` or the forward switch is, the tiled
    backward-data also where the backward-data one is and the ring
    backward-weights where the backward-weights one is; "all" is not
    inherited."""
    if not fused_bn_enabled() or os.environ.get("CGX_NATIVE_CONV1X1") == "0":
        return "0"
    if (kernel == "wrw_ring"
            and os.environ.get("CGX_NATIVE_CONV1X1_WRW") == "0"):
        return "0"
    if (kernel == "tiled_bwd"
            and os.environ.get("CGX_NATIVE_CONV1X1_BWD") == "0"):
        return "0"
    return os.environ.get(_CONV1X1_KERNELS[kernel][0], "1")


def native_conv1x1_mode() -> str:
    return _conv1x1_mode("fwd")


def native_conv1x1_bwd_mode() -> str:
    return _conv1x1_mode("bwd")


def native_conv1x1_wrw_mode() -> str:
    return _conv1x1_mode("wrw")


def native_conv1x1_wrw_ring_mode() -> str:
    return _conv1x1_mode("wrw_ring")


def _conv1x1_takes(kernel: str, shape, *with_add) -> bool:
    """Whether ``kernel`` is to run at ``shape`` = (rows, K, N): its switch is
    on and its plan has measured it faster there, or the switch says "all"."""
    mode = _conv1x1_mode(kernel)
    if mode == "0":
        return False
    plan = getattr(_C, _CONV1X1_KERNELS[kernel][1])(*shape, *with_add)
    return plan["eligible"] and (plan["native"] or mode == "all")


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


def _conv(conv, bn, x, fork=False):
    """``(conv(x), part, skip)``: ``part`` are the partials for ``bn``, or
    None where the stock convolution ran; ``skip`` is what a residual path
    continues from instead of ``x``.  It is ``x`` itself unless ``fork`` is
    set and the native backward-data is to add the path's gradient."""
    shape = _conv1x1_shape(conv, bn, x)
    if shape is None:
        return conv(x), None, x
    fwd = ("tiled" if _conv1x1_takes("tiled_fwd", shape)
           else _conv1x1_takes("fwd", shape))
    grad = torch.is_grad_enabled()

    def bwd(with_add):
        return (_conv1x1_takes("tiled_bwd", shape, with_add)
                or _conv1x1_takes("bwd", shape, with_add))

    fork = fork and grad and bwd(True)
    if not (fwd or fork or (grad and (bwd(False)
                                      or _conv1x1_takes("wrw_ring", shape)
                                      or _conv1x1_takes("wrw", shape)))):
        return conv(x), None, x
    y, part, skip = _Conv1x1.apply(x, conv.weight, fwd, fork)
    return y, part, (skip if fork else x)


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
    (``_Conv1x1``).  Where that does not apply ``skip`` is ``x``."""
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
