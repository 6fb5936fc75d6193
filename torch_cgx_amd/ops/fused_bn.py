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

The three 1x1 / stride 2 downsample convolutions (``identity_conv`` of the
first block of ``layer2..4``) have a native forward of their own,
``_C.conv1x1s2_stats`` (csrc/conv1x1s2_kernels.hip): both operands through a
ring of LDS stages, the stride-2 gather in the loads' addresses, and the
partials of its output for ``identity_bn``, so that the join needs no
statistics pass.  ``CGX_NATIVE_CONV1X1_S2`` switches it like the others and
depends on none of them; both gradients are the stock ones.

``conv3x3(conv, x)`` is ``conv(x)`` for the 3x3 / stride 1 / padding 1
convolution of a bottleneck.  Its weight gradient has a native implicit GEMM
(``_C.conv3x3_wrw``, csrc/conv3x3_kernels.hip) with the fixed summation order
of the 1x1 one; ``CGX_NATIVE_CONV3X3_WRW`` switches it like the others and
depends on none of them.  ``conv3x3_bn_act(conv, bn, x)`` is
``bn_act(bn, conv3x3(conv, x))`` with a native forward as well
(``_C.conv3x3_stats``), which hands ``bn`` its statistics as the 1x1 forward
does; ``CGX_NATIVE_CONV3X3`` switches it, on its own.  The input gradient of
both has the forward's implicit GEMM with the taps mirrored and the weight
read transposed (``_C.conv3x3_bwd_data``); ``CGX_NATIVE_CONV3X3_BWD`` switches
it, on its own as well.  The three 3x3 / stride 2 / padding 1 convolutions
(``conv2`` of the first block of ``layer2..4``) have a native forward of their
own, ``_C.conv3x3s2_stats``, which de-interleaves the input into four parity
planes in LDS and hands ``bn`` its statistics likewise;
``CGX_NATIVE_CONV3X3_S2`` switches it, on its own.  Their input gradient is
native as well (``_C.conv3x3s2_bwd_data``): the four pixels of every 2x2 cell
of dX are four sums over the rows of dY, nine products in all and none with an
inserted zero; ``CGX_NATIVE_CONV3X3_S2_BWD`` switches it, on its own.  So is their weight
gradient (``_C.conv3x3s2_wrw``, the ring of ``_C.conv3x3_wrw_ring`` on four
parity planes of the input, the same bits on every run);
``CGX_NATIVE_CONV3X3_S2_WRW`` switches it, on its own.

``conv_stem_bn_act_pool(conv, bn, x, pool)`` is
``bn_act_pool(bn, conv(x), pool)`` for the stem, ``Conv2d(3, 64, 7, stride=2,
padding=3)``.  Its forward has a native implicit GEMM built for three input
channels (``_C.conv_stem_stats``, csrc/conv_stem_kernels.hip), which hands
``bn`` its statistics as the other forwards do, so that the stem's statistics
pass disappears; its weight gradient is the stock one and it has no input
gradient to speak of.  ``CGX_NATIVE_CONV_STEM`` switches it like the others
(``0`` off, ``all`` every eligible problem, by default those its plan's table
has measured faster) and depends on none of them.

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
                eps, part=None):
        out, mean, invstd, arg = _C.bn_act_pool_forward(
            x, weight, bias, running_mean, running_var, momentum, eps, part)
        ctx.save_for_backward(x, mean, invstd, weight, arg)
        return out

    @staticmethod
    def backward(ctx, dy):
        x, mean, invstd, weight, arg = ctx.saved_tensors
        dx, dgamma, dbeta = _C.bn_act_pool_backward(dy, x, mean, invstd,
                                                    weight, arg)
        return (dx, dgamma, dbeta, None, None, None, None, None)


def fused_bn_enabled() -> bool:
    return os.environ.get("CGX_FUSED_BN", "1") != "0"


def _bn_native(bn) -> bool:
    """What the native kernels ask of the module, whatever its input."""
    return (bn.training and bn.track_running_stats
            and bn.momentum is not None and fused_bn_enabled()
            and bn.weight is not None and bn.bias is not None
            and bn.weight.dtype == torch.float32)


def _native(bn, x, identity) -> bool:
    if not _bn_native(bn):
        return False
    if not (x.is_cuda and _C.bn_eligible(x)):
        return False
    if identity is not None and not (
            identity.shape == x.shape and identity.device == x.device
            and _C.bn_eligible(identity)):
        return False
    return True


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


def native_conv1x1_s2_mode() -> str:
    """``CGX_NATIVE_CONV1X1_S2``, the switch of the stride-2 forward with
    statistics (``_C.conv1x1s2_stats``): "0" off, "all" every eligible
    problem, else ("1", the default) the problems its plan has measured
    faster.  Off where ``CGX_FUSED_BN`` is; no other switch reaches it."""
    if not fused_bn_enabled():
        return "0"
    return os.environ.get("CGX_NATIVE_CONV1X1_S2", "1")


class _Conv1x1S2(torch.autograd.Function):
    """``(y, part) = f(x, weight)``: ``conv2d(x, weight, stride=2)`` for a
    1x1 convolution by ``_C.conv1x1s2_stats``, with the BatchNorm partials of
    ``y``.  Both gradients are the stock ones."""

    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda", cast_inputs=torch.bfloat16)
    def forward(ctx, x, weight):
        ctx.save_for_backward(x, weight)
        y, part = _C.conv1x1s2_stats(x, weight)
        ctx.mark_non_differentiable(part)
        return y, part

    @staticmethod
    @torch.amp.custom_bwd(device_type="cuda")
    def backward(ctx, dy, _dpart):
        x, weight = ctx.saved_tensors
        dx, dw, _ = torch.ops.aten.convolution_backward(
            dy, x, weight, None, (2, 2), (0, 0), (1, 1), False, (0, 0), 1,
            (ctx.needs_input_grad[0], ctx.needs_input_grad[1], False))
        return dx, dw


def _conv1x1_s2(conv, bn, x):
    """``_conv`` for the 1x1 / stride 2 convolution of a downsample path:
    through ``_Conv1x1S2`` where its switch and its plan's table say so."""
    if _conv1x1_shape(conv, bn, x, (2, 2)) is None:
        return conv(x), None, x
    plan = _C.conv1x1s2_plan(x.shape[0], x.shape[2], x.shape[3], x.shape[1],
                             conv.weight.shape[0])
    if not _takes(native_conv1x1_s2_mode(), plan):
        return conv(x), None, x
    return (*_Conv1x1S2.apply(x, conv.weight), x)


def _conv1x1_shape(conv, bn, x, stride=(1, 1)):
    """(rows, K, N) of the input where everything but the plan admits the
    native kernels of a 1x1 convolution of that stride, (1, 1) or (2, 2),
    else None."""
    s2 = stride == (2, 2)
    if (native_conv1x1_s2_mode() if s2 else native_conv1x1_mode()) == "0":
        return None
    if not (type(conv) is torch.nn.Conv2d and conv.kernel_size == (1, 1)
            and conv.stride == stride and conv.padding == (0, 0)
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
    eligible = _C.conv1x1s2_eligible if s2 else _C.conv1x1_eligible
    if w.dtype == torch.bfloat16 and not eligible(x, w):
        return None  # e.g. a weight view that is not dense or not aligned
    return x.numel() // x.shape[1], x.shape[1], w.shape[0]


def _conv(conv, bn, x, fork=False):
    """``(conv(x), part, skip)``: ``part`` are the partials for ``bn``, or
    None where the stock convolution ran; ``skip`` is what a residual path
    continues from instead of ``x``.  It is ``x`` itself unless ``fork`` is
    set and the native backward-data is to add the path's gradient.  Stride
    2 has a forward of its own (``_conv1x1_s2``)."""
    if getattr(conv, "stride", None) == (2, 2):
        return _conv1x1_s2(conv, bn, x)
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


class _Conv3x3(torch.autograd.Function):
    """``(y, part) = f(x, weight)``: ``conv2d(x, weight, padding=1)``, by the
    native implicit GEMM with the BatchNorm partials of ``y``
    (``_C.conv3x3_stats``) where ``native_fwd`` says so, else stock with
    ``part`` None.  The weight gradient comes from ``_C.conv3x3_wrw_ring``
    where its switch and table have the problem, else with ``native_wrw`` from
    the native implicit GEMM (``_C.conv3x3_wrw``), and with ``native_bwd`` the
    input gradient from ``_C.conv3x3_bwd_data``, each where it takes the
    gradient that arrives; the stock backward computes what remains."""

    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda", cast_inputs=torch.bfloat16)
    def forward(ctx, x, weight, native_fwd, native_wrw, native_bwd=False):
        ctx.save_for_backward(x, weight)
        ctx.native_wrw = native_wrw
        ctx.native_bwd = native_bwd
        if native_fwd:
            y, part = _C.conv3x3_stats(x, weight)
            ctx.mark_non_differentiable(part)
            return y, part
        return F.conv2d(x, weight, padding=1), None

    @staticmethod
    @torch.amp.custom_bwd(device_type="cuda")
    def backward(ctx, dy, _dpart):
        x, weight = ctx.saved_tensors
        need_dx, need_dw = ctx.needs_input_grad[:2]
        dx = dw = None
        if need_dw and _conv3x3_wrw_ring_takes(dy, x):
            dw, need_dw = _C.conv3x3_wrw_ring(dy, x), False
        if need_dw and ctx.native_wrw and _C.conv3x3_wrw_eligible(dy, x):
            dw, need_dw = _C.conv3x3_wrw(dy, x), False
        if (need_dx and ctx.native_bwd
                and _C.conv3x3_bwd_eligible(dy, weight)):
            dx, need_dx = _C.conv3x3_bwd_data(dy, weight), False
        if need_dx or need_dw:
            dx_stock, dw_stock, _ = torch.ops.aten.convolution_backward(
                dy, x, weight, None, (1, 1), (1, 1), (1, 1), False, (0, 0), 1,
                (need_dx, need_dw, False))
            dx = dx_stock if need_dx else dx
            dw = dw_stock if need_dw else dw
        return dx, dw, None, None, None


def native_conv3x3_wrw_ring_mode() -> str:
    """``CGX_NATIVE_CONV3X3_WRW_RING``, the switch of the weight gradient
    through a ring of LDS stages (``_C.conv3x3_wrw_ring``): "0" off, "all"
    every eligible problem, else ("1", the default) the problems its plan has
    measured faster than the path they take without it.  Off where
    ``CGX_FUSED_BN`` is."""
    if not fused_bn_enabled():
        return "0"
    return os.environ.get("CGX_NATIVE_CONV3X3_WRW_RING", "1")


def _conv3x3_wrw_ring_takes(dy, x) -> bool:
    mode = native_conv3x3_wrw_ring_mode()
    if mode == "0" or not _C.conv3x3_wrw_ring_eligible(dy, x):
        return False
    return mode == "all" or _C.conv3x3_wrw_ring_plan(
        x.shape[0], x.shape[2], x.shape[3], x.shape[1], dy.shape[1])["native"]


def native_conv3x3_wrw_mode() -> str:
    """``CGX_NATIVE_CONV3X3_WRW``: "0" off, "all" every eligible problem, else
    ("1", the default) the problems its plan has measured faster.  Off where
    ``CGX_FUSED_BN`` is; the 1x1 switches and ``CGX_NATIVE_CONV3X3`` do not
    reach it."""
    if not fused_bn_enabled():
        return "0"
    return os.environ.get("CGX_NATIVE_CONV3X3_WRW", "1")


def native_conv3x3_mode() -> str:
    """``CGX_NATIVE_CONV3X3``, the switch of the forward with statistics, with
    the values of ``CGX_NATIVE_CONV3X3_WRW`` and as independent."""
    if not fused_bn_enabled():
        return "0"
    return os.environ.get("CGX_NATIVE_CONV3X3", "1")


def native_conv3x3_bwd_mode() -> str:
    """``CGX_NATIVE_CONV3X3_BWD``, the switch of the input gradient, with the
    values of ``CGX_NATIVE_CONV3X3_WRW`` and as independent."""
    if not fused_bn_enabled():
        return "0"
    return os.environ.get("CGX_NATIVE_CONV3X3_BWD", "1")


def native_conv3x3_s2_mode() -> str:
    """``CGX_NATIVE_CONV3X3_S2``, the switch of the stride-2 forward with
    statistics (``_C.conv3x3s2_stats``), with the values of
    ``CGX_NATIVE_CONV3X3_WRW``.  Off where ``CGX_FUSED_BN`` is; no other
    switch reaches it."""
    if not fused_bn_enabled():
        return "0"
    return os.environ.get("CGX_NATIVE_CONV3X3_S2", "1")


def native_conv3x3_s2_bwd_mode() -> str:
    """``CGX_NATIVE_CONV3X3_S2_BWD``, the switch of the stride-2 input
    gradient (``_C.conv3x3s2_bwd_data``), with the values of
    ``CGX_NATIVE_CONV3X3_WRW``.  Off where ``CGX_FUSED_BN`` is; no other
    switch reaches it, ``CGX_NATIVE_CONV3X3_S2`` and
    ``CGX_NATIVE_CONV3X3_BWD`` included."""
    if not fused_bn_enabled():
        return "0"
    return os.environ.get("CGX_NATIVE_CONV3X3_S2_BWD", "1")


def native_conv3x3_s2_wrw_mode() -> str:
    """``CGX_NATIVE_CONV3X3_S2_WRW``, the switch of the stride-2 weight
    gradient (``_C.conv3x3s2_wrw``), with the values of
    ``CGX_NATIVE_CONV3X3_WRW``.  Off where ``CGX_FUSED_BN`` is; no other
    switch reaches it."""
    if not fused_bn_enabled():
        return "0"
    return os.environ.get("CGX_NATIVE_CONV3X3_S2_WRW", "1")


class _Conv3x3S2(torch.autograd.Function):
    """``(y, part) = f(x, weight)``: ``conv2d(x, weight, stride=2,
    padding=1)``, by ``_C.conv3x3s2_stats`` with the BatchNorm partials of
    ``y`` where ``native_fwd`` says so, else stock with ``part`` None.  With
    ``native_bwd`` the input gradient comes from ``_C.conv3x3s2_bwd_data`` and
    with ``native_wrw`` the weight gradient from ``_C.conv3x3s2_wrw``, each
    where it takes the gradient that arrives; the stock backward computes
    what remains and is not called where nothing does."""

    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda", cast_inputs=torch.bfloat16)
    def forward(ctx, x, weight, native_fwd=True, native_bwd=False,
                native_wrw=False):
        ctx.save_for_backward(x, weight)
        ctx.native_bwd = native_bwd
        ctx.native_wrw = native_wrw
        if native_fwd:
            y, part = _C.conv3x3s2_stats(x, weight)
            ctx.mark_non_differentiable(part)
            return y, part
        return F.conv2d(x, weight, stride=2, padding=1), None

    @staticmethod
    @torch.amp.custom_bwd(device_type="cuda")
    def backward(ctx, dy, _dpart):
        x, weight = ctx.saved_tensors
        need_dx, need_dw = ctx.needs_input_grad[:2]
        dx = dw = None
        if (need_dx and ctx.native_bwd
                and _C.conv3x3s2_bwd_eligible(dy, weight)):
            dx, need_dx = _C.conv3x3s2_bwd_data(dy, weight), False
        if need_dw and ctx.native_wrw and _C.conv3x3s2_wrw_eligible(dy, x):
            dw, need_dw = _C.conv3x3s2_wrw(dy, x), False
        if need_dx or need_dw:
            dx_stock, dw_stock, _ = torch.ops.aten.convolution_backward(
                dy, x, weight, None, (2, 2), (1, 1), (1, 1), False, (0, 0), 1,
                (need_dx, need_dw, False))
            dx = dx_stock if need_dx else dx
            dw = dw_stock if need_dw else dw
        return dx, dw, None, None, None


def _conv3x3_weight(conv, x, stride):
    """The weight of a bias-free 3x3 / padding 1 convolution of that stride
    on a channels_last bf16 CUDA activation, where a native kernel could take
    the two, else None."""
    if not (type(conv) is torch.nn.Conv2d and conv.kernel_size == (3, 3)
            and conv.stride == stride and conv.padding == (1, 1)
            and conv.dilation == (1, 1) and conv.groups == 1
            and conv.bias is None and conv.padding_mode == "zeros"):
        return None
    if not (x.is_cuda and x.dim() == 4 and x.dtype == torch.bfloat16
            and _C.bn_eligible(x)):
        return None
    w = conv.weight
    # under bf16 autocast the fp32 weight reaches the convolution as bf16
    autocast = (torch.is_autocast_enabled("cuda")
                and torch.get_autocast_dtype("cuda") == torch.bfloat16)
    if not (w.device == x.device and w.shape[1] == x.shape[1]
            and (w.dtype == torch.bfloat16
                 or (autocast and w.dtype == torch.float32))):
        return None
    return w


def _takes(mode, plan):
    return mode != "0" and plan["eligible"] and (plan["native"]
                                                 or mode == "all")


def _conv3x3_s2(conv, x, bn):
    """``_conv3x3`` for stride 2: through ``_Conv3x3S2`` where the native
    forward is to run, which needs a training ``bn`` to take its partials,
    the native input gradient or the native weight gradient, which need grad
    mode; each by its own switch and its plan's table."""
    fwd_mode = native_conv3x3_s2_mode() if bn is not None else "0"
    bwd_mode = (native_conv3x3_s2_bwd_mode() if torch.is_grad_enabled()
                else "0")
    wrw_mode = (native_conv3x3_s2_wrw_mode() if torch.is_grad_enabled()
                else "0")
    if fwd_mode == "0" and bwd_mode == "0" and wrw_mode == "0":
        return conv(x), None
    w = _conv3x3_weight(conv, x, (2, 2))
    if w is None:
        return conv(x), None
    shape = (x.shape[0], x.shape[2], x.shape[3], x.shape[1], w.shape[0])
    fwd = (_takes(fwd_mode, _C.conv3x3s2_fwd_plan(*shape))
           and _native(bn, x, None)
           and w.is_contiguous(memory_format=torch.channels_last)
           and (w.dtype != torch.bfloat16
                or _C.conv3x3s2_fwd_eligible(x, w)))
    bwd = (x.requires_grad and x.shape[2] % 2 == 0 and x.shape[3] % 2 == 0
           and _takes(bwd_mode, _C.conv3x3s2_bwd_plan(*shape)))
    wrw = (w.requires_grad
           and _takes(wrw_mode, _C.conv3x3s2_wrw_plan(*shape)))
    if not (fwd or bwd or wrw):
        return conv(x), None
    return _Conv3x3S2.apply(x, w, fwd, bwd, wrw)


def _conv3x3(conv, x, bn=None):
    """``(conv(x), part)``.  For a bias-free 3x3 / stride 1 / padding 1
    convolution of a channels_last bf16 CUDA activation it goes through
    ``_Conv3x3`` where the native forward (only with a training ``bn`` to
    take its partials), the native weight gradient or the native input
    gradient is to run, each by its own switch and its plan's table; in every
    other case it is the module call itself and ``part`` is None.  Stride 2
    has a forward and an input gradient of its own (``_conv3x3_s2``)."""
    if getattr(conv, "stride", None) == (2, 2):
        return _conv3x3_s2(conv, x, bn)
    fwd_mode = native_conv3x3_mode() if bn is not None else "0"
    wrw_mode = native_conv3x3_wrw_mode() if torch.is_grad_enabled() else "0"
    bwd_mode = native_conv3x3_bwd_mode() if torch.is_grad_enabled() else "0"
    if fwd_mode == "0" and wrw_mode == "0" and bwd_mode == "0":
        return conv(x), None
    w = _conv3x3_weight(conv, x, (1, 1))
    if w is None:
        return conv(x), None
    shape = (x.shape[0], x.shape[2], x.shape[3], x.shape[1], w.shape[0])
    # the cast of a weight keeps its strides: the kernel wants [N][3][3][C]
    fwd = (_takes(fwd_mode, _C.conv3x3_fwd_plan(*shape))
           and _native(bn, x, None)
           and w.is_contiguous(memory_format=torch.channels_last)
           and (w.dtype != torch.bfloat16 or _C.conv3x3_fwd_eligible(x, w)))
    wrw = w.requires_grad and _takes(wrw_mode, _C.conv3x3_wrw_plan(*shape))
    bwd = x.requires_grad and _takes(bwd_mode, _C.conv3x3_bwd_plan(*shape))
    if not (fwd or wrw or bwd):
        return conv(x), None
    return _Conv3x3.apply(x, w, fwd, wrw, bwd)


def conv3x3(conv: torch.nn.Conv2d, x: torch.Tensor) -> torch.Tensor:
    """``conv(x)``, through ``_Conv3x3`` where the native weight gradient is
    to compute the gradient of its weight (``native_conv3x3_wrw_mode``) or
    the native input gradient that of ``x`` (``native_conv3x3_bwd_mode``)."""
    return _conv3x3(conv, x)[0]


def conv3x3_bn_act(conv: torch.nn.Conv2d, bn: torch.nn.BatchNorm2d,
                   x: torch.Tensor, relu: bool = True) -> torch.Tensor:
    """``relu(bn(conv(x)))`` for the 3x3 convolution of a bottleneck: where
    the native forward runs (``native_conv3x3_mode``), ``bn`` takes its
    statistics from the partials that come with the output."""
    y, part = _conv3x3(conv, x, bn)
    return bn_act(bn, y, None, relu, part=part)


def _pool_is_3x3_s2_p1(pool) -> bool:
    def pair(v):
        return tuple(v) if isinstance(v, (tuple, list)) else (v, v)

    return (type(pool) is torch.nn.MaxPool2d
            and pair(pool.kernel_size) == (3, 3) and pair(pool.stride) == (2, 2)
            and pair(pool.padding) == (1, 1) and pair(pool.dilation) == (1, 1)
            and not pool.ceil_mode and not pool.return_indices)


def bn_act_pool(bn: torch.nn.BatchNorm2d, x: torch.Tensor,
                pool: torch.nn.Module, part: torch.Tensor = None
                ) -> torch.Tensor:
    """``pool(relu(bn(x)))``.  ``part`` are the statistics partials that came
    with ``x`` from the native stem convolution, if it produced them."""
    if _pool_is_3x3_s2_p1(pool) and _native(bn, x, None):
        bn.num_batches_tracked.add_(1)
        return _BnActPool.apply(x, *_bn_args(bn), part)
    return pool(bn_act(bn, x, part=part))


class _ConvStem(torch.autograd.Function):
    """``(y, part) = f(x, weight)``: ``conv2d(x, weight, stride=2,
    padding=3)``, by the native implicit GEMM with the BatchNorm partials of
    ``y`` (``_C.conv_stem_stats``) where ``native_fwd`` says so, else stock
    with ``part`` None.  With ``native_wrw`` the weight gradient comes from
    the native implicit GEMM (``_C.conv_stem_wrw``) where it takes the
    gradient that arrives; the stock backward computes what remains."""

    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda", cast_inputs=torch.bfloat16)
    def forward(ctx, x, weight, native_fwd, native_wrw=False):
        ctx.save_for_backward(x, weight)
        ctx.native_wrw = native_wrw
        if native_fwd:
            y, part = _C.conv_stem_stats(x, weight)
            ctx.mark_non_differentiable(part)
            return y, part
        return F.conv2d(x, weight, None, 2, 3), None

    @staticmethod
    @torch.amp.custom_bwd(device_type="cuda")
    def backward(ctx, dy, _dpart):
        x, weight = ctx.saved_tensors
        need_dx, need_dw = ctx.needs_input_grad[:2]
        dx = dw = None
        if need_dw and ctx.native_wrw and _C.conv_stem_wrw_eligible(dy, x):
            dw, need_dw = _C.conv_stem_wrw(dy, x), False
        if need_dx or need_dw:
            dx_stock, dw_stock, _ = torch.ops.aten.convolution_backward(
                dy, x, weight, None, (2, 2), (3, 3), (1, 1), False, (0, 0), 1,
                (need_dx, need_dw, False))
            dx = dx_stock if need_dx else dx
            dw = dw_stock if need_dw else dw
        return dx, dw, None, None


def native_conv_stem_wrw_mode() -> str:
    """``CGX_NATIVE_CONV_STEM_WRW``, the switch of the stem's weight gradient
    (``_C.conv_stem_wrw``): "0" off, "all" every eligible problem, else ("1",
    the default) the problems its plan has measured faster.  Off where
    ``CGX_FUSED_BN`` is; ``CGX_NATIVE_CONV_STEM`` does not reach it."""
    if not fused_bn_enabled():
        return "0"
    return os.environ.get("CGX_NATIVE_CONV_STEM_WRW", "1")


def native_conv_stem_mode() -> str:
    """``CGX_NATIVE_CONV_STEM``, the switch of the stem's forward with
    statistics: "0" off, "all" every eligible problem, else ("1", the
    default) the problems its plan has measured faster.  Off where
    ``CGX_FUSED_BN`` is; no other switch reaches it."""
    if not fused_bn_enabled():
        return "0"
    return os.environ.get("CGX_NATIVE_CONV_STEM", "1")


def _conv_stem_takes(conv, x) -> bool:
    """Whether ``conv`` is the stem and ``conv.weight`` and ``x`` are what
    its native kernels take."""
    if not (type(conv) is torch.nn.Conv2d and conv.kernel_size == (7, 7)
            and conv.stride == (2, 2) and conv.padding == (3, 3)
            and conv.dilation == (1, 1) and conv.groups == 1
            and conv.bias is None and conv.padding_mode == "zeros"
            and conv.in_channels == 3 and conv.out_channels == 64):
        return False
    # under bf16 autocast fp32 tensors reach the kernel as bf16; the cast
    # keeps the strides, and the kernel wants both channels_last.  A tensor
    # that is bf16 already reaches it as it is and must be 16-byte aligned.
    autocast = (torch.is_autocast_enabled("cuda")
                and torch.get_autocast_dtype("cuda") == torch.bfloat16)
    w = conv.weight

    def takes(t):
        return (t.is_cuda and t.dim() == 4
                and t.is_contiguous(memory_format=torch.channels_last)
                and (t.data_ptr() % 16 == 0 if t.dtype == torch.bfloat16
                     else autocast and t.dtype == torch.float32))

    return (takes(x) and takes(w) and w.device == x.device
            and x.shape[1] == 3)


def _conv_stem_native(conv, bn, x, pool) -> bool:
    """Whether ``_C.conv_stem_stats`` is to compute ``conv(x)`` for ``bn``
    and ``pool``: the switch and the plan say so and the modules and tensors
    are what the kernels take."""
    mode = native_conv_stem_mode()
    if mode == "0":
        return False
    if not (_conv_stem_takes(conv, x) and _pool_is_3x3_s2_p1(pool)):
        return False
    plan = _C.conv_stem_plan(x.shape[0], x.shape[2], x.shape[3])
    # the plan's bounds on the output's pixels are the BatchNorm kernels'
    return (plan["eligible"] and (plan["native"] or mode == "all")
            and _bn_native(bn))


def _conv_stem_wrw_native(conv, x) -> bool:
    """Whether ``_C.conv_stem_wrw`` is to compute the gradient of
    ``conv.weight``: the switch and the plan say so."""
    mode = native_conv_stem_wrw_mode() if torch.is_grad_enabled() else "0"
    if mode == "0" or not conv.weight.requires_grad:
        return False
    if not _conv_stem_takes(conv, x):
        return False
    plan = _C.conv_stem_wrw_plan(x.shape[0], x.shape[2], x.shape[3])
    return plan["eligible"] and (plan["native"] or mode == "all")


def conv_stem_bn_act_pool(conv: torch.nn.Conv2d, bn: torch.nn.BatchNorm2d,
                          x: torch.Tensor, pool: torch.nn.Module
                          ) -> torch.Tensor:
    """``pool(relu(bn(conv(x))))`` for the stem: where the native forward
    runs (``native_conv_stem_mode``), ``bn`` takes its statistics from the
    partials that come with the output; where the native weight gradient
    runs (``native_conv_stem_wrw_mode``), the backward takes it.  Each has
    its own switch and its plan's table, as in ``_conv3x3``."""
    fwd = _conv_stem_native(conv, bn, x, pool)
    wrw = _conv_stem_wrw_native(conv, x)
    if not (fwd or wrw):
        return bn_act_pool(bn, conv(x), pool)
    y, part = _ConvStem.apply(x, conv.weight, fwd, wrw)
    return bn_act_pool(bn, y, pool, part=part)
