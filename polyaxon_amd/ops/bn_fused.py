"""Autograd wrapper for the fused NHWC bf16 BatchNorm(+add)(+ReLU) HIP kernels (csrc/bn_kernels.hip).

Forward (training): stats → finalize (mean/invstd/scale/bias + running-stat update) → apply.
Backward: reduce (Σdz, Σdz·x̂) → finalize (dγ, dβ, dx coefficients) → dx (+ d_residual) in one pass.
With ReLU the forward also writes a 1-bit-per-element mask (1/16 of ``y``); the backward reads it instead of
``y``, one fewer full activation stream in each of its two passes.
"""
from __future__ import annotations

import ctypes
import functools

from typing import Optional

import torch

from polyaxon_amd.ops import _native
from polyaxon_amd.ops.conv1x1 import BnLink, PendingApply, ds_bwd_route, fill_pending
from polyaxon_amd.ops.flat import direct_grad


def _stream() -> int:
    return _native.current_stream()


_COUNTERS = {}


def _counters(dev: torch.device):
    """Zeroed ticket counters of the one-launch reduce + finalize (csrc/bn_kernels.hip ``reduce_l2_last``), one
    array per (device, stream): launches sharing it are stream-ordered and each leaves it zeroed again."""
    key = (dev.index, torch.cuda.current_stream(dev).cuda_stream)
    # >= ceil(2048 / 64) groups
    return _native.cached(_COUNTERS, key, lambda: torch.zeros(64, dtype=torch.int32, device=dev)).data_ptr()


@functools.lru_cache(maxsize=None)
def _lib() -> ctypes.CDLL:
    return _native.lib("plx_bn")  # loaded once: _native.lib takes a lock on every call


def _p(t):
    """Device address of a tensor; ``None`` and raw addresses pass through."""
    return t if t is None or isinstance(t, int) else t.data_ptr()


def _workspace(m: int, c: int, ext_part, ext_nblk: int, device) -> torch.Tensor:
    """fp32 workspace of one call: the level-2 rows for the ``ext_nblk`` rows of external partials, else (``ext_part``
    is ``None``) both levels of the call's own statistics / reduce pass -- the rule of csrc/bn_kernels.hip."""
    n = (_native.size("plx_bn", "plx_bn_l2_workspace", ext_nblk, c) if ext_part is not None
         else _native.size("plx_bn", "plx_bn_workspace", m, c))
    if n < 0:
        raise RuntimeError("unsupported channel count for fused BN")
    return torch.empty(n, dtype=torch.float32, device=device)


def bn_forward(*, x, m, c, gamma, beta, eps, momentum, save_mean, save_invstd, scale_bias, workspace, res=None,
               y=None, relu=False, running_mean=None, running_var=None, ext_part=None, ext_nblk=0, mask=None,
               res_sb=None, counters=None, stream=None) -> None:
    """``plx_bn_forward`` (csrc/bn_kernels.hip ``BnForwardArgs``, which documents the fields): pointers are tensors,
    raw addresses or ``None``.  Raises when the library refuses the call."""
    a = _native.BnForwardArgs(
        x=_p(x), res=_p(res), y=_p(y), M=m, C=c, relu=int(relu), gamma=_p(gamma), beta=_p(beta), eps=eps,
        momentum=momentum, running_mean=_p(running_mean), running_var=_p(running_var), save_mean=_p(save_mean),
        save_invstd=_p(save_invstd), scale_bias=_p(scale_bias), workspace=_p(workspace), ext_part=_p(ext_part),
        ext_nblk=ext_nblk, mask=_p(mask), res_sb=_p(res_sb), counters=_p(counters))
    rc = _lib().plx_bn_forward(ctypes.byref(a), _stream() if stream is None else stream)
    _native.check(rc, "plx_bn_forward")


def bn_backward(*, x, dy, m, c, gamma, save_mean, save_invstd, dgamma, dbeta, coef, workspace, mask=None, dx=None,
                dres=None, relu=False, accumulate=0, ext_part=None, ext_nblk=0, resbn=None, counters=None,
                stream=None, no_dres=False) -> None:
    """``plx_bn_backward`` (csrc/bn_kernels.hip ``BnBackwardArgs``); ``dx=None``: reduce + finalize only; ``resbn``:
    a :class:`~polyaxon_amd.ops._native.ResBnArgs` or ``None``; ``no_dres``: that ResBn comes without ``dres`` on
    purpose (its consumer takes ``dy`` and the mask).  Raises when the library refuses the call."""
    a = _native.BnBackwardArgs(
        x=_p(x), mask=_p(mask), dy=_p(dy), dx=_p(dx), dres=_p(dres), M=m, C=c, relu=int(relu), gamma=_p(gamma),
        save_mean=_p(save_mean), save_invstd=_p(save_invstd), dgamma=_p(dgamma), dbeta=_p(dbeta), coef=_p(coef),
        workspace=_p(workspace), ext_part=_p(ext_part), ext_nblk=ext_nblk, accumulate=int(accumulate),
        counters=_p(counters), no_dres=int(no_dres))
    if resbn is not None:
        a.resbn = resbn
    rc = _lib().plx_bn_backward(ctypes.byref(a), _stream() if stream is None else stream)
    _native.check(rc, "plx_bn_backward")


def _cl(t: torch.Tensor) -> torch.Tensor:
    return t if t.is_contiguous(memory_format=torch.channels_last) else t.contiguous(memory_format=torch.channels_last)


def supported(x: torch.Tensor) -> bool:
    if not x.is_cuda or x.dtype != torch.bfloat16 or x.dim() != 4:
        return False
    c = x.shape[1]
    g = c // 8
    return c % 8 == 0 and g > 0 and (g & (g - 1)) == 0 and x.numel() > 0


class _BNAct(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, running_mean, running_var, residual, momentum, eps, relu, ext=None, box=None,
                link=None, rlink=None, defer=False, dxsink=None, pend=None):
        # dxsink (ops.conv1x1.DxSink): x is a 1x1 convolution's output as is, and that convolution's data-gradient
        # GEMM can produce this BatchNorm's dx (the backward decides)
        ctx.dxsink = dxsink if x.is_contiguous(memory_format=torch.channels_last) else None
        x = _cl(x)
        n, c, h, w = x.shape
        m = n * h * w
        f32 = dict(dtype=torch.float32, device=x.device)
        # defer: no apply pass -- the output aliases x and its only consumer (the residual add of a fused
        # BatchNorm) applies scale/bias on the fly (link.affine); the backward is unchanged
        defer = bool(defer) and not relu and residual is None and link is not None
        y = None if defer else torch.empty_like(x, memory_format=torch.channels_last)
        # pend: reduce / finalize only -- y and the mask are allocated but left unwritten, and the forward GEMM of the
        # 1x1 convolution that reads y fills them (ops.conv1x1.PendingApply, handed to bn_act through the list `pend`)
        holder, pend = pend, pend is not None and relu and residual is not None and not defer
        stats = torch.empty(4 * c, **f32)  # mean | invstd | scale | bias
        res_sb = None
        if residual is not None:
            rl = getattr(residual, "_plx_bn_link", None)
            if rl is not None and rl.affine is not None and getattr(residual, "_plx_deferred", False):
                res_sb = rl.affine
        res = _cl(residual) if residual is not None else None
        mask = torch.empty(m * c // 8, dtype=torch.uint8, device=x.device) if relu else None
        # ext: channel sums from the producing conv's GEMM epilogue -- no stats pass over x
        part, nblk = ext if ext is not None else (None, 0)
        sp = stats.data_ptr()  # addresses of its rows below, not slices: a slice costs the host over a microsecond
        bn_forward(x=x, res=res, y=None if pend else y, m=m, c=c, gamma=weight, beta=bias, eps=float(eps),
                   momentum=float(momentum), running_mean=running_mean, running_var=running_var, save_mean=sp,
                   save_invstd=sp + 4 * c, scale_bias=sp + 8 * c, workspace=_workspace(m, c, part, nblk, x.device),
                   ext_part=part, ext_nblk=nblk, mask=mask, relu=relu, res_sb=res_sb, counters=_counters(x.device))
        ctx.save_for_backward(x, mask, weight, stats)
        ctx.pending = PendingApply(x, res, stats[2 * c:], res_sb, mask, y) if pend else None
        if pend:
            holder.append(ctx.pending)
        ctx.relu = relu
        ctx.has_res = residual is not None
        ctx.box = box if (box is not None and box.armed and residual is not None) else None
        if ctx.box is not None:
            ctx.box.expect = True
        # direct gradients: dgamma / dbeta accumulate into the flat gradient slots (ops.flat.direct_grad)
        gw, gb = direct_grad(weight), direct_grad(bias)
        ctx.direct = (gw, gb) if (gw is not None and gb is not None) else None
        # the consumer conv may produce this BN's backward partials in its dgrad epilogue (ops.conv1x1.BnLink)
        ctx.link = link
        if link is not None:
            link.x, link.mask, link.mean, link.invstd = x, mask, stats[:c], stats[c:2 * c]
            if defer:
                link.affine = stats[2 * c:]
        # rlink: the residual came from a fused BatchNorm whose output nothing else consumes (a downsampling branch):
        # d_residual is that BatchNorm's whole gradient, so the dx pass below reduces its backward partials too, or
        # (ops.conv1x1.ds_bwd_route "A") leaves the reduce to it; either way it gets (dy, mask) instead of d_residual
        # (c <= 2048: plx_bn_backward refuses a ResBn above 256 channel groups; that BatchNorm then runs its own reduce)
        ctx.rlink = rlink if (rlink is not None and residual is not None and rlink.x is not None
                              and rlink.x.shape == x.shape and ctx.box is None and c <= 2048) else None
        if defer:
            return x.view_as(x)  # the raw input; bn_act marks it _plx_deferred
        return y

    @staticmethod
    def backward(ctx, dy):
        x, mask, weight, stats = ctx.saved_tensors
        if ctx.pending is not None:  # the mask read below was left to the consumer's GEMM (or materialize) to write
            ctx.pending.check_done()
        n, c, h, w = x.shape
        m = n * h * w
        dy = _cl(dy)
        if dy.dtype != torch.bfloat16:
            dy = dy.to(torch.bfloat16)
        f32 = dict(dtype=torch.float32, device=x.device)
        dx = torch.empty_like(x, memory_format=torch.channels_last)
        # identity block: the residual's gradient dz = dy * mask is not written here; dy and the mask ride into
        # conv1's dgrad epilogue (GradMailbox.put_masked), which adds them
        masked_box = ctx.box is not None and ctx.relu and mask is not None
        # downsampling block (rlink): the residual's gradient is not written either -- dy itself is returned for it and
        # the downsample BatchNorm's backward forms dz = dy * mask from this ReLU's mask (BnLink.foreign), on route "A"
        # or "B" of ops.conv1x1.ds_bwd_route; "off" writes d_residual
        rl = ctx.rlink
        route = "off"
        # part: the consumer's dgrad epilogue already reduced dz and dz*xhat per block
        part, nblk = ctx.link.take() if ctx.link is not None else (None, 0)
        if rl is not None and ctx.relu and mask is not None and rl.mask is None:
            sk = ctx.dxsink
            route = ds_bwd_route(sk.cin if sk is not None else 0, c, sk is not None and part is not None)
        # the mask test of a BatchNorm that is itself on the receiving end: dz = dy * (the ReLU mask downstream)
        foreign, relu = (ctx.link.foreign if ctx.link is not None else None), ctx.relu
        if foreign is not None:
            ctx.link.foreign = None
            if relu or foreign[0].data_ptr() != dy.data_ptr() or foreign[0].shape != dy.shape:
                raise RuntimeError("BnLink.foreign: the gradient handed to the BatchNorm is not the one its mask masks")
            relu, mask = True, foreign[1]
        dres = (torch.empty_like(x, memory_format=torch.channels_last)
                if ctx.has_res and not masked_box and route == "off" else None)
        if ctx.direct is not None:
            dg_ptr, db_ptr, acc = ctx.direct[0].data_ptr(), ctx.direct[1].data_ptr(), 1
            dgb = None
        else:
            dgb = torch.empty(2 * c, **f32)
            dg_ptr, db_ptr, acc = dgb.data_ptr(), dgb[c:].data_ptr(), 0
        coef = torch.empty(3 * c, **f32)
        # only dx to write (dxsink): reduce / finalize here, and the data-gradient GEMM of the convolution that produced
        # x forms dx = coef[0]·dz + coef[1]·x + coef[2] itself, into this (still unwritten) buffer
        sink = ctx.dxsink if (dres is None and route != "B") else None
        rb = None
        if rl is not None and route != "A":  # the dx pass reduces the residual BatchNorm's partials, with or without dres
            rl.nblk = _native.size("plx_bn", "plx_bn_dx_blocks", m, c)
            rl.part = torch.empty(2 * rl.nblk * c, **f32)
            rb = _native.ResBnArgs(_p(rl.x), _p(rl.mask), _p(rl.mean), _p(rl.invstd), _p(rl.part))
        bn_backward(x=x, mask=mask, dy=dy, dx=None if sink is not None else dx, dres=dres, m=m, c=c, gamma=weight,
                    save_mean=stats, save_invstd=stats.data_ptr() + 4 * c, dgamma=dg_ptr, dbeta=db_ptr, coef=coef,
                    workspace=_workspace(m, c, part, nblk, x.device), ext_part=part, ext_nblk=nblk, relu=relu,
                    accumulate=acc, resbn=rb, counters=_counters(x.device), no_dres=route == "B")
        if sink is not None:
            sink.put(dy, x, mask if relu else None, coef, dx)
        if route != "off":  # the residual BatchNorm's backward gets dy itself and masks it with this ReLU's mask
            rl.foreign = (dy, mask)
            dres = dy
        if ctx.box is not None:  # the residual's gradient rides into conv1's dgrad epilogue (ops.conv1x1)
            if masked_box:
                ctx.box.put_masked(dy, mask)
            else:
                ctx.box.put(dres)
            dres = None
        dgamma = dgb[:c] if dgb is not None else None
        dbeta = dgb[c:] if dgb is not None else None
        return dx, dgamma, dbeta, None, None, dres, None, None, None, None, None, None, None, None, None, None


class _Materialize(torch.autograd.Function):
    """A deferred BatchNorm output (the raw input plus its pending scale/bias) made real for a consumer that does
    not apply the affine itself; the gradient passes through unchanged (it is the BatchNorm output's gradient)."""

    @staticmethod
    def forward(ctx, t, sb):
        c = t.shape[1]
        return (t.float() * sb[:c].view(1, c, 1, 1) + sb[c:].view(1, c, 1, 1)).to(t.dtype).contiguous(
            memory_format=torch.channels_last)

    @staticmethod
    def backward(ctx, g):
        return g, None


def materialize(t: Optional[torch.Tensor]) -> Optional[torch.Tensor]:
    """The real value of a possibly deferred BatchNorm output: :func:`bn_act` with ``defer_apply`` (the raw input
    plus its pending scale/bias), or with ``defer_res_relu`` (an unwritten output that no convolution took: the
    standalone apply + residual + ReLU kernel fills it in place, :class:`~polyaxon_amd.ops.conv1x1.PendingApply`)."""
    if t is None:
        return t
    fill_pending(t)
    if not getattr(t, "_plx_deferred", False):
        return t
    return _Materialize.apply(t, t._plx_bn_link.affine)


def bn_act(x: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor, running_mean: Optional[torch.Tensor],
           running_var: Optional[torch.Tensor], training: bool, momentum: float, eps: float,
           residual: Optional[torch.Tensor], act: bool, ext_stats=None, residual_grad_box=None,
           residual_link: bool = False, defer_apply: bool = False, dx_sink=None,
           defer_res_relu: bool = False) -> torch.Tensor:
    """``ext_stats`` = (fp32 [2][nblk][C] channel sums / sums of squares of ``x``, nblk) from the op that
    produced ``x`` (the 1x1-conv GEMM epilogue); training mode then skips the stats pass.  ``residual_link``:
    ``residual`` is the output of a fused BatchNorm that nothing else consumes; its backward partials are then
    reduced by this op's dx pass, and with ``PLX_DS_BWD_FUSED`` (ops.conv1x1.ds_bwd_route) the backward writes no
    d_residual: that BatchNorm gets this op's incoming gradient and ReLU mask.  ``defer_apply`` (training, no
    activation, no residual): skip the apply pass and return ``x`` itself marked ``_plx_deferred``; the fused BatchNorm that takes it as its residual applies
    the scale/bias while adding (a ResNet downsampling branch: ~0.3 ms of a bs-256 step), any other consumer
    must call :func:`materialize` first.  ``dx_sink``: the :class:`~polyaxon_amd.ops.conv1x1.DxSink` the 1x1
    convolution that produced ``x`` attached to it; the backward then leaves its dx pass to that convolution's
    data-gradient GEMM whenever it has no d_residual tensor to write.  ``defer_res_relu`` (training, activation and
    residual): run the reduce / finalize only and return the *unwritten* output carrying ``_plx_pending`` (a
    :class:`~polyaxon_amd.ops.conv1x1.PendingApply`); the caller guarantees that the next reader is a native 1x1
    convolution, whose forward GEMM fills the output and the ReLU mask on the way (any other must call
    :func:`materialize` first)."""
    fill_pending(residual)  # a block output still pending (its convolution did not run first) is read below
    if residual is not None and residual.dtype != x.dtype:
        residual = residual.to(x.dtype)
    if training:
        link = BnLink()
        rlink = getattr(residual, "_plx_bn_link", None) if (residual_link and residual is not None) else None
        defer = bool(defer_apply) and not act and residual is None
        pend = [] if (defer_res_relu and act and residual is not None) else None
        y = _BNAct.apply(x, weight, bias, running_mean, running_var, residual, momentum, eps, act, ext_stats,
                         residual_grad_box, link, rlink, defer, dx_sink, pend)
        y._plx_bn_link = link
        if defer:
            y._plx_deferred = True
        if pend:
            y._plx_pending = pend[0]
        return y
    residual = materialize(residual)
    # inference: fold running stats into scale/bias, one apply pass
    lib = _native.lib("plx_bn")
    x = _cl(x)
    n, c, h, w = x.shape
    inv = torch.rsqrt(running_var.float() + eps)
    scale = weight.float() * inv
    sb = torch.cat([scale, bias.float() - running_mean.float() * scale]).contiguous()
    y = torch.empty_like(x, memory_format=torch.channels_last)
    res = _cl(residual) if residual is not None else None
    rc = lib.plx_bn_apply(x.data_ptr(), res.data_ptr() if res is not None else None, y.data_ptr(), n * h * w, c,
                          sb.data_ptr(), int(act), _stream())
    _native.check(rc, "plx_bn_apply")
    return y
