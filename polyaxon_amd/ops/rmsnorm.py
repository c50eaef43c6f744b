"""RMSNorm and LayerNorm: fused HIP kernels (csrc/rmsnorm.hip) for bf16 CUDA tensors (bf16 in and out, fp32
statistics and parameters), PyTorch composition otherwise.  The fused add + norm pairs also carry residual dropout
(``drop=``, ops/dropout.py), and :func:`dropout` is its standalone pass."""
from __future__ import annotations

import os

import torch

from polyaxon_amd.ops import _native, side_stream

# the norms' parameter-gradient reduction on the side stream (ops/side_stream.py) when every parameter has a
# first-written flat slot and the side stream is in use this backward: only the optimizer / FlatDDP read those, after
# side_stream.join / fence
# (PLX_LM_WGRAD_STREAM=0: inline, as ops/lm.py)
_SIDE = os.environ.get("PLX_LM_WGRAD_STREAM", "1") != "0"


def rms_norm_reference(x: torch.Tensor, weight: torch.Tensor, eps: float) -> torch.Tensor:
    xf = x.float()
    y = xf * torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + eps) * weight.float()
    return y.to(x.dtype)


def _stream() -> int:
    return _native.current_stream()


def _param_grads(parts, params, d: int):
    """Column sums of the backward kernel's fp32 [nb, d] partial matrices (one per parameter) in one launch
    (csrc/rmsnorm.hip plx_partial_colsum).  A parameter with a direct fp32 flat-gradient slot (ops/flat.py) gets its
    sum written -- or, for a slot already written this step, accumulated -- there and None is returned for it (no
    autograd ``grad += g`` kernel; FlatDDP still sees the parameter through its post-accumulate hook); otherwise the sum is
    returned in the parameter's dtype."""
    from polyaxon_amd.ops.flat import direct_grad

    lib = _native.lib("plx_rms")
    dev = parts[0].device
    nb = parts[0].shape[0]
    outs, accs, ret = [], [], []
    for p in params:
        slot = direct_grad(p)
        if (slot is not None and slot.dtype == torch.float32 and slot.is_contiguous() and slot.numel() == d
                and slot.device == dev):
            accs.append(int(p._plx_flat.mark_written(slot)))
            outs.append(slot)
            ret.append(None)
        else:
            t = torch.empty(d, dtype=torch.float32, device=dev)
            accs.append(0)
            outs.append(t)
            ret.append(t)
    nz = len(parts)

    def reduce():  # workspace and tickets of the stream it runs on
        l2 = torch.empty(int(lib.plx_partial_colsum_workspace(nb, d, nz)), dtype=torch.float32, device=dev)
        cnt = _native.counters(dev, f"plx_partial_colsum:{_stream()}")
        _native.check(lib.plx_partial_colsum(parts[0].data_ptr(), parts[-1].data_ptr(), nb, d, nz, l2.data_ptr(),
                                             cnt.data_ptr(), outs[0].data_ptr(), outs[-1].data_ptr(), accs[0],
                                             accs[-1], _stream()), "plx_partial_colsum")
    # only beside side-stream work this backward already queued (GPT-2's weight gradients: +0.4 %,
    # r6_lm_norm_side_ab.jsonl); alone on it (Llama-3 8B, whose weight gradients stay inline) it cost 0.8 %
    # (r6_lm_norm_side_llama_ab.jsonl)
    if _SIDE and side_stream.busy(dev) and all(r is None for r in ret) and not any(accs):
        side_stream.run(reduce, parts, dev)
    else:
        reduce()
    return [r if r is None else r.to(p.dtype) for r, p in zip(ret, params)]


# ------------------------------------------------------------------------------------------ residual dropout
def _drop_args(state, site):
    return state.hp.data_ptr(), state.step_counter.data_ptr(), int(site)


def _drop_supported(x: torch.Tensor) -> bool:
    return x.is_cuda and x.dtype == torch.bfloat16 and x.numel() > 0 and x.numel() % 8 == 0 and x.is_contiguous()


def _drop_launch(x: torch.Tensor, state, site) -> torch.Tensor:
    y = torch.empty_like(x)
    _native.check(_native.lib("plx_rms").plx_dropout(x.data_ptr(), y.data_ptr(), x.numel() // 8,
                                                     *_drop_args(state, site), _stream()), "plx_dropout")
    return y


def _drop_grad(g, state, site):
    """The gradient of a dropped-out branch from the gradient ``g`` of its output (None stays None)."""
    if g is None:
        return None
    return _drop_launch(g.contiguous(), state, site)


class _Dropout(torch.autograd.Function):
    """y = keep ? c * x : 0 (csrc/rmsnorm.hip plx_dropout); the backward is the same kernel on dy at the same step."""

    @staticmethod
    def forward(ctx, x, state, site):
        ctx.drop = (state, site)
        return _drop_launch(x, state, site)

    @staticmethod
    def backward(ctx, dy):
        return _drop_launch(dy.contiguous().to(torch.bfloat16), *ctx.drop), None, None


def drop_factor(like: torch.Tensor, state, site) -> torch.Tensor:
    """fp32, shaped like ``like``: c where the element is kept, 0 where it is dropped -- the kernels' mask from its
    numpy twin (ops/dropout.py mask_reference) at the step the device counter holds now (one host read of it)."""
    from polyaxon_amd.ops import dropout as _drop

    n = like.numel()
    keep = _drop.mask_reference(state.key, state.step(), int(site), (n + 7) // 8, state.T).reshape(-1)[:n]
    return torch.from_numpy(keep.astype("float32")).to(like.device).view(like.shape) * state.c


def dropout(x: torch.Tensor, state, site: int) -> torch.Tensor:
    """Dropout of site ``site`` of ``state`` (ops/dropout.py DropoutState): the HIP pass for contiguous bf16 GPU
    tensors of a multiple of 8 elements, the same formula in torch with the same mask otherwise."""
    if _drop_supported(x):
        return _Dropout.apply(x, state, site)
    return (x.float() * drop_factor(x, state, site)).to(x.dtype)


def _drop_add_reference(x: torch.Tensor, res: torch.Tensor, state, site) -> torch.Tensor:
    """s = x + drop(res) where the fused kernels do not apply: the standalone pass and a separate add on the GPU, the
    contract's one-rounding formula in torch otherwise."""
    if _drop_supported(res) and res.dtype == x.dtype:
        return x + _Dropout.apply(res, state, site)
    return (x.float() + drop_factor(res, state, site) * res.float()).to(x.dtype)


class _RMSNorm(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, eps):
        lib = _native.lib("plx_rms")
        x = x.contiguous()
        d = x.shape[-1]
        rows = x.numel() // d
        y = torch.empty_like(x)
        rstd = torch.empty(rows, dtype=torch.float32, device=x.device)
        w = weight.float().contiguous()
        _native.check(lib.plx_rms_forward(x.data_ptr(), w.data_ptr(), y.data_ptr(), rstd.data_ptr(), rows, d,
                                          float(eps), _stream()), "plx_rms_forward")
        ctx.save_for_backward(x, w, rstd)
        ctx.param = weight
        return y

    @staticmethod
    def backward(ctx, dy):
        lib = _native.lib("plx_rms")
        x, w, rstd = ctx.saved_tensors
        dy = dy.contiguous().to(x.dtype)
        d = x.shape[-1]
        rows = x.numel() // d
        dx = torch.empty_like(x)
        nb = lib.plx_rms_bwd_blocks(rows)
        part = torch.empty((nb, d), dtype=torch.float32, device=x.device)
        _native.check(lib.plx_rms_backward(x.data_ptr(), w.data_ptr(), dy.data_ptr(), rstd.data_ptr(), dx.data_ptr(),
                                           part.data_ptr(), rows, d, _stream()), "plx_rms_backward")
        return dx, _param_grads([part], [ctx.param], d)[0], None


class _AddRMSNorm(torch.autograd.Function):
    """(s, y) = (x + res, RMSNorm(x + res)) in one pass (csrc/rmsnorm.hip plx_add_rms_forward); backward: the norm's
    dx plus the residual gradient ds in one pass, returned for both x and res."""

    @staticmethod
    def forward(ctx, x, res, weight, eps):
        ctx.set_materialize_grads(False)
        lib = _native.lib("plx_rms")
        d = x.shape[-1]
        rows = x.numel() // d
        s, y = torch.empty_like(x), torch.empty_like(x)
        rstd = torch.empty(rows, dtype=torch.float32, device=x.device)
        w = weight.float().contiguous()
        _native.check(lib.plx_add_rms_forward(x.data_ptr(), res.data_ptr(), w.data_ptr(), s.data_ptr(), y.data_ptr(),
                                              rstd.data_ptr(), rows, d, float(eps), _stream()), "plx_add_rms_forward")
        ctx.save_for_backward(s, w, rstd)
        ctx.param = weight
        return s, y

    @staticmethod
    def backward(ctx, ds, dy):
        lib = _native.lib("plx_rms")
        s, w, rstd = ctx.saved_tensors
        if dy is None:
            return ds, ds, None, None
        d = s.shape[-1]
        rows = s.numel() // d
        dy = dy.contiguous().to(s.dtype)
        dx = torch.empty_like(s)
        part = torch.empty((lib.plx_rms_bwd_blocks(rows), d), dtype=torch.float32, device=s.device)
        if ds is None:
            _native.check(lib.plx_rms_backward(s.data_ptr(), w.data_ptr(), dy.data_ptr(), rstd.data_ptr(), dx.data_ptr(),
                                               part.data_ptr(), rows, d, _stream()), "plx_rms_backward")
        else:
            ds = ds.contiguous().to(s.dtype)
            _native.check(lib.plx_add_rms_backward(s.data_ptr(), w.data_ptr(), dy.data_ptr(), rstd.data_ptr(),
                                                   ds.data_ptr(), dx.data_ptr(), part.data_ptr(), rows, d, _stream()),
                          "plx_add_rms_backward")
        return dx, dx, _param_grads([part], [ctx.param], d)[0], None


class _AddRMSNormDrop(torch.autograd.Function):
    """:class:`_AddRMSNorm` with residual dropout on ``res`` (csrc/rmsnorm.hip plx_add_rms_drop_*): s = x + drop(res);
    the backward regenerates the mask from the step counter and returns dx for x and its dropped-out copy for res."""

    @staticmethod
    def forward(ctx, x, res, weight, eps, state, site):
        ctx.set_materialize_grads(False)
        lib = _native.lib("plx_rms")
        d = x.shape[-1]
        rows = x.numel() // d
        s, y = torch.empty_like(x), torch.empty_like(x)
        rstd = torch.empty(rows, dtype=torch.float32, device=x.device)
        w = weight.float().contiguous()
        _native.check(lib.plx_add_rms_drop_forward(x.data_ptr(), res.data_ptr(), w.data_ptr(), s.data_ptr(),
                                                   y.data_ptr(), rstd.data_ptr(), rows, d, float(eps),
                                                   *_drop_args(state, site), _stream()), "plx_add_rms_drop_forward")
        ctx.save_for_backward(s, w, rstd)
        ctx.param, ctx.drop = weight, (state, site)
        return s, y

    @staticmethod
    def backward(ctx, ds, dy):
        lib = _native.lib("plx_rms")
        s, w, rstd = ctx.saved_tensors
        if dy is None:
            return ds, _drop_grad(ds, *ctx.drop), None, None, None, None
        d = s.shape[-1]
        rows = s.numel() // d
        dy = dy.contiguous().to(s.dtype)
        ds = None if ds is None else ds.contiguous().to(s.dtype)
        dx, dres = torch.empty_like(s), torch.empty_like(s)
        part = torch.empty((lib.plx_rms_bwd_blocks(rows), d), dtype=torch.float32, device=s.device)
        _native.check(lib.plx_add_rms_drop_backward(s.data_ptr(), w.data_ptr(), dy.data_ptr(), rstd.data_ptr(),
                                                    None if ds is None else ds.data_ptr(), dx.data_ptr(),
                                                    dres.data_ptr(), part.data_ptr(), rows, d, *_drop_args(*ctx.drop),
                                                    _stream()), "plx_add_rms_drop_backward")
        return dx, dres, _param_grads([part], [ctx.param], d)[0], None, None, None


def add_rms_norm(x: torch.Tensor, res: torch.Tensor, weight: torch.Tensor, eps: float = 1e-5, drop=None):
    """(s, y) = (x + res, RMSNorm(s)): the pre-norm residual add fused into the next RMSNorm for bf16 GPU rows; the
    separate add and :func:`rms_norm` otherwise.  ``drop = (state, site)``: residual dropout on ``res`` first
    (ops/dropout.py), inside the same kernels."""
    fused = supported(x) and res.dtype == x.dtype and res.shape == x.shape and x.is_contiguous() and res.is_contiguous()
    if drop is not None:
        if fused:
            return _AddRMSNormDrop.apply(x, res, weight, eps, *drop)
        s = _drop_add_reference(x, res, *drop)
        return s, rms_norm(s, weight, eps)
    if fused:
        return _AddRMSNorm.apply(x, res, weight, eps)
    s = x + res
    return s, rms_norm(s, weight, eps)


def supported(x: torch.Tensor) -> bool:
    d = x.shape[-1]
    return x.is_cuda and x.dtype == torch.bfloat16 and d % 8 == 0 and d <= 8192


def rms_norm(x: torch.Tensor, weight: torch.Tensor, eps: float = 1e-5) -> torch.Tensor:
    if x.is_cuda and x.dtype != torch.bfloat16 and torch.is_autocast_enabled("cuda"):
        x = x.to(torch.bfloat16)
    if supported(x):
        return _RMSNorm.apply(x, weight, eps)
    return rms_norm_reference(x, weight, eps)


def layer_norm_reference(x: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor, eps: float) -> torch.Tensor:
    if x.is_cuda and x.dtype != weight.dtype:
        # the types the fused path takes (bf16 rows, fp32 parameters) at a width it does not: F.layer_norm on the GPU
        # wants one dtype and raises outside autocast; fp32 math and the input's dtype out, as rms_norm_reference
        y = torch.nn.functional.layer_norm(x.float(), (x.shape[-1],), weight.float(), bias.float(), eps)
        return y.to(x.dtype)
    return torch.nn.functional.layer_norm(x, (x.shape[-1],), weight, bias, eps)


class _LayerNorm(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, eps):
        lib = _native.lib("plx_rms")
        x = x.contiguous()
        d = x.shape[-1]
        rows = x.numel() // d
        y = torch.empty_like(x)
        mean = torch.empty(rows, dtype=torch.float32, device=x.device)
        rstd = torch.empty(rows, dtype=torch.float32, device=x.device)
        w, b = weight.float().contiguous(), bias.float().contiguous()
        _native.check(lib.plx_ln_forward(x.data_ptr(), w.data_ptr(), b.data_ptr(), y.data_ptr(), mean.data_ptr(),
                                         rstd.data_ptr(), rows, d, float(eps), _stream()), "plx_ln_forward")
        ctx.save_for_backward(x, w, mean, rstd)
        ctx.params = (weight, bias)
        return y

    @staticmethod
    def backward(ctx, dy):
        lib = _native.lib("plx_rms")
        x, w, mean, rstd = ctx.saved_tensors
        dy = dy.contiguous().to(x.dtype)
        d = x.shape[-1]
        rows = x.numel() // d
        dx = torch.empty_like(x)
        nb = lib.plx_ln_bwd_blocks(rows, d)
        part = torch.empty((2, nb, d), dtype=torch.float32, device=x.device)
        _native.check(lib.plx_ln_backward(x.data_ptr(), w.data_ptr(), dy.data_ptr(), mean.data_ptr(), rstd.data_ptr(),
                                          dx.data_ptr(), part[0].data_ptr(), part[1].data_ptr(), rows, d, _stream()),
                      "plx_ln_backward")
        dw, db = _param_grads([part[0], part[1]], list(ctx.params), d)
        return dx, dw, db, None


def layer_norm(x: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor, eps: float = 1e-5) -> torch.Tensor:
    """LayerNorm over the last dim.  Under bf16 autocast the input is taken as bf16 and the output stays bf16 (what
    the next GEMM reads); the fused kernels need d % 8 == 0 and d <= 8192."""
    if x.is_cuda and x.dtype != torch.bfloat16 and torch.is_autocast_enabled("cuda"):
        x = x.to(torch.bfloat16)
    if supported(x):
        return _LayerNorm.apply(x, weight, bias, eps)
    return layer_norm_reference(x, weight, bias, eps)


class _AddLayerNorm(torch.autograd.Function):
    """(s, y) = (x + res, LayerNorm(x + res)) in one pass (csrc/rmsnorm.hip plx_add_ln_forward); backward: the norm's
    dx plus the residual gradient ds in one pass, returned for both x and res."""

    @staticmethod
    def forward(ctx, x, res, weight, bias, eps):
        ctx.set_materialize_grads(False)
        lib = _native.lib("plx_rms")
        d = x.shape[-1]
        rows = x.numel() // d
        s, y = torch.empty_like(x), torch.empty_like(x)
        mean = torch.empty(rows, dtype=torch.float32, device=x.device)
        rstd = torch.empty(rows, dtype=torch.float32, device=x.device)
        w, b = weight.float().contiguous(), bias.float().contiguous()
        _native.check(lib.plx_add_ln_forward(x.data_ptr(), res.data_ptr(), w.data_ptr(), b.data_ptr(), s.data_ptr(),
                                             y.data_ptr(), mean.data_ptr(), rstd.data_ptr(), rows, d, float(eps),
                                             _stream()), "plx_add_ln_forward")
        ctx.save_for_backward(s, w, mean, rstd)
        ctx.params = (weight, bias)
        return s, y

    @staticmethod
    def backward(ctx, ds, dy):
        lib = _native.lib("plx_rms")
        s, w, mean, rstd = ctx.saved_tensors
        d = s.shape[-1]
        rows = s.numel() // d
        if dy is None:  # only the residual stream is used downstream
            return ds, ds, None, None, None
        dy = dy.contiguous().to(s.dtype)
        dx = torch.empty_like(s)
        nb = lib.plx_ln_bwd_blocks(rows, d)
        part = torch.empty((2, nb, d), dtype=torch.float32, device=s.device)
        if ds is None:
            _native.check(lib.plx_ln_backward(s.data_ptr(), w.data_ptr(), dy.data_ptr(), mean.data_ptr(),
                                              rstd.data_ptr(), dx.data_ptr(), part[0].data_ptr(), part[1].data_ptr(),
                                              rows, d, _stream()), "plx_ln_backward")
        else:
            ds = ds.contiguous().to(s.dtype)
            _native.check(lib.plx_add_ln_backward(s.data_ptr(), w.data_ptr(), dy.data_ptr(), mean.data_ptr(),
                                                  rstd.data_ptr(), ds.data_ptr(), dx.data_ptr(), part[0].data_ptr(),
                                                  part[1].data_ptr(), rows, d, _stream()), "plx_add_ln_backward")
        dw, db = _param_grads([part[0], part[1]], list(ctx.params), d)
        return dx, dx, dw, db, None


class _AddLayerNormDrop(torch.autograd.Function):
    """:class:`_AddLayerNorm` with residual dropout on ``res`` (csrc/rmsnorm.hip plx_add_ln_drop_*): s = x + drop(res);
    the backward regenerates the mask from the step counter and returns dx for x and its dropped-out copy for res."""

    @staticmethod
    def forward(ctx, x, res, weight, bias, eps, state, site):
        ctx.set_materialize_grads(False)
        lib = _native.lib("plx_rms")
        d = x.shape[-1]
        rows = x.numel() // d
        s, y = torch.empty_like(x), torch.empty_like(x)
        mean = torch.empty(rows, dtype=torch.float32, device=x.device)
        rstd = torch.empty(rows, dtype=torch.float32, device=x.device)
        w, b = weight.float().contiguous(), bias.float().contiguous()
        _native.check(lib.plx_add_ln_drop_forward(x.data_ptr(), res.data_ptr(), w.data_ptr(), b.data_ptr(),
                                                  s.data_ptr(), y.data_ptr(), mean.data_ptr(), rstd.data_ptr(), rows, d,
                                                  float(eps), *_drop_args(state, site), _stream()),
                      "plx_add_ln_drop_forward")
        ctx.save_for_backward(s, w, mean, rstd)
        ctx.params, ctx.drop = (weight, bias), (state, site)
        return s, y

    @staticmethod
    def backward(ctx, ds, dy):
        lib = _native.lib("plx_rms")
        s, w, mean, rstd = ctx.saved_tensors
        d = s.shape[-1]
        rows = s.numel() // d
        if dy is None:  # only the residual stream is used downstream
            return ds, _drop_grad(ds, *ctx.drop), None, None, None, None, None
        dy = dy.contiguous().to(s.dtype)
        ds = None if ds is None else ds.contiguous().to(s.dtype)
        dx, dres = torch.empty_like(s), torch.empty_like(s)
        nb = lib.plx_ln_bwd_blocks(rows, d)
        part = torch.empty((2, nb, d), dtype=torch.float32, device=s.device)
        _native.check(lib.plx_add_ln_drop_backward(s.data_ptr(), w.data_ptr(), dy.data_ptr(), mean.data_ptr(),
                                                   rstd.data_ptr(), None if ds is None else ds.data_ptr(),
                                                   dx.data_ptr(), dres.data_ptr(), part[0].data_ptr(),
                                                   part[1].data_ptr(), rows, d, *_drop_args(*ctx.drop), _stream()),
                      "plx_add_ln_drop_backward")
        dw, db = _param_grads([part[0], part[1]], list(ctx.params), d)
        return dx, dres, dw, db, None, None, None


def add_layer_norm(x: torch.Tensor, res: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor,
                   eps: float = 1e-5, drop=None):
    """(s, y) = (x + res, LayerNorm(s)): the pre-norm transformer's residual add fused into the next norm for bf16 GPU
    rows of d <= 1024 (one wave per row); the separate add and :func:`layer_norm` otherwise.  ``drop = (state, site)``:
    residual dropout on ``res`` first (ops/dropout.py) -- inside the same kernels where they apply, the standalone
    :func:`dropout` pass before the separate add above d = 1024."""
    fused = (supported(x) and res.dtype == x.dtype and res.shape == x.shape and x.shape[-1] <= 1024
             and x.is_contiguous() and res.is_contiguous())
    if drop is not None:
        if fused:
            return _AddLayerNormDrop.apply(x, res, weight, bias, eps, *drop)
        s = _drop_add_reference(x, res, *drop)
        return s, layer_norm(s, weight, bias, eps)
    if fused:
        return _AddLayerNorm.apply(x, res, weight, bias, eps)
    s = x + res
    return s, layer_norm(s, weight, bias, eps)


class LayerNorm(torch.nn.Module):
    """``nn.LayerNorm(d)`` (same parameter names, fp32 weight / bias) on the fused kernels for bf16 GPU inputs."""

    def __init__(self, d: int, eps: float = 1e-5):
        super().__init__()
        self.eps = eps
        self.normalized_shape = (d,)
        self.weight = torch.nn.Parameter(torch.ones(d))
        self.bias = torch.nn.Parameter(torch.zeros(d))

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return layer_norm(x, self.weight, self.bias, self.eps)
