"""Mixture-of-experts feed-forward on the grouped MFMA GEMM (csrc/gemm_grouped.hip).

A token goes to ``top_k`` of ``E`` experts.  :func:`plan` sorts the (token, choice) pairs by expert into a packed
order; :func:`gather` copies the token rows into it, two :func:`grouped_linear` ops with the activation between them
run every expert's MLP on its own segment in ONE launch each, and :func:`combine` sums a token's ``k`` results with
its gates.  The segment sizes never leave the device: ``offs`` is read by the kernels, no launch depends on it, and
``plan`` is sync-free torch, so the whole layer sits inside a captured step and follows the router from replay to
replay.

``grouped_linear``'s three GEMMs: forward and data gradient in the kernel's rows mode (M-tiles that never cross a
segment), the weight gradient in its reduce mode (an expert's tokens are its K range).  Everything is deterministic:
no atomics, a fixed summation order.

CPU tensors, fp32 / fp64 tensors and shapes the kernel refuses (``gemm.grouped_supported``) run a reference path -- a
loop over the experts with ``F.linear`` in (at least) fp32 -- which reads the segment sizes on the host.
"""
from __future__ import annotations

from typing import Tuple

import torch
import torch.nn.functional as F

from polyaxon_amd.ops import _native, gemm
from polyaxon_amd.ops import lm as lm_ops

ACTS = ("swiglu", "gelu")


def plan(ids: torch.Tensor, E: int) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """``ids`` [T, k] (expert of each of a token's k choices) -> ``(offs [E + 1], token_of [P], slot_of [T, k])``, all
    int32, P = T k: the pairs in a STABLE sort by expert (a counting sort: a pair's place is its expert's start plus
    the number of earlier pairs of that expert), so inside a segment the rows are in token order.  Packed row p holds
    token ``token_of[p]``; choice j of token t sits in packed row ``slot_of[t, j]``.  No host read, no op whose output
    size depends on the data: it runs inside a captured step."""
    T, k = ids.shape
    flat = ids.reshape(-1).long()
    # [E, P], scanned along its contiguous dimension: pairs of expert e up to and including this one
    seen = (torch.arange(E, device=ids.device)[:, None] == flat[None, :]).to(torch.int32).cumsum(1)
    offs = torch.zeros(E + 1, dtype=torch.int64, device=ids.device)
    offs[1:] = seen[:, -1].cumsum(0)
    slot = offs[flat] + seen.gather(0, flat[None, :]).squeeze(0) - 1
    token_of = torch.empty(T * k, dtype=torch.int32, device=ids.device)
    token_of.scatter_(0, slot, (torch.arange(T * k, device=ids.device) // k).to(torch.int32))
    return offs.to(torch.int32), token_of, slot.to(torch.int32).view(T, k)


def _stream() -> int:
    return _native.current_stream()


def _lib():
    return _native.lib("plx_gemm_grouped")


def _native_rows(x: torch.Tensor) -> bool:
    return x.is_cuda and x.dtype == torch.bfloat16 and x.dim() == 2 and x.shape[1] % 8 == 0 and x.shape[0] > 0


# ------------------------------------------------------------------------------------------------ gather / combine
def _gather_rows(x, idx, scale, P):
    out = torch.empty(P, x.shape[1], dtype=x.dtype, device=x.device)
    _native.check(_lib().plx_moe_gather(x.data_ptr(), idx.data_ptr(), None if scale is None else scale.data_ptr(),
                                        out.data_ptr(), P, x.shape[0], x.shape[1], _stream()), "plx_moe_gather")
    return out


def _combine_rows(yp, slot_of, gates):
    T, k = slot_of.shape
    y = torch.empty(T, yp.shape[1], dtype=yp.dtype, device=yp.device)
    _native.check(_lib().plx_moe_combine(yp.data_ptr(), slot_of.data_ptr(), None if gates is None else gates.data_ptr(),
                                         y.data_ptr(), T, k, yp.shape[0], yp.shape[1], _stream()), "plx_moe_combine")
    return y


class _Gather(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, token_of, slot_of):
        ctx.save_for_backward(slot_of)
        return _gather_rows(x.contiguous(), token_of, None, token_of.numel())

    @staticmethod
    def backward(ctx, dxp):
        (slot_of,) = ctx.saved_tensors
        return _combine_rows(dxp.contiguous(), slot_of, None), None, None  # dx[t] = sum_j dxp[slot_of[t][j]]


class _Combine(torch.autograd.Function):
    @staticmethod
    def forward(ctx, yp, gates, token_of, slot_of):
        yp, gates = yp.contiguous(), gates.contiguous()
        ctx.save_for_backward(yp, gates, token_of, slot_of)
        return _combine_rows(yp, slot_of, gates)

    @staticmethod
    def backward(ctx, dy):
        yp, gates, token_of, slot_of = ctx.saved_tensors
        dy = dy.contiguous()
        T, k = slot_of.shape
        P = yp.shape[0]
        packed = torch.empty(P, dtype=torch.float32, device=dy.device)
        packed.scatter_(0, slot_of.reshape(-1).long(), gates.reshape(-1))  # the gate of each packed row
        dyp = _gather_rows(dy, token_of, packed, P)
        dgates = torch.empty(T, k, dtype=torch.float32, device=dy.device)
        _native.check(_lib().plx_moe_gate_grad(dy.data_ptr(), yp.data_ptr(), slot_of.data_ptr(), dgates.data_ptr(), T, k,
                                               P, yp.shape[1], _stream()), "plx_moe_gate_grad")
        return dyp, dgates, None, None


def gather(x: torch.Tensor, token_of: torch.Tensor, slot_of: torch.Tensor) -> torch.Tensor:
    """xp[p] = x[token_of[p]] (x [T, D]); its backward sums a token's k packed gradients in fixed order"""
    if _native_rows(x):
        return _Gather.apply(x, token_of, slot_of)
    return x[token_of.long()]


def combine(yp: torch.Tensor, gates: torch.Tensor, token_of: torch.Tensor, slot_of: torch.Tensor) -> torch.Tensor:
    """y[t] = sum_j gates[t, j] * yp[slot_of[t, j]], j in order, summed in fp32 (``gates`` fp32 [T, k])"""
    if _native_rows(yp):
        return _Combine.apply(yp, gates.float(), token_of, slot_of)
    ct = torch.promote_types(yp.dtype, torch.float32)
    return (yp[slot_of.long()].to(ct) * gates.to(ct)[..., None]).sum(1).to(yp.dtype)


# ------------------------------------------------------------------------------------------------ grouped linear
class _GroupedLinear(torch.autograd.Function):
    @staticmethod
    def forward(ctx, xp, weight, offs):
        xp = xp.contiguous()
        E, N, K = weight.shape
        ctx.save_for_backward(xp, weight, offs)
        return gemm.grouped_rows(xp, weight, offs, N, K, True)

    @staticmethod
    def backward(ctx, dy):
        xp, weight, offs = ctx.saved_tensors
        E, N, K = weight.shape
        dy = dy.contiguous()
        dx = dw = None
        if ctx.needs_input_grad[0]:  # dx[p][k] = sum_n dy[p][n] W_e[n][k]: W_e is the MN-major operand as stored
            dx = gemm.grouped_rows(dy, weight, offs, K, N, False)
        if ctx.needs_input_grad[1]:  # dW_e[n][k] = sum over the segment of dy[p][n] xp[p][k]
            dw = gemm.grouped_wgrad(dy, xp, offs, E)
        return dx, dw, None


def _grouped_linear_reference(xp, weight, offs):
    ct = torch.promote_types(xp.dtype, torch.float32)
    o = offs.tolist()
    parts = [F.linear(xp[o[e]:o[e + 1]].to(ct), weight[e].to(ct)) for e in range(weight.shape[0])]
    return torch.cat(parts, 0).to(xp.dtype)


def grouped_supported(xp: torch.Tensor, weight: torch.Tensor) -> bool:
    return (_native_rows(xp) and weight.is_cuda and weight.dtype == torch.bfloat16 and weight.dim() == 3
            and weight.is_contiguous() and xp.shape[1] == weight.shape[2]
            and gemm.grouped_supported(xp.shape[0], *weight.shape))


def grouped_linear(xp: torch.Tensor, weight: torch.Tensor, offs: torch.Tensor) -> torch.Tensor:
    """y[p] = weight[e] xp[p] for the packed rows p of segment e (``offs`` int32 [E + 1], ``offs[E]`` = P): weight
    [E, N, K], xp [P, K] -> [P, N].  bf16 CUDA tensors run the grouped kernel, forward and both gradients."""
    if grouped_supported(xp, weight):
        return _GroupedLinear.apply(xp, weight, offs)
    return _grouped_linear_reference(xp, weight, offs)


# ------------------------------------------------------------------------------------------------ the layer
def route(x: torch.Tensor, router_w: torch.Tensor, top_k: int):
    """``(ids [T, k], gates [T, k], aux)``: the router in fp32 (wider when x is) -- softmax of x W_r^T, the top-k
    experts, their probabilities renormalised over the k chosen -- and the Switch load-balance term
    E sum_e f_e mean_t P[t][e] with f_e the fraction of the T k choices that went to expert e."""
    ct = torch.promote_types(x.dtype, torch.float32)
    E = router_w.shape[0]
    with torch.autocast(x.device.type, enabled=False):
        probs = torch.softmax(x.to(ct) @ router_w.to(ct).t(), dim=-1)
        top, ids = probs.topk(top_k, dim=-1)
        gates = top / top.sum(-1, keepdim=True)
        frac = (ids[..., None] == torch.arange(E, device=ids.device)).to(ct).sum((0, 1)) / ids.numel()
        aux = E * (frac * probs.mean(0)).sum()
    return ids, gates, aux


def _activation(h: torch.Tensor, act: str) -> torch.Tensor:
    if act == "swiglu":
        return lm_ops.swiglu(h)
    return F.gelu(h, approximate="tanh")


def experts(x: torch.Tensor, ids: torch.Tensor, gates: torch.Tensor, w_up: torch.Tensor, w_down: torch.Tensor,
            act: str = "swiglu") -> torch.Tensor:
    """The expert MLPs for a fixed routing: x [T, d], ids / gates [T, k], w_up [E, F or 2 F, d], w_down [E, d, F]
    (no biases) -> [T, d].  Under CUDA autocast fp32 operands are computed from as bf16, as ``F.linear`` would."""
    if act not in ACTS:
        raise ValueError(f"unknown activation {act!r}; known: {ACTS}")
    if x.is_cuda and torch.is_autocast_enabled("cuda"):
        lp = torch.get_autocast_dtype("cuda")
        x, w_up, w_down = x.to(lp), w_up.to(lp), w_down.to(lp)
    offs, token_of, slot_of = plan(ids, w_up.shape[0])
    xp = gather(x, token_of, slot_of)
    h = _activation(grouped_linear(xp, w_up, offs), act)
    return combine(grouped_linear(h, w_down, offs), gates, token_of, slot_of)


def moe_mlp(x: torch.Tensor, router_w: torch.Tensor, w_up: torch.Tensor, w_down: torch.Tensor, top_k: int = 2,
            act: str = "swiglu") -> Tuple[torch.Tensor, torch.Tensor]:
    """``(y, aux)`` for x [..., d]: :func:`route`, then :func:`experts`"""
    x2 = x.reshape(-1, x.shape[-1])
    ids, gates, aux = route(x2, router_w, top_k)
    return experts(x2, ids, gates, w_up, w_down, act).view(x.shape), aux
