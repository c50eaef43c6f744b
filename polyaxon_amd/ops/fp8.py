"""FP8 GEMMs of the transformer linears with per-tensor scales kept on the device (csrc/gemm_fp8.hip).

A bf16 tensor is quantised in two launches: ``plx_fp8_amax`` leaves amax, ``scale`` and ``1 / scale`` in three fp32
device words, ``plx_fp8_cast`` reads the tensor once and writes its FP8 bytes row-major and transposed, so every GEMM
of a layer -- forward, data gradient, weight gradient -- sees K-contiguous operands.  The scale is a power of two,
``2^floor(log2(FMAX / amax))`` (:func:`scale_for`; 1 when amax is 0 or not finite): multiplying by it and by its
inverse is exact, so data already representable in the format survives quantisation unchanged.  ``plx_gemm_fp8`` takes
POINTERS to the two inverse scales and applies them in its epilogue: nothing is read back to the host and a captured
step stays valid.  Activations and weights use E4M3, output gradients E5M2 (the GEMM's A operand takes either).

The second recipe, ``mx`` (the ``mx_*`` functions at the end, csrc/gemm_mxfp8.hip), applies the same scale rule per
block of 32 K-values: one cast pass computes the scales with the data, and the MFMA applies them.

Names, constants and :func:`scale_for` are pure Python: polyflow/programs.py reads the key from here, and the
scheduler process that imports it never loads torch.  Everything else imports torch when called.
"""
from __future__ import annotations

import math
from typing import Any, Dict, Optional

KEYS = ("fp8",)

E4M3, E5M2 = 0, 1  # the kernels' format codes
FMAX = {E4M3: 448.0, E5M2: 57344.0}
_ws: Dict[Any, Any] = {}


def _fmt(fmt: int) -> int:
    if fmt not in FMAX:
        raise ValueError(f"unknown FP8 format {fmt!r} (E4M3 = {E4M3}, E5M2 = {E5M2})")
    return fmt


def validate(key: str, value: Any) -> bool:
    """The program param ``fp8`` as a bool; ValueError for anything that is not one."""
    if key not in KEYS:
        raise KeyError(key)
    if not isinstance(value, bool):
        raise ValueError(f"{key} must be true or false, got {value!r}")
    return value


def scale_for(amax: float, fmt: int) -> float:
    """The kernel's scale rule on the host: 2^floor(log2(FMAX / amax)), capped at 2^126 so its inverse is a normal
    number; 1 when ``amax`` is 0 or not finite."""
    a = abs(float(amax))
    if a == 0.0 or not math.isfinite(a):
        return 1.0
    a = max(a, 2.0 ** -149)  # fp32's smallest magnitude
    _, ex = math.frexp(FMAX[_fmt(fmt)] / a)  # q = m 2^ex, m in [0.5, 1)
    return 2.0 ** min(ex - 1, 126)


def supported(M: int, N: int, K: int) -> bool:
    """csrc/gemm_fp8.hip: every dimension a positive multiple of 16 (16-byte chunks never straddle a matrix edge)"""
    return M > 0 and N > 0 and K > 0 and M % 16 == 0 and N % 16 == 0 and K % 16 == 0


def _torch_dtype(fmt: int):
    import torch

    return torch.float8_e5m2 if _fmt(fmt) == E5M2 else torch.float8_e4m3fn


def quantize_reference(t, fmt: int):
    """(values, inv_scale) of the fake-quantised ``t``: the kernels' scale rule, a round trip through torch's float8
    dtype, the FP8 values (still scaled) as fp32 and 1 / scale as a float.  For CPU tensors and as the reference."""
    import torch

    x = t.detach().float()
    scale = scale_for(float(x.abs().max()) if x.numel() else 0.0, fmt)
    lim = FMAX[fmt]
    return torch.clamp(x * scale, -lim, lim).to(_torch_dtype(fmt)).float(), 1.0 / scale


def amax_scale(t, fmt: int):
    """fp32 device words [amax, scale, 1 / scale, -] of the bf16 CUDA tensor ``t`` (plx_fp8_amax)."""
    import torch

    from polyaxon_amd.ops import _native

    if not (t.is_cuda and t.dtype == torch.bfloat16 and t.is_contiguous() and t.numel() > 0 and t.numel() % 8 == 0):
        raise ValueError("plx_fp8_amax takes a contiguous bf16 CUDA tensor of a multiple of 8 elements")
    lib = _native.lib("plx_gemm_fp8")
    words = torch.empty(4, dtype=torch.float32, device=t.device)
    state = _native.counters(t.device, f"plx_fp8_amax:{_native.current_stream()}", 2)
    _native.check(lib.plx_fp8_amax(t.data_ptr(), t.numel(), _fmt(fmt), state.data_ptr(), words.data_ptr(),
                                   _native.current_stream()), "plx_fp8_amax")
    return words


def cast(t, words, fmt: int):
    """(q [R][C], qT [C][R]) uint8: the FP8 bytes of bf16 ``t`` [R][C] times ``words[1]`` (plx_fp8_cast)."""
    import torch

    from polyaxon_amd.ops import _native

    if t.dim() != 2 or t.shape[0] % 16 or t.shape[1] % 16 or not t.is_contiguous() or t.dtype != torch.bfloat16:
        raise ValueError(f"plx_fp8_cast takes a contiguous bf16 [R][C] with R, C multiples of 16, got {tuple(t.shape)}")
    R, C = t.shape
    q = torch.empty(R, C, dtype=torch.uint8, device=t.device)
    qt = torch.empty(C, R, dtype=torch.uint8, device=t.device)
    _native.check(_native.lib("plx_gemm_fp8").plx_fp8_cast(t.data_ptr(), q.data_ptr(), qt.data_ptr(), R, C, _fmt(fmt),
                                                           words.data_ptr(), _native.current_stream()), "plx_fp8_cast")
    return q, qt


def quantize(t, fmt: int):
    """(q, qT, inv_scale) of the bf16 CUDA matrix ``t``: its FP8 bytes row-major and transposed, and the device word
    holding 1 / scale (a one-element view of the words :func:`amax_scale` returns)."""
    words = amax_scale(t, fmt)
    q, qt = cast(t, words, fmt)
    return q, qt, words[2:3]


def _workspace(device, floats: int):
    import torch

    from polyaxon_amd.ops import _native

    return _native.cached(_ws, (device.type, device.index or 0, _native.current_stream()),
                          lambda: torch.empty(max(floats, 1 << 20), dtype=torch.float32, device=device),
                          ok=lambda w: w.numel() >= floats)


def gemm(a, a_fmt: int, ia, b, ib, M: int, N: int, K: int, out=None, accumulate: bool = False, alpha: float = 1.0,
         bias=None, gelu_out=None):
    """out[M][N] (bf16, unit column stride) = ia * ib * alpha * A . B^T (+ bias) (+ out): ``a`` FP8 bytes [M][K] of
    format ``a_fmt``, ``b`` E4M3 bytes [N][K], both contiguous uint8; ``ia`` / ``ib`` the one-element fp32 device
    tensors of their inverse scales.  ``bias`` [N] is added in fp32 (not with ``accumulate``); ``gelu_out``, laid out
    like ``out``, also receives gelu_tanh(out)."""
    import torch

    from polyaxon_amd.ops import _native

    if not supported(M, N, K):
        raise ValueError(f"the FP8 GEMM needs M, N, K > 0 and multiples of 16 (got {M}x{N}x{K})")
    for x, rows in ((a, M), (b, N)):
        if x.dtype != torch.uint8 or not x.is_contiguous() or x.numel() != rows * K:
            raise ValueError("the FP8 GEMM takes contiguous uint8 operands of M x K and N x K bytes")
    for s in (ia, ib):
        if s.dtype != torch.float32 or s.numel() != 1 or s.device != a.device:
            raise ValueError("ia / ib are one-element fp32 tensors on the operands' device")
    if out is None:
        if accumulate:
            raise ValueError("accumulate needs out")
        out = torch.empty(M, N, dtype=torch.bfloat16, device=a.device)
    if (out.dtype != torch.bfloat16 or out.dim() != 2 or out.shape != (M, N) or out.stride(1) != 1
            or out.stride(0) % 8 or out.data_ptr() % 16):
        raise ValueError("out must be a 16-byte aligned [M][N] bf16 matrix with unit column stride and a row stride "
                         "that is a multiple of 8")
    if bias is not None:
        if accumulate or bias.numel() != N:
            raise ValueError("bias needs numel N and no accumulate")
        bias = bias.to(torch.float32).contiguous()
        if bias.data_ptr() % 16:
            bias = bias.clone()
    if gelu_out is not None and (accumulate or gelu_out.dtype != torch.bfloat16 or gelu_out.shape != out.shape
                                 or gelu_out.stride() != out.stride() or gelu_out.data_ptr() % 16):
        raise ValueError("gelu_out must be a bf16 tensor laid out like out (and no accumulate)")
    floats = _native.size("plx_gemm_fp8", "plx_gemm_fp8_ws", M, N, K)
    ws = _workspace(a.device, floats).data_ptr() if floats else None
    rc = _native.lib("plx_gemm_fp8").plx_gemm_fp8(
        a.data_ptr(), b.data_ptr(), out.data_ptr(), ws, M, N, K, K, K, out.stride(0), _fmt(a_fmt), ia.data_ptr(),
        ib.data_ptr(), float(alpha), int(accumulate), bias.data_ptr() if bias is not None else None,
        gelu_out.data_ptr() if gelu_out is not None else None, _native.current_stream())
    if rc != 0:
        raise RuntimeError(f"plx_gemm_fp8 failed ({rc}) for {M}x{N}x{K}")
    return out


def linear_supported(x, weight) -> bool:
    """Do the three GEMMs of ``linear(x, weight)`` run on the FP8 kernel?  bf16 CUDA tensors, a contiguous weight,
    tokens, in and out multiples of 16."""
    import torch

    if not (x.is_cuda and x.dtype == torch.bfloat16 and weight.dtype == torch.bfloat16 and weight.is_contiguous()):
        return False
    return x.shape[-1] == weight.shape[1] and supported(x.numel() // x.shape[-1], weight.shape[0], weight.shape[1])


# ----------------------------------------------------------------------------- the "mx" recipe (csrc/gemm_mxfp8.hip)
# OCP microscaling: one E8M0 scale byte per 32 consecutive K-values of an operand row, applied by the MFMA itself.  A
# block's scale depends on its 32 values only, so ``plx_mxfp8_cast`` is one pass: no amax launch, no state words.
RECIPES = ("tensor", "mx")
MX_BLOCK = 32


def validate_recipe(value: Any) -> str:
    """The program param ``fp8_recipe`` as one of :data:`RECIPES`; ValueError for anything else."""
    if not isinstance(value, str) or value not in RECIPES:
        raise ValueError(f"fp8_recipe must be one of {RECIPES}, got {value!r}")
    return value


def mx_scale_byte(amax: float, fmt: int) -> int:
    """The E8M0 byte of a block whose amax is ``amax``: 127 - e with 2^e = :func:`scale_for` (the block's elements
    are x 2^e, its scale 2^(byte - 127)).  e <= 126 and bf16's range keep the byte in [1, 247]: never 255 (NaN)."""
    return 127 - (math.frexp(scale_for(amax, fmt))[1] - 1)


def mx_supported(M: int, N: int, K: int) -> bool:
    """csrc/gemm_mxfp8.hip: M and N positive multiples of 16, K a positive multiple of the 32-value block"""
    return M > 0 and N > 0 and K > 0 and M % 16 == 0 and N % 16 == 0 and K % MX_BLOCK == 0


def mx_quantize_reference(t, fmt: int):
    """(values, bytes) of ``t`` fake-quantised in blocks of 32 along its last dim (a ragged last block is padded with
    zeros): per block the kernels' scale rule, a round trip through torch's float8 dtype, and the values already
    multiplied back by the block scales, as fp32 shaped like ``t``; ``bytes`` [..., ceil(n / 32)] uint8 are the E8M0
    scale bytes.  For CPU tensors and as the reference."""
    import torch
    import torch.nn.functional as F

    x = t.detach().float()
    n = x.shape[-1]
    blocks = F.pad(x, (0, -n % MX_BLOCK)).unflatten(-1, (-1, MX_BLOCK))
    amax = blocks.abs().amax(-1).double()
    live = torch.isfinite(amax) & (amax > 0)
    # floor(log2(FMAX / amax)) from frexp: q = m 2^ex with m in [0.5, 1)
    _, ex = torch.frexp(FMAX[_fmt(fmt)] / torch.where(live, amax, torch.ones_like(amax)))
    e = torch.where(live, (ex - 1).clamp(max=126), torch.zeros_like(ex))
    scale = torch.ldexp(torch.ones_like(amax), e).float().unsqueeze(-1)
    lim = FMAX[fmt]
    vals = torch.clamp(blocks * scale, -lim, lim).to(_torch_dtype(fmt)).float() / scale
    return vals.flatten(-2)[..., :n], (127 - e).to(torch.uint8)


def mx_quantize(t, fmt: int):
    """(q [R][C], sq, qT [C][R], sqT) of the bf16 CUDA matrix ``t`` [R][C] (plx_mxfp8_cast, one read): uint8 FP8 bytes
    with blocks along C, their scale words ``sq`` uint8 [ceil(C / 128)][R][4] (byte j of word [kt][r]: K-block
    4 kt + j, 127 past the end), and the transposed copy quantised on its own from the bf16 values, blocks along R,
    with ``sqT`` [ceil(R / 128)][C][4].  R, C multiples of 32."""
    import torch

    from polyaxon_amd.ops import _native

    if (t.dim() != 2 or t.shape[0] % MX_BLOCK or t.shape[1] % MX_BLOCK or not t.is_contiguous() or not t.is_cuda
            or t.dtype != torch.bfloat16 or t.numel() == 0):
        raise ValueError(f"plx_mxfp8_cast takes a contiguous bf16 CUDA [R][C] with R, C multiples of 32, got "
                         f"{tuple(t.shape)} ({t.dtype})")
    R, C = t.shape
    q = torch.empty(R, C, dtype=torch.uint8, device=t.device)
    qt = torch.empty(C, R, dtype=torch.uint8, device=t.device)
    sq = torch.empty((C + 127) // 128, R, 4, dtype=torch.uint8, device=t.device)
    sqt = torch.empty((R + 127) // 128, C, 4, dtype=torch.uint8, device=t.device)
    _native.check(_native.lib("plx_gemm_mxfp8").plx_mxfp8_cast(
        t.data_ptr(), q.data_ptr(), sq.data_ptr(), qt.data_ptr(), sqt.data_ptr(), R, C, _fmt(fmt),
        _native.current_stream()), "plx_mxfp8_cast")
    return q, sq, qt, sqt


def mx_gemm(a, a_fmt: int, sa, b, sb, M: int, N: int, K: int, out=None, accumulate: bool = False, alpha: float = 1.0,
            bias=None, gelu_out=None):
    """out[M][N] (bf16, unit column stride) = alpha * (A 2^(sa - 127)) . (B 2^(sb - 127))^T (+ bias) (+ out): ``a``
    FP8 bytes [M][K] of format ``a_fmt``, ``b`` E4M3 bytes [N][K], both contiguous uint8; ``sa`` / ``sb`` their scale
    words as :func:`mx_quantize` lays them out, [ceil(K / 128)][rows][4] uint8.  ``bias`` [N] is added in fp32 (not
    with ``accumulate``); ``gelu_out``, laid out like ``out``, also receives gelu_tanh(out)."""
    import torch

    from polyaxon_amd.ops import _native

    if not mx_supported(M, N, K):
        raise ValueError(f"the MXFP8 GEMM needs M, N multiples of 16 and K a multiple of 32 (got {M}x{N}x{K})")
    for x, s, rows in ((a, sa, M), (b, sb, N)):
        if x.dtype != torch.uint8 or not x.is_contiguous() or x.numel() != rows * K:
            raise ValueError("the MXFP8 GEMM takes contiguous uint8 operands of M x K and N x K bytes")
        if (s.dtype != torch.uint8 or not s.is_contiguous() or s.numel() != (K + 127) // 128 * rows * 4
                or s.device != x.device or s.data_ptr() % 4):
            raise ValueError("sa / sb are contiguous uint8 [ceil(K / 128)][rows][4] scale words on the operands' device")
    if out is None:
        if accumulate:
            raise ValueError("accumulate needs out")
        out = torch.empty(M, N, dtype=torch.bfloat16, device=a.device)
    if (out.dtype != torch.bfloat16 or out.dim() != 2 or out.shape != (M, N) or out.stride(1) != 1
            or out.stride(0) % 8 or out.data_ptr() % 16):
        raise ValueError("out must be a 16-byte aligned [M][N] bf16 matrix with unit column stride and a row stride "
                         "that is a multiple of 8")
    if bias is not None:
        if accumulate or bias.numel() != N:
            raise ValueError("bias needs numel N and no accumulate")
        bias = bias.to(torch.float32).contiguous()
        if bias.data_ptr() % 16:
            bias = bias.clone()
    if gelu_out is not None and (accumulate or gelu_out.dtype != torch.bfloat16 or gelu_out.shape != out.shape
                                 or gelu_out.stride() != out.stride() or gelu_out.data_ptr() % 16):
        raise ValueError("gelu_out must be a bf16 tensor laid out like out (and no accumulate)")
    floats = _native.size("plx_gemm_mxfp8", "plx_gemm_mxfp8_ws", M, N, K)
    ws = _workspace(a.device, floats).data_ptr() if floats else None
    rc = _native.lib("plx_gemm_mxfp8").plx_gemm_mxfp8(
        a.data_ptr(), sa.data_ptr(), b.data_ptr(), sb.data_ptr(), out.data_ptr(), ws, M, N, K, K, K, out.stride(0),
        _fmt(a_fmt), float(alpha), int(accumulate), bias.data_ptr() if bias is not None else None,
        gelu_out.data_ptr() if gelu_out is not None else None, _native.current_stream())
    if rc != 0:
        raise RuntimeError(f"plx_gemm_mxfp8 failed ({rc}) for {M}x{N}x{K}")
    return out


def mx_linear_supported(x, weight) -> bool:
    """Do the three GEMMs of ``linear(x, weight)`` run on the MXFP8 kernel?  bf16 CUDA tensors, a contiguous weight,
    tokens, in and out multiples of 32 (each of them is the blocked K of one GEMM)."""
    import torch

    if not (x.is_cuda and x.dtype == torch.bfloat16 and weight.dtype == torch.bfloat16 and weight.is_contiguous()):
        return False
    T, (fout, fin) = x.numel() // max(x.shape[-1], 1), weight.shape
    return x.shape[-1] == fin and min(T, fin, fout) > 0 and T % MX_BLOCK == 0 and fin % MX_BLOCK == 0 \
        and fout % MX_BLOCK == 0
